"""simple-knn / operate_points / stereo_vision: oracle sanity on CPU, bit-exact parity on the GPU."""
import numpy as np
import pytest
import torch

from oracle import gs_oracle

DEV = "cuda:0"


def _pts(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, 3)) * np.array([2.0, 1.0, 0.5])).astype(np.float32)


# the O(P^2) brute-force oracle takes 2.9 s at 65 537 points and 12.1 s at 131 072 on an 8-core host: above this size the
# float64 k-d-tree candidate oracle below takes over
BRUTE_MAX = 120_000


def knn_candidates_oracle(p, k=16):
    """gs_oracle.knn_mean_dist2 restricted to the k float64-nearest neighbours of every point (scipy's cKDTree): the float32
    arithmetic of the oracle -- (dx*dx + dy*dy) + dz*dz with dx = neighbour - query, no contraction, the three smallest
    kept in ascending order, (b0 + b1) + b2, / 3.0f.  Exact as long as the three smallest float32 distances are among the k
    nearest in float64, which only a run of more than k - 3 float64 ties could break; needs P > k."""
    from scipy.spatial import cKDTree
    P = p.shape[0]
    p64 = p.astype(np.float64)
    _, idx = cKDTree(p64).query(p64, k=k + 1)
    d = p[idx] - p[:, None, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    d2[idx == np.arange(P)[:, None]] = np.inf         # the point itself (by index: duplicates of it stay candidates)
    b = np.sort(d2, axis=1)[:, :3]
    return ((b[:, 0] + b[:, 1]) + b[:, 2]) / np.float32(3.0)


def knn_oracle(p):
    """Mean squared 3-NN distance like the reference: brute force up to BRUTE_MAX points, the candidate oracle above (brute
    force again where scipy is missing)."""
    p = np.ascontiguousarray(p, dtype=np.float32)
    if p.shape[0] > BRUTE_MAX:
        try:
            return knn_candidates_oracle(p)
        except ImportError:
            pass
    return gs_oracle.knn_mean_dist2(p)


def depth_surface_points(width, height, f, seed):
    """A dense synthetic depth map back-projected through a pinhole (f px, principal point at the centre): a wavy wall about
    0.6 m away, so that neighbouring pixels lie under 1 mm apart."""
    rng = np.random.default_rng(seed)
    u, v = np.meshgrid(np.arange(width, dtype=np.float64), np.arange(height, dtype=np.float64))
    z = 0.6 + 0.04 * np.sin(u / 37.0) * np.cos(v / 23.0) + 0.0005 * rng.random(u.shape)
    x, y = (u - width / 2) / f * z, (v - height / 2) / f * z
    return np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1).astype(np.float32)


def test_knn_candidate_oracle_matches_brute_force():
    """The candidate oracle the GPU tests use above BRUTE_MAX equals the brute-force one bit for bit at 65 537 points, on a
    plain cloud, on a cloud of duplicated points and on a 1-mm lattice (many equal distances)."""
    rng = np.random.default_rng(7)
    plain = _pts(65_537, 3)
    dup = np.concatenate([plain[:32_768], plain[:32_769]])
    lattice = (rng.integers(-40, 40, (65_537, 3)) * np.float32(0.001)).astype(np.float32)
    lattice = np.unique(lattice, axis=0)
    for name, p in (("plain", plain), ("duplicated", dup), ("lattice", lattice)):
        got, ref = knn_candidates_oracle(p), gs_oracle.knn_mean_dist2(p)
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), name


def test_knn_oracle_against_kdtree():
    from scipy.spatial import cKDTree
    p = _pts(3000, 1)
    got = gs_oracle.knn_mean_dist2(p)
    d, _ = cKDTree(p.astype(np.float64)).query(p.astype(np.float64), k=4)
    ref = (d[:, 1:] ** 2).mean(axis=1)
    assert np.allclose(got, ref, rtol=1e-5, atol=1e-9)
    # duplicates: a duplicated point has nearest distance 0
    q = np.concatenate([p[:10], p[:10]])
    assert np.all(gs_oracle.knn_mean_dist2(q)[:10] <= gs_oracle.knn_mean_dist2(p[:10]) + 1e-6)


def test_quaternion_transform_oracle_is_rotation_composition():
    rng = np.random.default_rng(2)
    q = rng.standard_normal((50, 4)).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    ang = 0.7
    Rz = np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]], dtype=np.float32)
    M = np.eye(4, dtype=np.float32)
    M[:3, :3] = Rz
    M[:3, 3] = [0.1, -0.2, 0.3]
    Mt = np.ascontiguousarray(M.T)  # transposed layout, auxiliary.h:59-67
    p = _pts(50, 3)
    out_p, out_r = gs_oracle.scale_and_transform_points(p, q, Mt, np.ones(50, np.uint8), 2.0)
    assert np.allclose(out_p, (2.0 * p) @ Rz.T + M[:3, 3], atol=1e-5)
    # (w, x) of the composed rotation are right; slot 2 holds z and slot 3 stays 0 (the reference's insert_rot_to_rots quirk)
    def quat_to_R(w, x, y, z):
        return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                         [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                         [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    for i in range(50):
        Rn = Rz @ quat_to_R(*q[i])
        w = 0.5 * np.sqrt(max(1e-12, 1 + np.trace(Rn)))
        if np.trace(Rn) > 0:
            assert abs(out_r[i, 0] - w) < 1e-4
            assert abs(out_r[i, 1] - (Rn[2, 1] - Rn[1, 2]) / (4 * w)) < 1e-4
            assert abs(out_r[i, 2] - (Rn[1, 0] - Rn[0, 1]) / (4 * w)) < 1e-4
        assert out_r[i, 3] == 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("n", [5, 1000, 20000])
def test_dist2_gpu_bit_exact(n):
    from segs_slam_amd import points as sp
    p = _pts(n, n)
    got = sp.distCUDA2(torch.from_numpy(p).to(DEV)).cpu().numpy()
    ref = gs_oracle.knn_mean_dist2(p)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))


def _dist2_bit_exact(p):
    from segs_slam_amd import points as sp
    got = sp.distCUDA2(torch.from_numpy(np.ascontiguousarray(p)).to(DEV)).cpu().numpy()
    ref = knn_oracle(p)
    bad = np.flatnonzero(got.view(np.uint32) != ref.view(np.uint32))
    assert bad.size == 0, (p.shape[0], bad.size, bad[:5], got[bad[:5]], ref[bad[:5]])
    return got


# around the 256-point box (one workgroup / LDS tile) and the 256-boxes-per-round candidate test of knn_query_kernel:
# 65 537 and 65 793 points make 257 and 258 boxes, the first sizes that need a second round; P < 4 leaves FLT_MAX in the
# best-three list (a mean of ~1.1e38 at P = 3, inf at P <= 2, as in the reference)
@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 3, 4, 255, 256, 257, 65_535, 65_536, 65_537, 65_793, 200_003])
def test_dist2_gpu_bit_exact_across_box_rounds(n):
    got = _dist2_bit_exact(_pts(n, 100 + n))
    if n == 3:
        assert 1e38 < got.min() and np.isfinite(got).all()
    elif n <= 2:
        assert np.isinf(got).all()


DEGENERATE = {"duplicated": 41, "planar_z0": 42, "collinear": 43, "far_cluster": 44, "two_clusters": 45}


def _degenerate_cloud(shape):
    rng = np.random.default_rng(DEGENERATE[shape])
    if shape == "duplicated":                       # every point twice: nearest distance 0
        p = _pts(32_769, DEGENERATE[shape])
        return np.concatenate([p, p[::-1]])
    if shape == "planar_z0":                        # z == 0 exactly: zero extent on that axis, Morton coordinate 0/0
        p = _pts(65_537, DEGENERATE[shape])
        p[:, 2] = 0.0
        return p
    if shape == "collinear":                        # one line through the origin, regularly spaced with jitter
        t = (np.arange(65_793) - 30_000) * 1e-3 + rng.random(65_793) * 1e-4
        return (t[:, None] * np.array([0.6, -0.48, 0.64])).astype(np.float32)
    if shape == "far_cluster":                      # the bounding box holds the origin: Morton order degenerates, nearly every
        p = rng.standard_normal((65_537, 3)) * 0.05 + np.array([50.0, 50.0, 50.0])      # box is a candidate of every other
        return p.astype(np.float32)
    if shape == "two_clusters":
        a = rng.standard_normal((40_000, 3)) * 0.3 + np.array([-20.0, 0.0, 5.0])
        b = rng.standard_normal((30_003, 3)) * 0.2 + np.array([30.0, 10.0, -40.0])
        return np.concatenate([a, b]).astype(np.float32)
    raise KeyError(shape)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", sorted(DEGENERATE))
def test_dist2_gpu_bit_exact_on_degenerate_clouds(shape):
    p = _degenerate_cloud(shape)
    got = _dist2_bit_exact(p)
    if shape == "duplicated":                       # point i and point P-1-i coincide
        assert np.array_equal(got, got[::-1]) and float(got.min()) > 0.0


@pytest.mark.gpu
def test_dist2_gpu_bit_exact_on_millimetre_voxel_centres():
    """distCUDA2 of the 1-mm voxel centres of a dense depth surface, as createFromPcd makes them (anchors_from_points): a
    lattice surface of more than 65 536 points with many equal distances; the log-scales built from it follow."""
    from segs_slam_amd import neural_gaussians as ng
    pts = torch.from_numpy(depth_surface_points(480, 360, 700.0, 12)).to(DEV)
    fused, scaling = ng.anchors_from_points(pts, 0.001)
    u = fused.cpu().numpy()
    assert u.shape[0] > 65_536
    d2 = _dist2_bit_exact(u)
    ref = torch.log(torch.sqrt(torch.from_numpy(d2).clamp_min(0.0000001))).unsqueeze(1).repeat(1, 6)
    assert torch.allclose(scaling.cpu(), ref, rtol=1e-6, atol=1e-6)


@pytest.mark.gpu
def test_operate_points_gpu_bit_exact():
    from segs_slam_amd import points as sp
    from segs_slam_amd import scenes
    sc = scenes.make_scene(5000, 320, 240, 250.0, 250.0, seed=8)
    cam = sc.camera
    rng = np.random.default_rng(4)
    A = rng.standard_normal((3, 3))
    Q, _ = np.linalg.qr(A)
    M = np.eye(4, dtype=np.float32)
    M[:3, :3] = Q.astype(np.float32)
    M[:3, 3] = [0.05, 0.02, -0.03]
    Mt = np.ascontiguousarray(M.T)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    out = sp.transformPoints(t(sc.means3D), t(Mt)).cpu().numpy()
    assert np.array_equal(out.view(np.uint32), gs_oracle.transform_points(sc.means3D, Mt).view(np.uint32))
    # scaleAndTransformThenMarkVisiblePoints
    ntm = rng.random(sc.P) < 0.7
    unst = rng.random(sc.P) < 0.8
    pts, rots, m1 = t(sc.means3D), t(sc.rotations), torch.from_numpy(ntm).to(DEV)
    n = sp.scaleAndTransformThenMarkVisiblePoints(pts, rots, m1, torch.from_numpy(unst).to(DEV), t(Mt),
                                                  t(cam.world_view_transform), t(cam.full_proj_transform), 3, 1.5)
    present = gs_oracle.mark_visible(sc.means3D, cam.world_view_transform, cam.full_proj_transform)
    final = ntm & unst & present
    assert n == 3 + int(final.sum())
    rp, rr = gs_oracle.scale_and_transform_points(sc.means3D, sc.rotations, Mt, final.astype(np.uint8), 1.5)
    exp_p, exp_r = sc.means3D.copy(), sc.rotations.copy()
    exp_p[final], exp_r[final] = rp[final], rr[final]
    assert np.array_equal(pts.cpu().numpy().view(np.uint32), exp_p.view(np.uint32))
    assert np.array_equal(rots.cpu().numpy().view(np.uint32), exp_r.view(np.uint32))
    assert np.array_equal(m1.cpu().numpy(), ntm & ~final)


@pytest.mark.gpu
def test_stereo_vision_gpu_bit_exact():
    from segs_slam_amd import points as sp
    rng = np.random.default_rng(9)
    W, H = 64, 48
    depth = (rng.random(W * H) * 5 + 0.2).astype(np.float32)
    mask = rng.random(W * H) < 0.6
    intr = [60.5, 61.25, 31.7, 23.9]
    got = sp.reprojectDepthPinhole(torch.from_numpy(depth).to(DEV), torch.from_numpy(mask).to(DEV), intr, W).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), gs_oracle.reproject_depths_pinhole(depth, mask, intr, W).view(np.uint32))
    N = 700
    px = np.stack([rng.integers(0, W, N), rng.integers(0, H, N)], axis=1).astype(np.float32)
    has3d = rng.random(N) < 0.4
    p3 = np.concatenate([rng.standard_normal((N, 2)), rng.random((N, 1)) * 4 + 0.3], axis=1).astype(np.float32)
    colors = rng.random(W * H + 3).astype(np.float32)
    rp, rc = sp.monocularPinholeInactiveGeoDensifyBySearchingNeighborhoodKeypoints(
        torch.from_numpy(px).to(DEV), torch.from_numpy(has3d).to(DEV), torch.from_numpy(p3).to(DEV),
        torch.from_numpy(colors).to(DEV), 3.0, intr, W)
    op, oc = gs_oracle.search_neighborhood_depth(px, has3d, p3, colors, 3.0, intr, W)
    valid = op[:, 2] > 0
    assert np.array_equal(rp.cpu().numpy().view(np.uint32), op[valid].view(np.uint32))
    assert np.array_equal(rc.cpu().numpy().view(np.uint32), oc[valid].view(np.uint32))
    assert 0 < valid.sum() < N
