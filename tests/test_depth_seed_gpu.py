"""segs_depth_seed on the device against the float32 reference of tests/_depth_seed_ref.py -- counts, n_new and the new anchor
rows bit for bit (a mismatch is a finding about the order of operations, never grounds for a tolerance) -- and the seeding
through ScaffoldTrainerStep.seed_keyframe."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import _depth_seed_ref as ref  # noqa: E402

DEV = "cuda:0"
SENTINEL = -12345.5
SEGS_ERR_INVALID_ARGUMENT = -1


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def device_seed(anchor, target, depth, alpha, M, p, max_new=None, tanfov=ref.TANFOV, rows=None, check=True):
    """One call of the C entry point.  -> (status, counts[6], n_new, the whole (rows, 3) output buffer pre-filled with SENTINEL)."""
    from segs_slam_amd import _capi
    lib = _capi.lib()
    H, W = target.shape
    n_lat = len(ref.lattice(H, W, p.stride)[0])
    max_new = n_lat if max_new is None else max_new
    rows = max(max_new, n_lat, 1) if rows is None else rows
    A = len(anchor)
    d_anchor, d_target, d_depth, d_alpha = _t(anchor.astype(np.float32)) if A else None, _t(target), _t(depth), _t(alpha)
    out = torch.full((rows, 3), SENTINEL, dtype=torch.float32, device=DEV)
    words = torch.full((8,), -7, dtype=torch.int32, device=DEV)
    temp = torch.empty(max(lib.segs_depth_seed_temp_bytes(A, H, W, p.stride), 256), dtype=torch.uint8, device=DEV)
    cp = _capi.DepthSeedParamsC(p.stride, p.alpha_max, int(p.use_front), p.front_abs, p.front_rel, p.voxel_size)
    cm = (C.c_float * 16)(*np.asarray(M, dtype=np.float32).reshape(-1).tolist())
    st = lib.segs_depth_seed(A, _ptr(d_anchor), H, W, _ptr(d_target), _ptr(d_depth), _ptr(d_alpha), tanfov[0], tanfov[1], cm,
                             C.byref(cp), max_new, _ptr(out), C.c_void_p(words.data_ptr() + 24), _ptr(words), _ptr(temp),
                             C.c_void_p(torch.cuda.current_stream().cuda_stream))
    if check:
        _capi.check(st, "segs_depth_seed")
    torch.cuda.synchronize()
    w = words.cpu().numpy()
    return st, w[:6].tolist(), int(w[6]), out.cpu().numpy()


def assert_matches(got, want, max_new=None):
    _, counts, n_new, out = got
    assert counts == want["counts"], (counts, want["counts"])
    assert n_new == want["n_new"]
    k = n_new if max_new is None else min(n_new, max_new)
    assert np.array_equal(out[:k].view(np.uint32), want["new_anchor"][:k].view(np.uint32))
    assert np.all(out[k:] == np.float32(SENTINEL))            # nothing behind the rows that were due


_SHAPES = [(hw, s) for hw in ref.SIZES for s in ref.STRIDES] + ref.SMALL


@pytest.mark.parametrize("shape", _SHAPES, ids=lambda s: f"{s[0][1]}x{s[0][0]}-stride{s[1]}")
def test_synthetic_maps_match_the_reference_bit_for_bit(shape):
    (H, W), stride = shape
    cases = [c for c in ref.synthetic_cases() if (c["H"], c["W"], c["p"].stride) == (H, W, stride)]
    assert len(cases) == len(ref.ANCHOR_COUNTS) * 2
    from segs_slam_amd import _capi
    lib = _capi.lib()
    for c in cases:
        M = ref.cam_to_world(c["view"])
        # the target goes through segs_depth_target, as in the step
        z = _t(c["sensor"])
        block = torch.empty(int(lib.segs_depth_target_floats(H, W)), dtype=torch.float32, device=DEV)
        _capi.check(lib.segs_depth_target(_ptr(z), H, W, ref.MIN_DEPTH, ref.MAX_DEPTH, _ptr(block),
                                          C.c_void_p(torch.cuda.current_stream().cuda_stream)), "segs_depth_target")
        target = block[:H * W].view(H, W).cpu().numpy()
        assert np.array_equal(target.view(np.uint32), c["target"].view(np.uint32))
        want = ref.seed(c["anchor"], target, c["depth"], c["alpha"], *ref.TANFOV, M, c["p"])
        print(f"{W}x{H} stride {stride} A {c['A']} use_front {c['p'].use_front}: counts {want['counts']}")
        assert_matches(device_seed(c["anchor"], target, c["depth"], c["alpha"], M, c["p"]), want)
        # and without a render: every valid lattice pixel is a candidate
        want0 = ref.seed(c["anchor"], target, None, None, *ref.TANFOV, M, c["p"])
        assert want0["counts"][1] == want0["counts"][0] and want0["counts"][2] == 0
        assert_matches(device_seed(c["anchor"], target, None, None, M, c["p"]), want0)


def _plane(H, W, z=2.0):
    return np.full((H, W), z, dtype=np.float32)


def test_runs_longer_than_a_workgroup_and_a_whole_image_in_one_voxel():
    H, W = 48, 64                                     # 3072 lattice pixels at stride 1
    M = np.eye(4, dtype=np.float32)                   # fronto-parallel: the plane z = 2 spans 2.28 x 1.72 m
    target = _plane(H, W)
    none = np.zeros((0, 3), np.float32)
    p = ref.Params(stride=1, voxel_size=1.0)
    want = ref.seed(none, target, None, None, *ref.TANFOV, M, p)
    sizes = np.unique(np.rint(_world(target, M, p) / np.float32(1.0)), axis=0, return_counts=True)[1]
    assert sizes.max() > 256 and len(sizes) > 1        # a run longer than a workgroup, next to others
    assert_matches(device_seed(none, target, None, None, M, p), want)
    p = ref.Params(stride=1, voxel_size=8.0)
    want = ref.seed(none, target, None, None, *ref.TANFOV, M, p)
    assert want["counts"] == [H * W, H * W, 0, 0, 1, 1]
    assert_matches(device_seed(none, target, None, None, M, p), want)
    assert_matches(device_seed(np.array([[0.5, -1.0, 3.0]], np.float32), target, None, None, M, p),
                   dict(counts=[H * W, H * W, 0, 0, 1, 0], n_new=0, new_anchor=np.zeros((0, 3), np.float32)))


def _world(target, M, p):
    """float32 world points of every lattice pixel of an all-valid target (the reference's arithmetic)."""
    H, W = target.shape
    u, v = ref.lattice(H, W, p.stride)
    f = np.float32
    Z = target[v, u]
    xv = ((2 * u + 1).astype(f) / f(W) - f(1)) * f(ref.TANFOV[0]) * Z
    yv = ((2 * v + 1).astype(f) / f(H) - f(1)) * f(ref.TANFOV[1]) * Z
    return np.stack([((xv * M[0, d] + yv * M[1, d]) + Z * M[2, d]) + M[3, d] for d in range(3)], axis=1)


def test_existing_anchors_block_exactly_their_voxels():
    c = next(c for c in ref.synthetic_cases() if (c["H"], c["W"], c["p"].stride, c["A"], c["p"].use_front) == (48, 64, 2, 0, True))
    M, p = ref.cam_to_world(c["view"]), c["p"]
    args = (c["target"], c["depth"], c["alpha"], M, p)
    _, counts, n_new, out = device_seed(c["anchor"], *args)
    assert n_new == counts[4] > 20
    first = out[:n_new]
    # seed, append, seed the same maps again
    _, counts2, n_new2, out2 = device_seed(first, *args)
    assert n_new2 == 0 and counts2 == counts[:5] + [0] and np.all(out2 == np.float32(SENTINEL))
    # anchors placed by hand (off-centre, in shuffled order) in every second candidate voxel remove exactly those
    rng = np.random.default_rng(5)
    jitter = (rng.random((len(first[::2]), 3)).astype(np.float32) - np.float32(0.5)) * np.float32(0.8 * p.voxel_size)
    by_hand = (first[::2] + jitter)[rng.permutation(len(jitter))]
    assert set(map(tuple, ref.anchor_voxels(by_hand, p.voxel_size).tolist())) == set(map(tuple, ref.anchor_voxels(first[::2], p.voxel_size).tolist()))
    _, counts3, n_new3, out3 = device_seed(by_hand, *args)
    assert counts3[:5] == counts[:5] and n_new3 == n_new - len(by_hand)
    assert np.array_equal(out3[:n_new3].view(np.uint32), first[1::2].view(np.uint32))


def test_max_new_below_the_count():
    c = next(c for c in ref.synthetic_cases() if (c["H"], c["W"], c["p"].stride, c["A"], c["p"].use_front) == (48, 64, 2, 257, False))
    M = ref.cam_to_world(c["view"])
    want = ref.seed(c["anchor"], c["target"], c["depth"], c["alpha"], *ref.TANFOV, M, c["p"])
    assert want["n_new"] > 40
    for max_new in (0, 1, 37, want["n_new"] - 1, want["n_new"]):
        got = device_seed(c["anchor"], c["target"], c["depth"], c["alpha"], M, c["p"], max_new=max_new, rows=want["n_new"] + 8)
        assert got[2] == want["n_new"] and got[1][5] == want["n_new"]        # the full count
        assert_matches(got, want, max_new=max_new)


def test_no_candidates_and_a_single_null_map():
    H, W = 17, 33
    M = ref.cam_to_world(ref.rotated_view())
    p = ref.Params(stride=2, use_front=True)
    target, alpha = _plane(H, W), np.ones((H, W), np.float32)
    depth = target.copy()                             # D / A == Z: nothing in front
    n_lat = len(ref.lattice(H, W, 2)[0])
    st, counts, n_new, out = device_seed(np.zeros((0, 3), np.float32), target, depth, alpha, M, p)
    assert counts == [n_lat, 0, 0, 0, 0, 0] and n_new == 0 and np.all(out == np.float32(SENTINEL))
    st, counts, n_new, out = device_seed(np.zeros((0, 3), np.float32), np.zeros((H, W), np.float32), depth, alpha, M, p)
    assert counts == [0] * 6 and n_new == 0 and np.all(out == np.float32(SENTINEL))
    for d, a in ((depth, None), (None, alpha)):
        st, counts, n_new, out = device_seed(np.zeros((0, 3), np.float32), target, d, a, M, p, check=False)
        assert st == SEGS_ERR_INVALID_ARGUMENT
        assert counts == [-7] * 6 and n_new == -7 and np.all(out == np.float32(SENTINEL))     # nothing was launched


def test_out_of_range_voxels_are_dropped_and_counted():
    H, W = 17, 33
    view = ref.rotated_view()
    M = ref.cam_to_world(view)
    p = ref.Params(stride=1, voxel_size=0.01)
    z, depth, alpha = ref.maps(H, W, seed=77)
    target = ref.depth_target(z, ref.MIN_DEPTH, ref.MAX_DEPTH)
    # move the camera so that the 2^20-th voxel boundary along x (10485.76 m at 1 cm) cuts through the back-projected points
    w = _world(np.where(target > 0, target, np.float32(2.0)), M, p)
    M2 = M.copy()
    M2[3, 0] += np.float32(10485.76) - np.float32(np.median(w[:, 0]))
    want = ref.seed(np.zeros((0, 3), np.float32), target, depth, alpha, *ref.TANFOV, M2, p)
    assert want["counts"][3] > 10 and want["counts"][4] > 10, want["counts"]
    assert want["new_voxels"][:, 0].max() == ref.KEY_BIAS - 1     # the last voxel inside is used, the first outside is not clamped into it
    assert_matches(device_seed(np.zeros((0, 3), np.float32), target, depth, alpha, M2, p), want)
    M3 = M.copy()
    M3[3, 1] -= np.float32(10485.76) + np.float32(np.median(w[:, 1]))     # and the lower edge, -2^20, which is inside
    want = ref.seed(np.zeros((0, 3), np.float32), target, depth, alpha, *ref.TANFOV, M3, p)
    assert want["counts"][3] > 10 and want["counts"][4] > 10 and want["new_voxels"][:, 1].min() == -ref.KEY_BIAS
    assert_matches(device_seed(np.zeros((0, 3), np.float32), target, depth, alpha, M3, p), want)


def test_two_calls_give_identical_bytes():
    c = next(c for c in ref.synthetic_cases() if (c["H"], c["W"], c["p"].stride, c["A"], c["p"].use_front) == (48, 64, 1, 5000, True))
    M = ref.cam_to_world(c["view"])
    a = device_seed(c["anchor"], c["target"], c["depth"], c["alpha"], M, c["p"])
    b = device_seed(c["anchor"], c["target"], c["depth"], c["alpha"], M, c["p"])
    assert a[1] == b[1] and a[2] == b[2] and a[3].tobytes() == b[3].tobytes() and a[2] > 100


# ---- through the step ------------------------------------------------------------------------------------------------
W_STEP, H_STEP, Z_PLANE = 64, 48, 3.0


def _step(graph, A=2000, voxel_size=0.01):
    from segs_slam_amd import mapper_config as mc, neural_gaussians as ng, scenes
    from segs_slam_amd.densify import DepthSeedParams
    dev = torch.device(DEV)
    cfg = mc.load_committed_config("cfg/gaussian_mapper/RGB-D/Replica/office0.yaml")
    cfg.densify.update_until = 0                      # no adjust_anchor in these few iterations: seeding is the only growth
    cfg.densify.voxel_size = voxel_size
    cam = scenes.make_camera(W_STEP, H_STEP, 60.0, 60.0, np.eye(3, dtype=np.float32), np.zeros(3, dtype=np.float32))
    model = ng.synthetic_model(max(A, 1), cfg.model, cam, dev, seed=11)
    if A > 0:
        with torch.no_grad():                         # the map covers the left half of the view only
            a = model.param("anchor")
            a[:, 0] = -a[:, 0].abs() - 0.05 * a[:, 2]
    else:
        model.A = 0
    step = mc.make_mapper_step(cfg, model, W_STEP, H_STEP, depth_seed=DepthSeedParams(stride=2, alpha_max=0.5))
    step.enable_graph(graph)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    kf = ng.Keyframe(t(cam.world_view_transform), t(cam.full_proj_transform), t(cam.camera_center),
                     torch.tensor([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0], device=dev), cam.tanfovx, cam.tanfovy)
    gt = torch.rand(3, H_STEP, W_STEP, generator=torch.Generator().manual_seed(2)).to(dev)
    depth = torch.full((H_STEP, W_STEP), Z_PLANE, dtype=torch.float32, device=dev)
    return step, kf, gt, depth


def _pixels_of(anchor, kf):
    """The pixel every anchor projects into with the keyframe's full projection (the rasterizer's ndc2Pix, rounded)."""
    a = anchor.double().cpu().numpy()
    P = kf.proj.double().cpu().numpy()
    h = np.concatenate([a, np.ones((len(a), 1))], axis=1) @ P
    ndc = h[:, :2] / h[:, 3:4]
    px = ((ndc[:, 0] + 1) * W_STEP - 1) * 0.5
    py = ((ndc[:, 1] + 1) * H_STEP - 1) * 0.5
    return np.rint(px).astype(int), np.rint(py).astype(int), px, py


def _seed_sequence(graph):
    step, kf, gt, depth = _step(graph)
    m = step.model
    assert step.engine.render_depth and step.anchors_frozen()
    losses = [float(step.training_once([kf], [gt])) for _ in range(3)]       # a map in use: calibrated, moments non-zero
    A0 = m.A
    counts = step.seed_keyframe(kf, depth)
    alpha = step.engine.out_alpha.cpu().numpy().copy()                        # the render the seeding read
    assert counts["new anchors"] > 50 and m.A == A0 + counts["new anchors"]
    assert counts["valid lattice pixels"] == (H_STEP // 2) * (W_STEP // 2)
    assert counts["unobserved"] >= counts["distinct voxels"] >= counts["new anchors"] and counts["in front"] == 0
    new = m.param("anchor")[A0:].clone()
    ix, iy, px, py = _pixels_of(new, kf)
    assert np.all((ix >= 0) & (ix < W_STEP) & (iy >= 0) & (iy < H_STEP))
    assert np.all(alpha[iy, ix] < 0.5)                                        # only where the map rendered less than alpha_max
    assert np.all(ix % 2 == 1) and np.all(iy % 2 == 1)                        # the lattice pixels of stride 2
    assert np.abs(px - ix).max() < 0.25 and np.abs(py - iy).max() < 0.25     # (1 cm voxels: within a quarter pixel of the centre)
    # the quarter of the view farthest from the map is seeded at every lattice pixel; the map's own side is not
    assert int((ix >= 3 * W_STEP // 4).sum()) == (W_STEP // 8) * (H_STEP // 2)
    assert counts["unobserved"] < counts["valid lattice pixels"]
    print(f"seed_keyframe (graph {graph}): A {A0} -> {m.A}, counts {counts}")
    # the rows _append writes
    no = m.dims.n_offsets
    for bucket in (m.exp_avg, m.exp_avg_sq, m.grads):
        for name in m.widths:
            assert not bool(m._view(bucket, name)[A0:].any())
    for name in step.densifier.STAT_NAMES:
        n0 = A0 if name in ("opacity_accum", "anchor_demon") else A0 * no
        assert not bool(step.densifier.stat(name)[n0:].any())
    assert not bool(m.param("offset")[A0:].any()) and not bool(m.param("anchor_feat")[A0:].any())
    assert torch.equal(m.param("scaling")[A0:], torch.full_like(m.param("scaling")[A0:], float(np.log(np.float32(0.01)))))
    again = step.seed_keyframe(kf, depth)
    assert again["new anchors"] == 0 and m.A == A0 + counts["new anchors"]
    losses += [float(step.training_once([kf], [gt])) for _ in range(4)]
    # after training the map covers other pixels than before, so a later call may seed again -- but never a voxel that holds
    # an anchor: the frozen anchors of the first seeding still block theirs
    A1 = m.A
    final = step.seed_keyframe(kf, depth)
    assert m.A == A1 + final["new anchors"] and final["new anchors"] <= final["unobserved"]
    vox = ref.anchor_voxels(m.param("anchor").cpu().numpy(), 0.01)
    assert len(np.unique(vox[A0:], axis=0)) == m.A - A0                        # every seeded anchor has a voxel of its own
    assert not set(map(tuple, vox[A0:].tolist())) & set(map(tuple, vox[:A0].tolist()))
    step.finish()
    torch.cuda.synchronize()
    assert step.dropped_steps() == step.redone_steps
    return step, losses, counts, new.cpu().numpy()


def test_seed_keyframe_through_the_step_eager_and_captured():
    se, le, ce, ne = _seed_sequence(False)
    assert np.isfinite(le).all() and bool(torch.isfinite(se.model.params).all())
    sg, lg, cg, ng_ = _seed_sequence(True)
    # the standard of tests/test_graph_step_gpu.py around adjust_anchor: replay resumes at the new size, nothing is dropped,
    # losses agree to 1e-3 (atomics noise through Adam), everything stays finite; the seeding itself is deterministic
    assert np.isfinite(lg).all() and bool(torch.isfinite(sg.model.params).all())
    assert se.graph_replays == 0 and sg.graph_replays >= 4
    assert sg._mlp_count.value() == 7 == se._mlp_count.value() and sg.dropped_steps() == 0
    np.testing.assert_allclose(lg, le, rtol=1e-3)
    np.testing.assert_allclose(lg[:3], le[:3], rtol=1e-5)


def test_seed_keyframe_starts_a_map_from_the_frame_alone():
    step, kf, gt, depth = _step(False, A=0)
    assert step.model.A == 0
    counts = step.seed_keyframe(kf, depth)
    n_lat = (H_STEP // 2) * (W_STEP // 2)
    assert counts["valid lattice pixels"] == counts["unobserved"] == n_lat
    assert counts["new anchors"] == counts["distinct voxels"] == step.model.A > 0.9 * n_lat
    a = step.model.param("anchor")
    assert float((a[:, 2] - Z_PLANE).abs().max()) <= 0.005 + 1e-6            # the plane, to half a voxel
    ix, iy, _, _ = _pixels_of(a, kf)
    assert len(set(zip(ix.tolist(), iy.tolist()))) == step.model.A             # one anchor per lattice pixel it came from
    losses = [float(step.training_once([kf], [gt])) for _ in range(2)]
    assert np.isfinite(losses).all()
    assert step.seed_keyframe(kf, depth)["new anchors"] == 0
