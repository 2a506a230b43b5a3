"""The packed per-Gaussian backward (csrc/preprocess.hip: preprocess_bwd_packed_kernel): with the "row written" bytes a workgroup
of at most 64 reached rows lists them and one of its waves runs the projection backward while the other three store the zeros of
the rows not reached; a workgroup with more than 64 keeps a lane per row.  The comparison arm is the same engine under
SEGS_RASTER_UNPACKED_BACKWARD (the kernel that gives every row a lane, with the bytes), in places also
SEGS_RASTER_NO_WRITTEN_BYTES.  The two kernels are callers of ONE projection backward, ONE lane-per-row body and ONE camera fold
(projection_backward_row, preprocess_bwd_rows, camera_fold), so the bit-for-bit tests below pin the packing -- list order, the
slots of the camera fold, the zeros -- and not the arithmetic against a second copy; the arithmetic is held to float64 and to
the oracle by tests/test_raster_gpu.py, test_camera_grad_gpu.py, test_depth_render_gpu.py and test_backward_written_rows_gpu.py.

Against ANOTHER BUILD of the library (the parent commit's, which cannot be built from a checkout of this one) this module runs as
a script, once per library:
    SEGS_RASTER_LIB=/path/to/libsegs_raster.so python -m tests.test_backward_packed_rows_gpu dump a.npz
    python -m tests.test_backward_packed_rows_gpu dump b.npz && python -m tests.test_backward_packed_rows_gpu compare a.npz b.npz
The dump holds the raw bits of every gradient tensor of the scenes whose sums have no atomic-order noise (quadrant_case in its four
forms under flags 0, UNPACKED and NO_WRITTEN_BYTES; blocks_scene under 0 and UNPACKED) and of the stage-alone debug entries on
the same two scenes, with scales and with cov3D_precomp, plain and in the camera form with dL_dz (the body's path without
accumulator rows); compare wants every array equal as int32.  profiles/r09_shared_projection_backward.txt records its result
for the parent of the change that made the three pieces shared.

Scenes, helpers and the noise rule are those of tests/test_backward_written_rows_gpu.py (64x64, at most 2 000 Gaussians): two
backwards of the same inputs differ by the float atomics of the tile backward, so two arms may differ by ten times the largest
difference between two runs of the NO_WRITTEN_BYTES arm plus 1e-5 of the tensor's largest entry.

Where that noise does not exist the arms must agree BIT FOR BIT: in `quadrant_scene` every Gaussian sits on the centre of one 8x8
quadrant with a 3-sigma radius of at most 3 px, so it passes the alpha test only inside that quadrant, one wave of the tile
backward adds into its accumulator row exactly once, and two backwards leave the same accumulator bits."""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest
import torch

from segs_slam_amd import _capi, scenes
from tests.test_backward_written_rows_gpu import (DEV, FOCAL, NO_WRITTEN_BYTES, TENSORS, _t, assert_arena_clean, layered_scene,
                                                  main_case, second_pose)

UNPACKED = 256      # SEGS_RASTER_UNPACKED_BACKWARD (include/segs_raster.h)


def test_flag_value_and_that_the_engine_does_not_take_it_from_the_environment():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "segs_raster.h")) as f:
        assert re.search(r"^#define\s+SEGS_RASTER_UNPACKED_BACKWARD\s+256u\b", f.read(), flags=re.M)
    with open(os.path.join(os.path.dirname(scenes.__file__), "raster_engine.py")) as f:
        assert re.search(r'SEGS_RASTER_EXTRA_FLAGS", "0"\), 0\) & 16\b', f.read())      # still only the one bit


# ---------------------------------------------------------------------------------------------------------------- scenes
def generic_scene(P, w, h, seed, R=None, t=None):
    sc = scenes.make_scene(P, w, h, FOCAL, FOCAL, seed=seed, bg=(0.1, 0.2, 0.3), name="packed")
    cam = scenes.make_camera(w, h, FOCAL, FOCAL, np.eye(3, dtype=np.float32) if R is None else R,
                             np.zeros(3, dtype=np.float32) if t is None else t)
    rng = np.random.default_rng(seed)
    z = (1.5 + 3.0 * rng.random(P)).astype(np.float32)
    sc.means3D[:, 2] = z
    sc.means3D[:, 0] = (rng.random(P) * 2 - 1).astype(np.float32) * 1.3 * z * np.float32(cam.tanfovx)
    sc.means3D[:, 1] = (rng.random(P) * 2 - 1).astype(np.float32) * 1.3 * z * np.float32(cam.tanfovy)
    sc.scales[:] = (0.03 + 0.08 * rng.random((P, 3))).astype(np.float32)
    sc.opacity[:] = (0.3 + 0.69 * rng.random((P, 1))).astype(np.float32)
    dL = rng.standard_normal((3, h, w)).astype(np.float32) / np.float32(3 * h * w)
    return dataclasses.replace(sc, camera=cam, dL_dout_color=dL)


def quadrant_scene(kinds, seed=21, w=64, h=64):
    """One Gaussian per entry of `kinds`, in this order: 'v' visible (opacity 0.2-0.6), 'f' front layer (opacity 0.99, nearest),
    'b' behind the camera (radius 0), 'd' dim (opacity 0.003: binned by radius, no instance, never reached).  Visible and front
    ones sit on quadrant centres, dealt round-robin, each deeper than the one before it on the same quadrant."""
    P = len(kinds)
    sc = generic_scene(P, w, h, seed)
    cam = sc.camera
    rng = np.random.default_rng(seed)
    qx, qy = w // 8, h // 8
    depth_of = {"f": 1.0, "v": 2.0, "d": 2.0, "b": -2.0}
    count = {k: 0 for k in depth_of}
    for i, k in enumerate(kinds):
        j = count[k]
        count[k] += 1
        q, layer = j % (qx * qy), j // (qx * qy)
        z = np.float32(depth_of[k] + (0.02 if k == "f" else 0.1) * layer)
        px, py = 8 * (q % qx) + 3.5, 8 * (q // qx) + 3.5
        sc.means3D[i] = ((2 * px + 1) / w - 1) * abs(z) * cam.tanfovx, ((2 * py + 1) / h - 1) * abs(z) * cam.tanfovy, z
        sc.scales[i] = (0.3 + 0.15 * rng.random(3)) * abs(z) / FOCAL     # sigma <= 0.45 px: the larger eigenvalue of the 2D covariance
        #   is at most mid + sqrt(max(0.1, .)) with mid <= 0.2 * 1.25 + 0.3 (off-axis stretch included), below 1: radius <= 3
        sc.opacity[i] = {"f": 0.99, "d": 0.003}.get(k, 0.2 + 0.4 * rng.random())
    return sc


def cov3d_of(sc):
    """(P, 6) upper triangles of R diag(s^2) R^T (any symmetric positive input would do: both arms get the same)."""
    r, x, y, z = (sc.rotations[:, i].astype(np.float64) for i in range(4))
    R = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)], -1),
                  np.stack([2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)], -1),
                  np.stack([2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], -1)], 1)
    S = R @ (sc.scales.astype(np.float64)[:, :, None] ** 2 * np.transpose(R, (0, 2, 1)))
    return np.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1).astype(np.float32)


def oracle_sets(sc):
    """(never walked, touched) per Gaussian from the CPU oracle, as in the written-rows tests but for any image size: a
    Gaussian is never walked when it has no instance, or sits at or beyond the largest n_contrib of every tile that lists it."""
    from oracle import gs_oracle
    o, g = gs_oracle.run_scene(sc)
    w, h = sc.camera.width, sc.camera.height
    nc, ranges, pl = o.get("n_contrib"), o.get("ranges").astype(np.int64), o.get("point_list")
    tiles_x = (w + 15) // 16
    walked = np.zeros(sc.P, dtype=bool)
    for tile, (s, _e) in enumerate(ranges):
        ty, tx = divmod(tile, tiles_x)
        walked[pl[s:s + int(nc[ty * 16:ty * 16 + 16, tx * 16:tx * 16 + 16].max())]] = True
    touched = np.abs(g["dL_dcolor"]).sum(axis=1) != 0
    assert not (touched & ~walked).any()
    return ~walked, touched, o.get("radii")


# ---------------------------------------------------------------------------------------------------------------- engine
class Run:
    """One resident engine of `rows` rows, of which the scene's P are active.  step() = forward + backward under `flags` and
    returns clones of the seven tensors (all `rows` rows), radii, and the camera matrices of a camera_grad engine."""

    def __init__(self, sc, rows=None, **engine_kw):
        from segs_slam_amd.raster_engine import RasterEngine
        self.eng = RasterEngine(rows or sc.P, sc.camera.width, sc.camera.height, DEV, resident=True, want_cov3D_grad=True, **engine_kw)
        self.eng.set_active(sc.P)
        self.g = [_t(x) for x in (sc.bg, sc.means3D, sc.colors, sc.opacity, sc.scales, sc.rotations)]
        self.step(sc)       # the calibrating pass (synchronising path); every later one is resident
        assert self.eng.check()

    def outputs(self):
        eng = self.eng
        return [*eng.grads.values(), eng.dL_dmean2D, eng.dL_dcov3D]

    def collect(self):
        eng = self.eng
        out = {k: v.clone() for k, v in eng.grads.items()}
        out["mean2D"], out["cov3D"], out["radii"] = eng.dL_dmean2D.clone(), eng.dL_dcov3D.clone(), eng.radii.clone()
        if eng.camera_grad:
            out["view"], out["proj"] = eng.dL_dviewmatrix.clone(), eng.dL_dprojmatrix.clone()
        assert sorted(k for k in out if k not in ("view", "proj", "radii")) == sorted(TENSORS)
        return out

    def cam_args(self, sc):
        cam = sc.camera
        return _t(cam.world_view_transform), _t(cam.full_proj_transform), _t(cam.camera_center), cam.tanfovx, cam.tanfovy

    def step(self, sc, flags=0, nan=False, **backward_kw):
        self.eng.forward(*self.g, *self.cam_args(sc))
        if nan:
            for t in self.outputs():
                t.fill_(float("nan"))
        with _capi.raster_flags(flags, clear_mirror=False):
            self.eng.backward(_t(sc.dL_dout_color), **backward_kw)
        return self.collect()

    def step_cov3d(self, sc, cov, flags=0):
        """A resident step with cov3D_precomp in place of scales and rotations (the engine itself never passes one)."""
        eng = self.eng
        assert eng.can_take_projected() and eng.check()
        bg, m3, col, op, sca, rot = self.g
        view, proj, campos, tx, ty = self.cam_args(sc)
        p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
        with _capi.raster_flags(eng.flags, eng._status_mirror):
            eng._call("segs_rasterize_forward_resident", (
                *eng._scratch_r, eng.capacity, eng.P, eng.P_active, 0, 0, p(bg), eng.W, eng.H, p(m3), None, p(col), p(op), None, 1.0, None,
                p(cov), p(view), p(proj), p(campos), float(tx), float(ty), p(eng.out_color), p(eng.radii), p(eng._status)))
        eng._status_issued()
        eng._last = (bg, m3, col, None, sca, rot, view, proj, campos, tx, ty, 1.0)
        name, args = eng._backward_args(_t(sc.dL_dout_color))
        assert name == "segs_rasterize_backward_resident"
        args = list(args)
        assert args[13].value == sca.data_ptr() and args[15].value == rot.data_ptr() and args[16] is None
        args[13], args[15], args[16] = None, None, p(cov)
        with _capi.raster_flags(flags, clear_mirror=False):
            eng._call(name, tuple(args))
        return self.collect()

    def resident_and_clean(self):
        assert self.eng._last_resident and self.eng.check()
        assert_arena_clean(self.eng._geom_r, self.eng.P)


def assert_bits_equal(a, b, rows=None):
    for k in b:
        x, y = (v[k] if rows is None or k in ("view", "proj") else v[k][:rows] for v in (a, b))
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), k      # the bit patterns: -0.0 != +0.0, NaN == NaN


def assert_within_noise(got, want, null1, null2, rows=None):
    """got against want by the rule of the written-rows tests; null1 / null2 are two runs of the NO_WRITTEN_BYTES arm (the noise)."""
    for k in want:
        if k == "radii":
            assert torch.equal(got[k], want[k])
            continue
        a, b, n1, n2 = (x[k] if rows is None or k in ("view", "proj") else x[k][:rows] for x in (got, want, null1, null2))
        scale = max(float(b.abs().max()), 1e-30)
        noise = float((n1 - n2).abs().max())
        dev = float((a - b).abs().max())
        print(f"{k}: differs by {dev:.3e}, run-to-run {noise:.3e}, largest entry {scale:.3e}")
        assert dev <= 10.0 * noise + 1e-5 * scale, (k, dev, noise, scale)


# ------------------------------------------------------------------------------------------ 1. bit equality, deterministic sums
@functools.lru_cache(maxsize=None)
def quadrant_case():
    """896 Gaussians in four workgroups of the per-Gaussian backward.  Rows 0-383: a 0.99 front layer two deep over the left half of
    the quadrants, visible ones behind it and in the open, some behind the camera and some dim ones in between -- workgroups 0
    and 1 have more than 64 reached rows each (the dense path).  Rows 384-895 are behind the camera or dim but for every sixth row
    from 512 on, which is visible: workgroups 2 and 3 have some, and at most 64, reached rows (the sparse path).  So every form
    of the test below goes through both paths; asserted here from the oracle.  Also checked on the oracle: radius <= 3 and the
    centre on a quadrant centre, hence at most one (Gaussian, quadrant) pair each -- the next quadrant's nearest pixel is 4.5 px
    from the centre, where alpha <= 0.99 exp(-4.5^2 / 2) = 4e-5 < 1/255 for a 2D covariance of at most 1."""
    rng = np.random.default_rng(4)
    kinds = []
    for i in range(384):
        kinds.append("f" if i % 4 == 0 and (i // 4) % 8 < 4 else ("b" if rng.random() < 0.15 else "d" if rng.random() < 0.1 else "v"))
    for i in range(384, 896):
        kinds.append("v" if i >= 512 and i % 6 == 0 else "bd"[i % 2])
    # front-layer entries are dealt round-robin over ALL quadrants by their own counter; keep them on the left half
    sc = quadrant_scene(kinds)
    f = np.flatnonzero(np.array(kinds) == "f")
    for j, i in enumerate(f):
        q, layer = j % 32, j // 32
        z = np.float32(1.0 + 0.02 * layer)
        px, py = 8 * (q % 4) + 3.5, 8 * (q // 4) + 3.5
        old_z = sc.means3D[i, 2]
        sc.means3D[i] = ((2 * px + 1) / 64 - 1) * z * sc.camera.tanfovx, ((2 * py + 1) / 64 - 1) * z * sc.camera.tanfovy, z
        sc.scales[i] *= z / old_z
    never, touched, radii = oracle_sets(sc)
    assert radii.max() == 3 and (radii[np.array(kinds) == "b"] == 0).all() and touched.sum() >= 150 and never.sum() >= 40
    # reached rows of a workgroup: at least the touched ones, at most the visible and front ones (only they have instances)
    lo = [int(touched[b:b + 256].sum()) for b in range(0, 896, 256)]
    hi = [int(np.isin(kinds[b:b + 256], ("v", "f")).sum()) for b in range(0, 896, 256)]
    assert min(lo[0], lo[1]) > 64 and 20 <= lo[2] and hi[2] <= 64 and 10 <= lo[3] and hi[3] <= 64, (lo, hi)
    cam = sc.camera
    on = radii > 0
    pix = [((sc.means3D[on, a] / (sc.means3D[on, 2] * t) + 1) * 64 - 1) / 2 for a, t in ((0, cam.tanfovx), (1, cam.tanfovy))]
    for c in pix:
        assert np.abs((c - 3.5) / 8 - np.round((c - 3.5) / 8)).max() < 1e-4      # on a quadrant centre
    return sc, never, touched


FORMS = ("plain", "depth", "camera", "cov3D")


def form_run(sc, form):
    """-> (run, step): a resident engine of the form on the 64x64 scene `sc` and step(flags) = one forward + backward of that form."""
    rng = np.random.default_rng(17)
    kw, engine_kw = {}, {}
    if form == "depth":
        engine_kw = dict(render_depth=True)
        kw = dict(dL_ddepth=_t(rng.standard_normal((64, 64)).astype(np.float32) / 4096), dL_dalpha=_t(rng.standard_normal((64, 64)).astype(np.float32) / 4096))
    if form == "camera":
        engine_kw = dict(camera_grad=True)
    run = Run(sc, **engine_kw)
    if form == "cov3D":
        cov = _t(cov3d_of(sc))
        return run, lambda flags=0: run.step_cov3d(sc, cov, flags)
    return run, lambda flags=0: run.step(sc, flags, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_bit_equality_where_the_sums_are_deterministic(form):
    sc, never, touched = quadrant_case()
    run, step = form_run(sc, form)
    want, got, want2 = step(UNPACKED), step(), step(UNPACKED)
    if form == "cov3D":
        assert float(got["cov3D"][:512].abs().max()) > 0 and float(got["cov3D"][512:].abs().max()) > 0      # dense and sparse workgroups
    run.resident_and_clean()
    assert_bits_equal(want2, want)      # the premise: this scene's sums do not depend on the order of the atomics
    assert_bits_equal(got, want)
    assert float(got["colors"][torch.from_numpy(touched).to(DEV)].abs().sum(dim=1).min()) > 0
    if form == "camera":
        assert float(got["view"].abs().max()) > 0 and float(got["proj"].abs().max()) > 0


# ------------------------------------------------------------------------------------------ 2. general scenes
def _three_arms(run, sc, **kw):
    null1, null2 = run.step(sc, NO_WRITTEN_BYTES, **kw), run.step(sc, NO_WRITTEN_BYTES, **kw)
    want = run.step(sc, UNPACKED, **kw)
    got = run.step(sc, **kw)
    run.resident_and_clean()
    assert_within_noise(got, want, null1, null2)
    assert_within_noise(got, null1, null1, null2)
    return got


@pytest.mark.gpu
def test_layered_scene_both_poses():
    a, b, ka, kb = main_case()
    run = Run(a)
    for sc, (_binned, never, touched, _nc) in ((a, ka), (b, kb)):
        got = _three_arms(run, sc)
        idx = torch.from_numpy(np.flatnonzero(never)).to(DEV)
        for k in TENSORS:
            assert int(torch.count_nonzero(got[k][idx])) == 0, k
        assert float(got["colors"][torch.from_numpy(touched).to(DEV)].abs().sum(dim=1).min()) > 0


@pytest.mark.gpu
def test_all_touched_and_none_touched_scenes():
    sc = layered_scene(150, seed=3, n_front=0)
    sc.means3D[:, :2] *= 0.8
    sc.opacity[:] = 0.5
    got = _three_arms(Run(sc), sc)
    assert float(got["colors"].abs().sum(dim=1).min()) > 0
    sc = layered_scene(2000, seed=5, n_front=0)
    sc.opacity[:] = 0.003
    got = _three_arms(Run(sc), sc)
    for k in TENSORS:
        assert int(torch.count_nonzero(got[k])) == 0, k


# ------------------------------------------------------------------------------------------ 3. edges of the packing
@pytest.mark.gpu
@pytest.mark.parametrize("P", [1, 63, 64, 65, 255, 256, 257, 1999])
def test_row_counts_at_wave_and_workgroup_edges(P):
    sc = layered_scene(P, seed=11 + P, n_front=max(1, P // 3), cover=0.4)
    run = Run(sc)
    _three_arms(run, sc)
    _three_arms(run, second_pose(sc))
    assert int((run.eng.radii > 0).sum()) > 0


def blocks_scene():
    """Four workgroups of 256 rows: exactly 64 reached rows (the heavy wave full: the last size of the sparse path), 65 (the first
    of the dense path), none (nothing but zeros), and all 256 (no zeros at all)."""
    kinds = []
    for blk, n in enumerate((64, 65, 0, 256)):
        pick = set(np.random.default_rng(blk).permutation(256)[:n].tolist())
        kinds += ["v" if i in pick else "bd"[i % 2] for i in range(256)]
    sc = quadrant_scene(kinds, seed=8)
    sc.opacity[np.array(kinds) == "v"] = 0.1      # seven deep on every quadrant and still all of them contribute
    return sc


@pytest.mark.gpu
def test_blocks_with_64_65_0_and_256_reached_rows():
    """blocks_scene() is a quadrant scene: the arms agree bit for bit."""
    sc = blocks_scene()
    never, touched, _radii = oracle_sets(sc)
    assert [int(touched[256 * b:256 * b + 256].sum()) for b in range(4)] == [64, 65, 0, 256]
    assert not (never & touched).any()
    zero = ~touched      # behind the camera, or dim: in the oracle's lists by its radius, without an instance in the resident ones
    run = Run(sc)
    want = run.step(sc, UNPACKED, nan=True)
    got = run.step(sc, nan=True)
    run.resident_and_clean()
    assert_bits_equal(got, want)
    for k in TENSORS:
        assert int(torch.count_nonzero(got[k][torch.from_numpy(zero).to(DEV)].view(torch.int32))) == 0, k


# ------------------------------------------------------------------------------------------ 4. the zeros
def _assert_zeros(run, sc, rows, never, flags=0):
    got = run.step(sc, flags, nan=True)
    run.resident_and_clean()
    idx = torch.from_numpy(np.flatnonzero(never)).to(DEV)
    assert idx.numel() > 0
    for k in TENSORS:
        assert bool(torch.isfinite(got[k][:sc.P]).all()), k
        assert int(torch.count_nonzero(got[k][idx].view(torch.int32))) == 0, k      # +0.0: no bit set, the sign bit included
        assert rows > sc.P and bool(torch.isnan(got[k][sc.P:]).all()), k            # rows beyond the active ones: not written
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(16, 16), (40, 24), (64, 64)])
def test_zeros_of_rows_not_reached(w, h):
    sc = generic_scene(700, w, h, seed=w + h)
    never = oracle_sets(sc)[0]
    run = Run(sc, rows=1000)
    got = _assert_zeros(run, sc, 1000, never)
    assert int(torch.count_nonzero(got["colors"][:sc.P])) > 0
    want = _assert_zeros(run, sc, 1000, never, UNPACKED)
    null1, null2 = run.step(sc, NO_WRITTEN_BYTES), run.step(sc, NO_WRITTEN_BYTES)
    assert_within_noise(got, want, null1, null2, rows=sc.P)


@pytest.mark.gpu
def test_zeros_when_the_camera_sees_nothing_and_when_there_are_no_instances():
    back = np.diag([-1.0, 1.0, -1.0]).astype(np.float32)      # turned round: every Gaussian behind the camera
    sc = generic_scene(700, 64, 64, seed=2, R=back)
    run = Run(sc, rows=1000)
    got = _assert_zeros(run, sc, 1000, oracle_sets(sc)[0])
    assert int(run.eng.radii[:sc.P].abs().sum()) == 0 and run.eng.R == 0
    for k in TENSORS:
        assert int(torch.count_nonzero(got[k][:sc.P])) == 0, k
    sc = generic_scene(700, 64, 64, seed=2)
    sc.opacity[:] = 0.003      # radii > 0, alpha >= 1/255 nowhere: no instance
    run = Run(sc, rows=1000)
    got = _assert_zeros(run, sc, 1000, oracle_sets(sc)[0])
    assert int((run.eng.radii > 0).sum()) > 300 and run.eng.R == 0
    for k in TENSORS:
        assert int(torch.count_nonzero(got[k][:sc.P])) == 0, k


# ------------------------------------------------------------------------------------------ 5. the invariant
@pytest.mark.gpu
def test_arena_stays_clean_with_alternating_arms_and_after_a_redone_step():
    a, b, ka, kb = main_case()
    run = Run(a)
    null1, null2 = run.step(b, NO_WRITTEN_BYTES), run.step(b, NO_WRITTEN_BYTES)
    for sc, flags in ((a, 0), (b, UNPACKED), (a, UNPACKED), (b, 0), (a, NO_WRITTEN_BYTES), (b, 0)):
        got = run.step(sc, flags)
        run.resident_and_clean()
    want = run.step(b, UNPACKED)
    assert_within_noise(got, want, null1, null2)
    stale = torch.from_numpy(np.flatnonzero(ka[2] & kb[1])).to(DEV)      # touched from pose a, never walked from pose b
    assert stale.numel() > 0
    for k in TENSORS:
        assert int(torch.count_nonzero(got[k][stale])) == 0, k
    eng = run.eng
    arena = eng._geom_r
    eng.capacity = max(eng.R // 3, 1024)      # fewer instance slots than the scene needs
    assert eng.R > eng.capacity
    run.step(a)                               # dropped on the device: its tile kernels walk truncated lists
    assert eng._last_resident and eng.check(raise_on_overflow=False) is False
    assert_arena_clean(arena, eng.P)
    run.step(a)                               # redone through the synchronising path
    assert not eng._last_resident and eng.capacity > eng.R
    got = run.step(b)
    run.resident_and_clean()
    assert_within_noise(got, want, null1, null2)


# ------------------------------------------------------------------------------------------ 6. captured step
@pytest.mark.gpu
def test_captured_step_replayed():
    a, _b, (_binned, never, _touched, _nc), _kb = main_case()
    run = Run(a)
    null1, null2 = run.step(a, NO_WRITTEN_BYTES), run.step(a, NO_WRITTEN_BYTES)
    eager = run.step(a)
    run.resident_and_clean()
    eng = run.eng
    dL, args = _t(a.dL_dout_color), (*run.g, *run.cam_args(a))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        eng.forward(*args)
        eng.backward(dL)
    for _ in range(3):
        for t in run.outputs():
            t.fill_(float("nan"))
        graph.replay()
        eng.after_graph_replay()
        torch.cuda.synchronize()
        got = run.collect()
        run.resident_and_clean()
        assert_within_noise(got, eager, null1, null2)
        idx = torch.from_numpy(np.flatnonzero(never)).to(DEV)
        for k in TENSORS:
            assert int(torch.count_nonzero(got[k][idx].view(torch.int32))) == 0, k


# ------------------------------------------------------------------------------------------- two builds of the library
FLAG_ARMS = {"0": 0, "UNPACKED": UNPACKED, "NO_WRITTEN_BYTES": NO_WRITTEN_BYTES}


def dump(path):
    """The raw bits of every gradient tensor the loaded library gives on the scenes without atomic-order noise (see the module
    docstring), and of the stage-alone debug entries, which take the body's path without accumulator rows."""
    from oracle import gs_oracle
    from tests.test_camera_grad_gpu import stage
    out = {}

    def keep(prefix, tensors):
        for k, v in tensors.items():
            a = v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
            out[f"{prefix}/{k}"] = np.ascontiguousarray(a).view(np.int32) if a.dtype == np.float32 else a

    quadrant, blocks = quadrant_case()[0], blocks_scene()
    for form in FORMS:
        run, step = form_run(quadrant, form)
        for arm, flags in FLAG_ARMS.items():
            keep(f"quadrant/{form}/{arm}", step(flags))
        run.resident_and_clean()
    run = Run(blocks)
    for arm in ("0", "UNPACKED"):
        keep(f"blocks/{arm}", run.step(blocks, FLAG_ARMS[arm], nan=True))
    run.resident_and_clean()
    for name, sc in (("quadrant", quadrant), ("blocks", blocks)):
        o, g = gs_oracle.run_scene(sc)
        radii, g2, gc = o.get("radii"), g["dL_dmean2D"], g["dL_dconic"]
        dz = np.random.default_rng(29).standard_normal(sc.P).astype(np.float32) / 64
        for pre, cov in (("scales", None), ("cov3D_precomp", cov3d_of(sc))):
            names = ("mean3D", "cov3D") if cov is not None else ("mean3D", "cov3D", "scale", "rot")
            grads, _ = stage(sc, radii, g2, gc, cov3D=cov, camera=False)
            keep(f"stage/{name}/{pre}/plain", dict(zip(names, grads)))
            grads, mats = stage(sc, radii, g2, gc, dz=dz, cov3D=cov)
            keep(f"stage/{name}/{pre}/camera_dz", dict(zip(names, grads), view_proj=mats))
    np.savez(path, **out)
    print("wrote", len(out), "arrays to", path)


def compare(path_a, path_b):
    a, b = np.load(path_a), np.load(path_b)
    assert sorted(a.files) == sorted(b.files), sorted(set(a.files) ^ set(b.files))
    bad = 0
    for k in sorted(a.files):
        x, y = a[k], b[k]
        assert x.dtype == np.int32 and y.dtype == np.int32 and x.shape == y.shape, (k, x.dtype, y.dtype, x.shape, y.shape)
        if not np.array_equal(x, y):
            row = int(np.flatnonzero((x != y).reshape(x.shape[0], -1).any(axis=1))[0]) if x.ndim else 0
            print(f"DIFFERENT: {k}, first at row {row}: {x[row].view(np.float32).tolist()} against {y[row].view(np.float32).tolist()}")
            bad += 1
    print(len(a.files), "arrays compared as int32;", "all bit-identical" if not bad else f"{bad} DIFFERENT")
    return 1 if bad else 0


if __name__ == "__main__":
    import sys
    sys.exit(dump(sys.argv[2]) if sys.argv[1] == "dump" else compare(sys.argv[2], sys.argv[3]))
