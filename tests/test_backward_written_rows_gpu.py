"""The "row written" bytes of the resident backward (csrc/gs_layout.h): the tile backward sets one byte next
to every accumulator row it adds into, and the per-Gaussian backward reads, converts and clears only those rows.

Every scene is 64x64 with at most about 2 000 Gaussians.  The main one has an opaque front layer (300 large Gaussians of opacity
0.99 at depth 1.0-1.05) over the left 57 % of the image in front of the rest at depth 2-5, so that many binned Gaussians are never
reached by the tile backward while those behind the open part are.  The CPU oracle says which: a Gaussian is NEVER WALKED when in
every tile that lists it its position is at or beyond the tile's largest n_contrib (the resident lists are the oracle's with dead
instances left out, in the same order, so such a Gaussian is beyond every wave's last contributor there too), and TOUCHED when the
oracle's own backward gives it a non-zero dL/dcolor.

Comparisons between two runs of the engine use the rule of tools/fuzz_projecting_forward.py: the tile backward sums with float
atomics, so two backwards of the same inputs differ by that noise; the bar is ten times the largest difference between two runs of
the path WITHOUT the bytes (SEGS_RASTER_NO_WRITTEN_BYTES), plus 1e-5 of the tensor's largest entry."""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest
import torch

from segs_slam_amd import _capi, scenes

DEV = "cuda:0"
W = H = 64
FOCAL = 60.0
NO_WRITTEN_BYTES = 128      # SEGS_RASTER_NO_WRITTEN_BYTES (include/segs_raster.h; tests/test_written_rows_layout_cpu.py pins the value)
TENSORS = ("means3D", "scales", "rotations", "opacity", "colors", "mean2D", "cov3D")      # the seven gradient tensors


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def layered_scene(P, seed=7, n_front=300, cover=0.15):
    """P Gaussians in front of an unrotated camera at the origin: the first min(n_front, P) form the opaque layer, which reaches
    from the left edge to `cover` (in units of the half width) right of the centre; the others are small and lie at depth 2-5."""
    sc = scenes.make_scene(P, W, H, FOCAL, FOCAL, seed=seed, bg=(0.1, 0.2, 0.3), name="layered")
    cam = scenes.make_camera(W, H, FOCAL, FOCAL, np.eye(3, dtype=np.float32), np.zeros(3, dtype=np.float32))
    sc = dataclasses.replace(sc, camera=cam)
    rng = np.random.default_rng(seed)
    tx, ty = np.float32(cam.tanfovx), np.float32(cam.tanfovy)
    z = (2.0 + 3.0 * rng.random(P)).astype(np.float32)
    sc.means3D[:, 2] = z
    sc.means3D[:, 0] = (rng.random(P) * 2 - 1).astype(np.float32) * 1.1 * z * tx
    sc.means3D[:, 1] = (rng.random(P) * 2 - 1).astype(np.float32) * 1.1 * z * ty
    sc.scales[:] = (0.02 + 0.05 * rng.random((P, 3))).astype(np.float32)
    nf = min(n_front, P)
    if nf:
        zf = (1.0 + 0.05 * rng.random(nf)).astype(np.float32)
        sc.means3D[:nf, 2] = zf
        sc.means3D[:nf, 0] = (-1.1 + (1.1 + cover) * rng.random(nf)).astype(np.float32) * zf * tx
        sc.means3D[:nf, 1] = (rng.random(nf) * 2 - 1).astype(np.float32) * 1.1 * zf * ty
        sc.scales[:nf] = 0.12
        sc.opacity[:nf] = 0.99
    return sc


def second_pose(sc):
    """The same Gaussians from a camera moved sideways (t = (0.25, 0.05, 0)) and turned by -8 degrees about y, so that the layer
    hides another part of them, and another dL/dimage."""
    a = np.radians(-8.0)
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], dtype=np.float32)
    cam = scenes.make_camera(W, H, FOCAL, FOCAL, R, np.array([0.25, 0.05, 0.0], dtype=np.float32))
    dL = np.random.default_rng(99).standard_normal((3, H, W)).astype(np.float32) / np.float32(3 * H * W)
    return dataclasses.replace(sc, camera=cam, dL_dout_color=dL)


def oracle_kinds(sc):
    """(binned, never walked, touched) per Gaussian from the CPU oracle, and its n_contrib."""
    from oracle import gs_oracle
    o, g = gs_oracle.run_scene(sc)
    binned = o.get("radii") > 0
    nc, ranges, pl = o.get("n_contrib"), o.get("ranges").astype(np.int64), o.get("point_list")
    tiles_x = (W + 15) // 16
    walked = np.zeros(sc.P, dtype=bool)
    for tile, (s, _e) in enumerate(ranges):
        ty, tx = divmod(tile, tiles_x)
        walked[pl[s:s + int(nc[ty * 16:ty * 16 + 16, tx * 16:tx * 16 + 16].max())]] = True
    touched = np.abs(g["dL_dcolor"]).sum(axis=1) != 0
    assert not (touched & ~walked).any()
    return binned, binned & ~walked, touched, nc


@functools.lru_cache(maxsize=None)
def main_case():
    """The main scene at both poses with the oracle's sets, computed once and shared (nothing below changes them)."""
    a = layered_scene(2000)
    b = second_pose(a)
    ka, kb = oracle_kinds(a), oracle_kinds(b)
    for binned, never, touched, _ in (ka, kb):
        assert never.sum() >= 0.2 * binned.sum() and touched.sum() >= 0.2 * binned.sum(), (binned.sum(), never.sum(), touched.sum())
    return a, b, ka, kb


def test_main_scene_has_untouched_and_touched_gaussians():
    a, b, ka, kb = main_case()
    assert int((ka[2] & kb[1]).sum()) > 0      # touched from the first pose, never walked from the second: what could go stale


class Run:
    """One engine on one set of Gaussians; step() is a resident forward + backward and returns clones of the seven tensors."""

    def __init__(self, sc, **engine_kw):
        from segs_slam_amd.raster_engine import RasterEngine
        self.sc = sc
        self.eng = RasterEngine(sc.P, W, H, DEV, resident=True, want_cov3D_grad=True, **engine_kw)
        self.g = [_t(x) for x in (sc.bg, sc.means3D, sc.colors, sc.opacity, sc.scales, sc.rotations)]
        self.step(sc)       # the calibrating pass (synchronising path); every later one is resident
        assert self.eng.check()

    def step(self, sc, null=False, **backward_kw):
        cam = sc.camera
        eng = self.eng
        eng.forward(*self.g, _t(cam.world_view_transform), _t(cam.full_proj_transform), _t(cam.camera_center), cam.tanfovx, cam.tanfovy)
        with _capi.raster_flags(NO_WRITTEN_BYTES if null else 0, clear_mirror=False):
            eng.backward(_t(sc.dL_dout_color), **backward_kw)
        out = {k: v.clone() for k, v in eng.grads.items()}
        out["mean2D"], out["cov3D"] = eng.dL_dmean2D.clone(), eng.dL_dcov3D.clone()
        if eng.camera_grad:
            out["view"], out["proj"] = eng.dL_dviewmatrix.clone(), eng.dL_dprojmatrix.clone()
        assert sorted(k for k in out if k not in ("view", "proj")) == sorted(TENSORS)
        return out

    def resident_and_clean(self):
        """The last step took the resident path, was valid, and left every accumulator row and every byte of the arena zero."""
        assert self.eng._last_resident and self.eng.check()
        assert_arena_clean(self.eng._geom_r, self.eng.P)


def assert_arena_clean(geom, rows):
    lay = (C.c_size_t * 20)()
    _capi.check(_capi.lib().segs_debug_geometry_layout(rows, C.cast(lay, C.c_void_p), 10), "segs_debug_geometry_layout")
    base = (-geom.data_ptr()) % 256
    for region in (7, 9):      # accumulator rows, "row written" bytes
        off, n = int(lay[2 * region]), int(lay[2 * region + 1])
        assert n > 0 and int(torch.count_nonzero(geom[base + off:base + off + n])) == 0, region


def assert_same(got, want, want_again, rows=None):
    """got against want by the noise rule; want_again is a second run of want's path (the noise)."""
    for k in want:
        a, b, b2 = (x[k] if rows is None or k in ("view", "proj") else x[k][:rows] for x in (got, want, want_again))
        scale = max(float(b.abs().max()), 1e-30)
        noise = float((b - b2).abs().max())
        dev = float((a - b).abs().max())
        print(f"{k}: differs by {dev:.3e}, run-to-run {noise:.3e}, largest entry {scale:.3e}")
        assert dev <= 10.0 * noise + 1e-5 * scale, (k, dev, noise, scale)


def assert_rows_zero(out, rows):
    idx = torch.from_numpy(np.flatnonzero(rows)).to(DEV)
    assert idx.numel() > 0
    for k in TENSORS:
        assert int(torch.count_nonzero(out[k][idx])) == 0, k


@pytest.mark.gpu
def test_written_rows_against_the_path_without_the_bytes():
    a, _, (binned, never, touched, _nc), _ = main_case()
    run = Run(a)
    assert np.array_equal(run.eng.radii.cpu().numpy() > 0, binned)
    null1 = run.step(a, null=True)
    run.resident_and_clean()
    null2 = run.step(a, null=True)
    got = run.step(a)
    run.resident_and_clean()
    assert_same(got, null1, null2)
    assert_rows_zero(got, never)
    assert float(got["colors"][torch.from_numpy(touched).to(DEV)].abs().sum(dim=1).min()) > 0   # and the touched rows did arrive


@pytest.mark.gpu
def test_nothing_stale_from_the_step_before():
    a, b, ka, kb = main_case()
    run = Run(a)
    run.step(a)
    run.resident_and_clean()
    got = run.step(b)
    run.resident_and_clean()
    fresh = Run(b)
    want, want_again = fresh.step(b, null=True), fresh.step(b, null=True)
    assert_same(got, want, want_again)
    assert_rows_zero(got, ka[2] & kb[1])      # touched in the first step, never walked in the second


@pytest.mark.gpu
@pytest.mark.parametrize("P", [1, 63, 65, 255, 257])
def test_wave_and_workgroup_tails(P):
    sc = layered_scene(P, seed=11 + P, n_front=max(1, P // 3), cover=0.4)
    run = Run(sc)
    null1, null2 = run.step(sc, null=True), run.step(sc, null=True)
    got = run.step(sc)
    run.resident_and_clean()
    assert_same(got, null1, null2)
    got = run.step(second_pose(sc))      # and once more on the arena that step left
    run.resident_and_clean()
    assert int((run.eng.radii > 0).sum()) > 0


@pytest.mark.gpu
def test_scene_in_which_no_gaussian_is_touched():
    """Binned Gaussians none of which the tile backward reaches, with a non-zero dL/dimage: every opacity is below 1/255, so no
    pixel passes the alpha test, n_contrib is zero everywhere and no wave walks anything.  (An opaque layer does not give this
    case from either side: the layer's own Gaussians are touched.  dL/dimage = 0 does not either: rows are then written, with zeros.)"""
    sc = layered_scene(2000, seed=5, n_front=0)
    sc.opacity[:] = 0.003
    binned, never, touched, nc = oracle_kinds(sc)
    assert binned.sum() > 1000 and not touched.any() and not nc.any() and np.array_equal(never, binned)
    run = Run(sc)
    null1, null2 = run.step(sc, null=True), run.step(sc, null=True)
    got = run.step(sc)
    run.resident_and_clean()
    assert_same(got, null1, null2)
    assert int((run.eng.radii > 0).sum()) == int(binned.sum())
    for k in TENSORS:
        assert int(torch.count_nonzero(got[k])) == 0, k


@pytest.mark.gpu
def test_scene_in_which_every_gaussian_is_touched():
    sc = layered_scene(150, seed=3, n_front=0)
    sc.means3D[:, :2] *= 0.8      # every centre inside the image: the pixel next to it passes the alpha test
    sc.opacity[:] = 0.5
    binned, never, touched, _ = oracle_kinds(sc)
    assert binned.all() and touched.all() and not never.any()
    run = Run(sc)
    null1, null2 = run.step(sc, null=True), run.step(sc, null=True)
    got = run.step(sc)
    run.resident_and_clean()
    assert_same(got, null1, null2)
    assert float(got["colors"].abs().sum(dim=1).min()) > 0


@pytest.mark.gpu
def test_depth_form():
    a, _, (_b, never, _t2, _nc), _ = main_case()
    rng = np.random.default_rng(17)
    dz, da = (_t(rng.standard_normal((H, W)).astype(np.float32) / np.float32(H * W)) for _ in range(2))
    run = Run(a, render_depth=True)
    kw = dict(dL_ddepth=dz, dL_dalpha=da)
    null1, null2 = run.step(a, null=True, **kw), run.step(a, null=True, **kw)
    got = run.step(a, **kw)
    run.resident_and_clean()
    assert_same(got, null1, null2)
    assert_rows_zero(got, never)
    plain = run.step(a)       # the plain form on the arena the depth form left, against the depth form with zero map gradients
    zero = run.step(a, dL_ddepth=torch.zeros_like(dz), dL_dalpha=torch.zeros_like(da))
    run.resident_and_clean()
    assert_same(plain, zero, run.step(a, dL_ddepth=torch.zeros_like(dz), dL_dalpha=torch.zeros_like(da)))


@pytest.mark.gpu
def test_camera_gradient_form():
    a, _, (_b, never, _t2, _nc), _ = main_case()
    run = Run(a, camera_grad=True)
    null1, null2 = run.step(a, null=True), run.step(a, null=True)
    got = run.step(a)
    run.resident_and_clean()
    assert float(got["view"].abs().max()) > 0 and float(got["proj"].abs().max()) > 0
    assert_same(got, null1, null2)      # the seven tensors and both camera sums
    assert_rows_zero(got, never)


@pytest.mark.gpu
def test_step_that_overflows_the_capacity_and_is_redone():
    a, _, (_b, never, _t2, _nc), _ = main_case()
    run = Run(a)
    want, want_again = run.step(a, null=True), run.step(a, null=True)
    eng = run.eng
    arena = eng._geom_r
    eng.capacity = max(eng.R // 3, 1024)   # fewer instance slots than the scene needs (the buffers stay as large as they were)
    assert eng.R > eng.capacity
    run.step(a)                          # dropped on the device: its tile kernels walk truncated lists
    assert eng._last_resident and eng.check(raise_on_overflow=False) is False
    assert_arena_clean(arena, eng.P)     # ... and still every row they added into went back to zero, with its byte
    run.step(a)                          # redone: the synchronising path, which sizes the resident scratch anew
    assert not eng._last_resident and eng.capacity > eng.R
    got = run.step(a)
    run.resident_and_clean()
    assert_same(got, want, want_again)
    assert_rows_zero(got, never)
