"""GPU tests of the camera gradient (segs_*_camera; run with -m gpu on an MI355X).

dL/dviewmatrix and dL/dprojmatrix are cancelling sums over the binned Gaussians, so the bar is relative to S_k = sum_i |c_ik|, the
absolute sum of the per-Gaussian contributions of entry k (float64 closed form of tests/test_camera_grad_cpu.py, fed the CPU
oracle's dL_dmean2D / dL_dconic):  |have_k - want_k| <= 1e-4 S_k, the project's per-Gaussian relative gradient bar carried
through the sum.  `want` is that closed form for the per-Gaussian stage alone and float64 autograd of oracle.torch_ref.render
with the two matrices as leaves for the whole backward (the closed form sits within 1e-6 S_k of it; test_camera_grad_cpu.py).
Every test prints its worst err / S before it asserts.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import gs_oracle
from segs_slam_amd import scenes
from tests import test_camera_grad_cpu as ref
from tests.test_depth_render_gpu import GRAD_NAMES, _small_scene, depth_backward, depth_forward
from tests.test_raster_gpu import DEV, _t, assert_grad_close, gpu_forward

pytestmark = pytest.mark.gpu

BAR = 1e-4
ZEROS = ref.STRUCTURAL_ZEROS


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class _CameraOut:
    """The two (4, 4) outputs, NaN-filled so that every float must be written, the scratch, and the struct over them."""

    def __init__(self, rows):
        from segs_slam_amd import _capi
        self.view = torch.full((4, 4), float("nan"), device=DEV)
        self.proj = torch.full((4, 4), float("nan"), device=DEV)
        self.temp = torch.empty(_capi.lib().segs_camera_grad_temp_bytes(rows), dtype=torch.uint8, device=DEV)
        self.struct = _capi.CameraGrads(self.view.data_ptr(), self.proj.data_ptr(), self.temp.data_ptr())

    def flat(self):
        torch.cuda.synchronize()
        return torch.cat([self.view.reshape(-1), self.proj.reshape(-1)]).cpu().numpy()


def stage(sc, radii, g2, gc, dz=None, cov3D=None, camera=True):
    """segs_debug_preprocess_backward[_camera] -> ([dL_dmean3D, dL_dcov3D, dL_dscale, dL_drot] as numpy, 32 floats or None)."""
    from segs_slam_amd import _capi
    cam, P = sc.camera, sc.P
    m3, sca, rot = _t(sc.means3D), _t(sc.scales), _t(sc.rotations)
    view, proj = _t(cam.world_view_transform), _t(cam.full_proj_transform)
    rad = _t(radii, torch.int32)
    d2, dc = _t(np.asarray(g2, dtype=np.float32)), _t(np.asarray(gc, dtype=np.float32))
    outs = [torch.full((P, n), float("nan"), device=DEV) for n in (3, 6, 3, 4)]
    pre = _t(cov3D) if cov3D is not None else None
    dzt = _t(dz) if dz is not None else None
    head = (P, cam.width, cam.height, _p(m3), _p(rad), None if pre is not None else _p(sca), 1.0, None if pre is not None else _p(rot),
            _p(pre), _p(view), _p(proj), cam.tanfovx, cam.tanfovy, _p(d2), _p(dc), _p(outs[0]), _p(outs[1]),
            None if pre is not None else _p(outs[2]), None if pre is not None else _p(outs[3]))
    if camera:
        out = _CameraOut(P)
        st = _capi.lib().segs_debug_preprocess_backward_camera(*head, _p(dzt), C.byref(out.struct), _stream())
        _capi.check(st, "segs_debug_preprocess_backward_camera")
        mats = out.flat()
    else:
        _capi.check(_capi.lib().segs_debug_preprocess_backward(*head, _stream()), "segs_debug_preprocess_backward")
        torch.cuda.synchronize()
        mats = None
    return [t.cpu().numpy() for t in (outs[:2] if pre is not None else outs)], mats


def _stage_case(name):
    """-> (scene, radii, g2 (P,3) float32, gc (P,2,2) float32) with the CPU oracle's per-Gaussian inputs of the stage."""
    if name in ("G", "C"):
        sc, o, _, _ = ref.case(name)
        g2, gc, _ = ref.oracle_inputs(name, False)
        return sc, o.get("radii"), g2.astype(np.float32), gc.astype(np.float32), o
    P, W, H = {"1000@64x64": (1000, 64, 64), "257@64x64": (257, 64, 64), "17@33x17": (17, 33, 17), "1@16x16": (1, 16, 16)}[name]
    sc = _small_scene(P, W, H, (0.1, 0.2, 0.3))
    o, g = gs_oracle.run_scene(sc)
    return sc, o.get("radii"), g["dL_dmean2D"], g["dL_dconic"], o


@pytest.mark.parametrize("name", ["G", "C", "1000@64x64", "257@64x64", "17@33x17", "1@16x16"])
def test_stage_alone_matches_the_closed_form_and_is_bit_reproducible(name):
    """The per-Gaussian stage alone: 12 workgroups (G), clamped coordinates (C), a partly filled last workgroup (1000), one live
    lane in the second workgroup (257), less than a wave (17) and a single Gaussian."""
    sc, radii, g2, gc, o = _stage_case(name)
    cam = sc.camera
    if name == "C":
        assert ref.clamped_mask(sc, radii).sum() >= 1
    plain, _ = stage(sc, radii, g2, gc, camera=False)
    dzv = (scenes.uniform01(sc.P, 77, 5) * 2 - 1).astype(np.float32)
    for dz in (None, dzv):
        outs, mats = stage(sc, radii, g2, gc, dz=dz)
        outs2, mats2 = stage(sc, radii, g2, gc, dz=dz)
        assert np.array_equal(mats.view(np.uint32), mats2.view(np.uint32)), "two calls must give the same bits"
        c = ref.contributions_f64(sc.means3D, sc.scales, sc.rotations, cam.world_view_transform, cam.full_proj_transform, cam.width,
                                  cam.height, cam.tanfovx, cam.tanfovy, g2, gc, radii, sc.scale_modifier, dz=dz)
        S = np.abs(c).sum(0)
        ratio = ref.worst_ratio(mats, c.sum(0), S)
        print(f"stage {name} dz={dz is not None}: binned {int((radii > 0).sum())}, worst err/S = {ratio:.3e}")
        assert ratio <= BAR, (name, ratio)
        assert np.all(mats[ZEROS] == 0)
        # the per-Gaussian outputs are the plain stage's bits (dL/dmean3D carries the dz term when dz is given)
        for k, (a, b) in enumerate(zip(outs, plain)):
            if dz is None or k != 0:
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (name, k)
        if dz is not None:
            V = cam.world_view_transform.reshape(4, 4).astype(np.float64)
            want = plain[0].astype(np.float64) + np.where(radii[:, None] > 0, dzv[:, None].astype(np.float64) * V[:3, 2][None, :], 0.0)
            assert np.all(np.abs(outs[0] - want) <= 1e-5 * np.abs(want) + 1e-6 * max(np.abs(want).max(), 1e-30))


def test_stage_alone_with_precomputed_covariances():
    sc, radii, g2, gc, o = _stage_case("C")
    cam = sc.camera
    cov6 = o.get("cov3D")
    outs, mats = stage(sc, radii, g2, gc, cov3D=cov6)
    plain, _ = stage(sc, radii, g2, gc, cov3D=cov6, camera=False)
    c = ref.contributions_f64(sc.means3D, None, None, cam.world_view_transform, cam.full_proj_transform, cam.width, cam.height,
                              cam.tanfovx, cam.tanfovy, g2, gc, radii, cov3D=cov6)
    S = np.abs(c).sum(0)
    ratio = ref.worst_ratio(mats, c.sum(0), S)
    print(f"stage C with cov3D_precomp: worst err/S = {ratio:.3e}")
    assert ratio <= BAR and np.all(mats[ZEROS] == 0) and S[0] > 0
    for a, b in zip(outs, plain):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def camera_backward(sc, args, fwd, dL, dD, dA):
    """RasterizeGaussiansCameraBackwardCUDA on the state of depth_forward -> (dict of numpy gradients, 32 floats)."""
    from segs_slam_amd import rasterize_points as rp
    cam = sc.camera
    e = torch.empty(0, device=DEV)
    R, color, radii, depth, alpha, geom, binning, img = fwd
    out = rp.RasterizeGaussiansCameraBackwardCUDA(args["bg"], args["means3D"], radii, args["colors"], args["scales"], args["rotations"],
                                                  sc.scale_modifier, e, args["view"], args["proj"], cam.tanfovx, cam.tanfovy, dL, dD, dA,
                                                  e, 0, args["campos"], geom, R, binning, img)
    torch.cuda.synchronize()
    assert out[8].shape == (4, 4) and out[9].shape == (4, 4)
    mats = torch.cat([out[8].reshape(-1), out[9].reshape(-1)]).cpu().numpy()
    return {k: v.cpu().numpy() for k, v in zip(GRAD_NAMES, out[:8])}, mats


@pytest.mark.parametrize("name,maps", [("G", False), ("G", True), ("C", False)])
def test_full_backward_matches_float64_autograd(name, maps):
    sc, o, unstable, (dL, dD, dA) = ref.case(name)
    g2, gc, dz = ref.oracle_inputs(name, maps)
    c = ref.scene_contributions(sc, o, g2, gc, dz=dz)
    S = np.abs(c).sum(0)
    truth = ref.autograd_truth(name, maps or name == "G")
    want = truth["colour"] + (truth["maps"] if maps else 0.0)
    # the test can see both terms a chain through dL/dmean3D would miss: without either the closed form leaves the bar
    assert ref.worst_ratio(ref.scene_contributions(sc, o, g2, gc, dz=dz, with_jt=False).sum(0), want, S) > BAR
    if maps:
        assert ref.worst_ratio(ref.scene_contributions(sc, o, g2, gc).sum(0), want, S) > BAR
    if name == "C":
        assert ref.clamped_mask(sc, o.get("radii")).sum() >= 1
    args, _ = gpu_forward(sc)
    fwd = depth_forward(sc, args)
    assert np.array_equal(fwd[2].cpu().numpy(), o.get("radii"))
    tD, tA = (_t(dD), _t(dA)) if maps else (None, None)
    got, mats = camera_backward(sc, args, fwd, _t(dL), tD, tA)
    ratio = ref.worst_ratio(mats, want, S)
    print(f"full backward {name} maps={maps}: unstable share {unstable.mean():.4f}, worst err/S = {ratio:.3e}")
    assert ratio <= BAR, (name, maps, ratio)
    assert np.all(mats[ZEROS] == 0)
    base = depth_backward(sc, args, fwd, _t(dL), tD, tA)
    for k in GRAD_NAMES:
        if base[k].size:
            assert_grad_close(k, got[k], base[k])


def _raw_backward(entry, sc, args, fwd, dL, extra, shs=None):
    """One of the segs_rasterize_backward* entry points with `extra` in front of `stream` -> (status, dict of tensors)."""
    from segs_slam_amd import _capi
    cam, P = sc.camera, sc.P
    R, color, radii, depth, alpha, geom, binning, img = fwd
    o = {k: torch.full((P, n), float("nan"), device=DEV) for k, n in (("dL_dmean2D", 3), ("dL_dopacity", 1), ("dL_dcolor", 3),
                                                                       ("dL_dmean3D", 3), ("dL_dcov3D", 6), ("dL_dscale", 3), ("dL_drot", 4))}
    dsh = torch.zeros((P, 1, 3), device=DEV) if shs is not None else None
    st = getattr(_capi.lib(), entry)(P, 0, 1 if shs is not None else 0, int(R), _p(args["bg"]), cam.width, cam.height, _p(args["means3D"]),
                                     _p(shs), _p(args["colors"]), _p(args["scales"]), 1.0, _p(args["rotations"]), None, _p(args["view"]),
                                     _p(args["proj"]), _p(args["campos"]), cam.tanfovx, cam.tanfovy, _p(radii), _p(geom), _p(binning),
                                     _p(img), _p(dL), _p(o["dL_dmean2D"]), None, _p(o["dL_dopacity"]), _p(o["dL_dcolor"]),
                                     _p(o["dL_dmean3D"]), _p(o["dL_dcov3D"]), _p(dsh), _p(o["dL_dscale"]), _p(o["dL_drot"]), *extra, _stream())
    torch.cuda.synchronize()
    return st, o


def test_edge_cases_empty_culled_null_struct_and_sh():
    from segs_slam_amd import _capi
    lib = _capi.lib()
    sc = _small_scene(1000, 64, 64, (0.1, 0.2, 0.3))
    cam = sc.camera
    args, _ = gpu_forward(sc)
    fwd = depth_forward(sc, args)
    dL = _t(sc.dL_dout_color)
    # P == 0: both matrices are zero-filled before the early return
    out = _CameraOut(0)
    st = lib.segs_rasterize_backward_camera(0, 0, 0, 0, _p(args["bg"]), cam.width, cam.height, *([None] * 3), None, 1.0, *([None] * 5),
                                            cam.tanfovx, cam.tanfovy, *([None] * 14), None, C.byref(out.struct), _stream())
    assert st == 0 and not out.flat().any()
    out = _CameraOut(0)
    st = lib.segs_debug_preprocess_backward_camera(0, cam.width, cam.height, *([None] * 3), 1.0, *([None] * 4), cam.tanfovx, cam.tanfovy,
                                                   *([None] * 7), C.byref(out.struct), _stream())
    assert st == 0 and not out.flat().any()
    # an all-culled scene (every Gaussian behind the camera): R == 0, zero matrices from the whole backward and from the stage alone
    behind = _small_scene(1000, 64, 64, (0.1, 0.2, 0.3))
    behind.means3D[:, 2] = -np.abs(behind.means3D[:, 2]) - 1.0
    b_args, _ = gpu_forward(behind)
    b_fwd = depth_forward(behind, b_args)
    assert b_fwd[0] == 0 and not bool(b_fwd[2].any())
    _, mats = camera_backward(behind, b_args, b_fwd, dL, None, None)
    assert not mats.any()
    _, mats = stage(behind, np.zeros(behind.P, np.int32), np.ones((behind.P, 3), np.float32), np.ones((behind.P, 2, 2), np.float32))
    assert not mats.any()
    # a NULL struct makes the call the depth entry point
    zero_maps = C.byref(_capi.DepthGrads(None, None))
    st0, want = _raw_backward("segs_rasterize_backward_depth", sc, args, fwd, dL, (zero_maps,))
    st1, got = _raw_backward("segs_rasterize_backward_camera", sc, args, fwd, dL, (zero_maps, None))
    assert st0 == 0 and st1 == 0
    for k in want:
        assert_grad_close(k, got[k].cpu().numpy(), want[k].cpu().numpy())
    # the SH colour branch depends on campos: refused, nothing written
    out = _CameraOut(sc.P)
    shs = torch.zeros((sc.P, 1, 3), device=DEV)
    st, _ = _raw_backward("segs_rasterize_backward_camera", sc, args, fwd, dL, (None, C.byref(out.struct)), shs=shs)
    assert st == -1 and b"campos" in lib.segs_last_error()          # SEGS_ERR_INVALID_ARGUMENT
    assert np.isnan(out.flat()).all()
    # and the same call without shs fills the matrices, the eight structural zeros exactly
    st, _ = _raw_backward("segs_rasterize_backward_camera", sc, args, fwd, dL, (None, C.byref(out.struct)))
    mats = out.flat()
    assert st == 0 and np.isfinite(mats).all() and np.all(mats[ZEROS] == 0) and np.abs(mats).max() > 0


def test_resident_engine_graph_capture_and_clean_rows():
    from segs_slam_amd.raster_engine import RasterEngine
    sc, o, unstable, (dL_np, _, _) = ref.case("G")
    cam = sc.camera
    g2, gc, _ = ref.oracle_inputs("G", False)
    S = np.abs(ref.scene_contributions(sc, o, g2, gc)).sum(0)
    rows = 4096                                   # geom_rows > P: the buffers are sized for more rows than are rasterized
    pad = lambda a: torch.cat([_t(a), torch.zeros((rows - sc.P,) + a.shape[1:], device=DEV)])  # noqa: E731
    a = [_t(sc.bg), pad(sc.means3D), pad(sc.colors), pad(sc.opacity), pad(sc.scales), pad(sc.rotations), _t(cam.world_view_transform),
         _t(cam.full_proj_transform), _t(cam.camera_center)]
    dL = _t(dL_np)
    mats = lambda e: torch.cat([e.dL_dviewmatrix.reshape(-1), e.dL_dprojmatrix.reshape(-1)]).cpu().numpy().copy()  # noqa: E731
    res = {}
    for resident in (False, True):
        eng = RasterEngine(rows, cam.width, cam.height, DEV, resident=resident, camera_grad=True)
        eng.set_active(sc.P)
        for _ in range(3):
            eng.forward(*a, cam.tanfovx, cam.tanfovy)
            eng.backward(dL)
        assert eng.check()
        torch.cuda.synchronize()
        assert eng._last_resident == resident
        res[resident] = (mats(eng), eng)
    (m_sync, _), (m_res, eng) = res[False], res[True]
    ratio = ref.worst_ratio(m_res, m_sync, S)
    print(f"resident vs synchronising: worst err/S = {ratio:.3e}")
    assert ratio <= BAR and np.abs(m_sync).max() > 0 and np.all(m_res[ZEROS] == 0)
    truth = ref.autograd_truth("G", True)["colour"]
    print(f"resident vs float64 autograd: worst err/S = {ref.worst_ratio(m_res, truth, S):.3e}")
    assert ref.worst_ratio(m_res, truth, S) <= BAR
    # with a render_depth engine and no map gradients the camera form gets a NULL depth struct: same matrices
    both = RasterEngine(rows, cam.width, cam.height, DEV, resident=False, camera_grad=True, render_depth=True)
    both.set_active(sc.P)
    both.forward(*a, cam.tanfovx, cam.tanfovy)
    both.backward(dL)
    torch.cuda.synchronize()
    assert ref.worst_ratio(mats(both), m_sync, S) <= BAR
    # a plain backward on the same resident buffers starts from clean accumulator rows: it matches a fresh plain engine
    eng.backward(dL, camera_grad=False)
    torch.cuda.synchronize()
    after = {k: v.cpu().numpy().copy() for k, v in eng.grads.items()}
    plain = RasterEngine(rows, cam.width, cam.height, DEV, resident=True)
    plain.set_active(sc.P)
    for _ in range(3):
        plain.forward(*a, cam.tanfovx, cam.tanfovy)
        plain.backward(dL)
    assert plain.check() and plain._last_resident
    torch.cuda.synchronize()
    for k, v in plain.grads.items():
        assert_grad_close(k, after[k][:sc.P], v.cpu().numpy()[:sc.P])
    # forward + backward captured once and replayed reproduce the eager matrices
    assert eng.check()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        eng.forward(*a, cam.tanfovx, cam.tanfovy)
        eng.backward(dL)
    eng.dL_dviewmatrix.fill_(float("nan"))
    eng.dL_dprojmatrix.fill_(float("nan"))
    graph.replay()
    eng.after_graph_replay()
    torch.cuda.synchronize()
    assert eng.check()
    ratio = ref.worst_ratio(mats(eng), m_res, S)
    print(f"graph replay vs eager: worst err/S = {ratio:.3e}")
    assert ratio <= BAR


def _pose_matrices(xi, V0, Pm):
    """V = V0 x D(xi), PV = V x Pm in the transposed layout: xi = (axis-angle, translation) moves the camera frame,
    D = [[R^T, 0], [t, 1]] with R = exp(skew(xi[:3])) (Rodrigues).  Works for any dtype / device of xi."""
    w, t = xi[:3], xi[3:]
    th = torch.sqrt((w * w).sum())
    k = w / th
    z = torch.zeros((), dtype=xi.dtype, device=xi.device)
    K = torch.stack([torch.stack([z, -k[2], k[1]]), torch.stack([k[2], z, -k[0]]), torch.stack([-k[1], k[0], z])])
    R = torch.eye(3, dtype=xi.dtype, device=xi.device) + torch.sin(th) * K + (1 - torch.cos(th)) * (K @ K)
    D = torch.zeros((4, 4), dtype=xi.dtype, device=xi.device)
    D = D + torch.nn.functional.pad(R.T, (0, 1, 0, 1))
    D = D + torch.nn.functional.pad(t[None, :], (0, 1, 3, 0))
    last = torch.zeros((4, 4), dtype=xi.dtype, device=xi.device)
    last[3, 3] = 1
    V = V0 @ (D + last)
    return V, V @ Pm


def test_autograd_fills_the_gradient_of_a_six_dof_pose():
    from segs_slam_amd.gaussian_rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    sc = ref.scene_C()
    base = sc.camera
    xi0 = [0.02, -0.03, 0.015, 0.01, -0.02, 0.03]
    xi = torch.tensor(xi0, device=DEV, requires_grad=True)
    V, PV = _pose_matrices(xi, _t(base.world_view_transform), _t(base.projection_matrix))
    # the scene as the device sees it: the float32 matrices of the chain, handed to the oracle for the integer decisions
    sc.camera = scenes.Camera(base.width, base.height, base.fovx, base.fovy, V.detach().cpu().numpy(), base.projection_matrix,
                              PV.detach().cpu().numpy(), base.camera_center)
    cam = sc.camera
    o, _ = gs_oracle.run_scene(sc, backward=False)
    unstable = o.unstable_pixels(3e-3)
    assert unstable.mean() < 0.05 and (o.get("radii") > 0).sum() > 50
    dL, dD, dA = ref.map_weights(sc, unstable)
    # device
    leaf = lambda x: _t(x).requires_grad_(True)  # noqa: E731
    m3, op, sca, rot, col = leaf(sc.means3D), leaf(sc.opacity), leaf(sc.scales), leaf(sc.rotations), leaf(sc.colors)
    rs = GaussianRasterizationSettings(cam.height, cam.width, cam.tanfovx, cam.tanfovy, _t(sc.bg), 1.0, V.detach(), PV.detach(), 0,
                                       _t(cam.camera_center), False)
    img, radii, depth, alpha = GaussianRasterizer(rs).forward_with_camera_grad(
        m3, torch.zeros_like(m3), op, True, True, False, col, scales=sca, rotations=rot, viewmatrix=V, projmatrix=PV)
    assert np.array_equal(radii.cpu().numpy(), o.get("radii"))
    ((img * _t(dL)).sum() + (depth * _t(dD)).sum() + (alpha * _t(dA)).sum()).backward()
    have = xi.grad.cpu().numpy().astype(np.float64)
    assert m3.grad is not None and float(m3.grad.abs().max()) > 0
    # float64 truth through the same chain, and the bar carried through the chain's Jacobian
    x64 = torch.tensor(xi0, dtype=torch.float64, requires_grad=True)
    V0, Pm = torch.tensor(base.world_view_transform.astype(np.float64)), torch.tensor(base.projection_matrix.astype(np.float64))
    V64, PV64 = _pose_matrices(x64, V0, Pm)
    colour, maps = ref.render_losses(sc, o, V64, PV64, dL, dD, dA)
    (want,) = torch.autograd.grad(colour + maps, x64)
    want = want.numpy()
    jac = torch.autograd.functional.jacobian(lambda x: torch.cat([m.reshape(-1) for m in _pose_matrices(x, V0, Pm)]), x64.detach()).numpy()
    g2, gc, dz = ref.inputs_for(sc, o, dL, dD, dA)
    S = np.abs(ref.scene_contributions(sc, o, g2, gc, dz=dz)).sum(0)
    bar = (np.abs(jac) * (BAR * S)[:, None]).sum(0)
    print("pose gradient: |have - want| / bar =", np.array2string(np.abs(have - want) / bar, precision=3), " want =", want)
    assert np.all(np.abs(want) > 0) and np.all(np.abs(have - want) <= bar), (have, want, bar)
