"""GPU tests of the depth and alpha maps (segs_rasterize_*_depth; run with -m gpu on an MI355X).

  depth[p] = sum_i z_i alpha_i T_i   (view-space z, no background term)      alpha[p] = 1 - T_final[p]

with the colour's contributors.  Both are the colour of the same render with colors_precomp = (z, z, z) resp. (1, 1, 1) on a
black background (the "colour trick"), which is what the forward is checked against, and what the float64 truth of the
gradients is built from (oracle.torch_ref.render, called three times here).

Float atomics sum a Gaussian's per-tile partials in arbitrary order, so gradients of two runs -- even of the very same kernel --
agree to rounding, not bit for bit (on BASELINE config 1, dL/dcov3D of two plain backwards differ by more than 1e-6 of its
largest entry); gradients of two device paths are held to assert_grad_close, the bar of the resident-vs-synchronising tests.
"""
import numpy as np
import pytest
import torch

from oracle import gs_oracle
from segs_slam_amd import scenes
from tests.test_raster_gpu import DEV, _t, assert_grad_close, gpu_forward, gpu_state

pytestmark = pytest.mark.gpu

GRAD_NAMES = ("dL_dmean2D", "dL_dcolor", "dL_dopacity", "dL_dmean3D", "dL_dcov3D", "dL_dsh", "dL_dscale", "dL_drot")


def _small_scene(P, W, H, bg):
    sc = scenes.make_scene(P, W, H, 0.9 * W, 0.9 * W, seed=4000 + P, bg=bg)       # the scenes of test_small_scenes
    sc.scales *= 3.0
    sc.dL_dout_color[:] = (scenes.uniform01(sc.dL_dout_color.size, 55, P).reshape(sc.dL_dout_color.shape) * 2 - 1)
    return sc


SCENES = {"1000@64x64": lambda: _small_scene(1000, 64, 64, (0.1, 0.2, 0.3)), "17@33x17": lambda: _small_scene(17, 33, 17, (0, 0, 0)),
          "5000@200x120": lambda: _small_scene(5000, 200, 120, (1, 1, 1)), "1@16x16": lambda: _small_scene(1, 16, 16, (0, 0, 0)),
          "c1": lambda: scenes.make_config_scene("c1")}


def depth_forward(sc, args, colors=None, bg=None):
    from segs_slam_amd import rasterize_points as rp
    cam = sc.camera
    e = torch.empty(0, device=DEV)
    return rp.RasterizeGaussiansDepthCUDA(args["bg"] if bg is None else bg, args["means3D"], args["colors"] if colors is None else colors,
                                          args["opacity"], args["scales"], args["rotations"], sc.scale_modifier, e, args["view"],
                                          args["proj"], cam.tanfovx, cam.tanfovy, cam.height, cam.width, e, 0, args["campos"], False)


def plain_forward(sc, args, colors, bg):
    from segs_slam_amd import rasterize_points as rp
    cam = sc.camera
    e = torch.empty(0, device=DEV)
    return rp.RasterizeGaussiansCUDA(bg, args["means3D"], colors, args["opacity"], args["scales"], args["rotations"], sc.scale_modifier,
                                     e, args["view"], args["proj"], cam.tanfovx, cam.tanfovy, cam.height, cam.width, e, 0,
                                     args["campos"], False)


def depth_backward(sc, args, fwd, dL, dD, dA):
    """RasterizeGaussiansDepthBackwardCUDA on the state of depth_forward -> dict of numpy gradients."""
    from segs_slam_amd import rasterize_points as rp
    cam = sc.camera
    e = torch.empty(0, device=DEV)
    R, color, radii, depth, alpha, geom, binning, img = fwd
    out = rp.RasterizeGaussiansDepthBackwardCUDA(args["bg"], args["means3D"], radii, args["colors"], args["scales"], args["rotations"],
                                                 sc.scale_modifier, e, args["view"], args["proj"], cam.tanfovx, cam.tanfovy, dL, dD, dA,
                                                 e, 0, args["campos"], geom, R, binning, img)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in zip(GRAD_NAMES, out)}


def plain_backward(sc, args, fwd, dL):
    from segs_slam_amd import rasterize_points as rp
    cam = sc.camera
    e = torch.empty(0, device=DEV)
    R, color, radii, geom, binning, img = fwd
    out = rp.RasterizeGaussiansBackwardCUDA(args["bg"], args["means3D"], radii, args["colors"], args["scales"], args["rotations"],
                                            sc.scale_modifier, e, args["view"], args["proj"], cam.tanfovx, cam.tanfovy, dL, e, 0,
                                            args["campos"], geom, R, binning, img)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in zip(GRAD_NAMES, out)}


def close_to_max(a, b, frac=1e-6):
    return float(np.abs(a - b).max(initial=0.0)) <= frac * max(float(np.abs(b).max(initial=0.0)), 1e-30)


@pytest.mark.parametrize("name", list(SCENES))
def test_depth_forward_keeps_the_plain_outputs_and_matches_the_colour_trick(name):
    from segs_slam_amd import rasterize_points as rp
    sc = SCENES[name]()
    cam = sc.camera
    args, plain = gpu_forward(sc)
    g = gpu_state(sc, plain)
    fwd = depth_forward(sc, args)
    R, color, radii, depth, alpha, geom, binning, img = fwd
    st = rp.debug_state(sc.P, cam.width, cam.height, R, radii, geom, binning, img)
    torch.cuda.synchronize()
    # (1) colour, radii, final_T and n_contrib are the plain forward's, bit for bit
    assert R == plain[0]
    assert torch.equal(color, plain[1]) and torch.equal(radii, plain[2])
    final_T = st["final_T"].cpu().numpy()
    assert np.array_equal(final_T.view(np.uint32), g["final_T"].view(np.uint32))
    assert np.array_equal(st["n_contrib"].cpu().numpy().view(np.uint32), g["n_contrib"])
    # (2) depth = channel 0 of the render with colours (z, z, z) on black; z = the record's view depth
    z = st["depths"].reshape(-1, 1).expand(sc.P, 3).contiguous()
    black = torch.zeros(3, device=DEV)
    trick_z = plain_forward(sc, args, z, black)[1][0]
    d = depth.cpu().numpy()
    assert close_to_max(d, trick_z.cpu().numpy()), float(np.abs(d - trick_z.cpu().numpy()).max())
    # (3) alpha = 1 - final_T exactly, and the render with colours 1 on black to 2e-6
    a = alpha.cpu().numpy()
    assert np.array_equal(a, (np.float32(1.0) - final_T).astype(np.float32))
    trick_1 = plain_forward(sc, args, torch.ones(sc.P, 3, device=DEV), black)[1][0].cpu().numpy()
    assert float(np.abs(a - trick_1).max()) <= 2e-6
    if sc.P > 1:
        assert d.max() > 0 and a.max() > 0
    reached = g["n_contrib"] > 0
    assert np.all(d[~reached] == 0) and np.all(a[~reached] == 0)


def test_depth_forward_of_an_empty_scene_gives_zero_maps():
    sc = _small_scene(1000, 64, 64, (0.1, 0.2, 0.3))
    args, _ = gpu_forward(sc)
    R, color, radii, depth, alpha, *_ = depth_forward(sc, dict(args, means3D=args["means3D"][:0]))
    assert R == 0 and not bool(depth.any()) and not bool(alpha.any())


def _gradient_scene():
    """Scene and bars of test_raster_gpu.test_device_gradients_match_independent_float64_autograd."""
    sc = scenes.make_scene(3000, 160, 96, 130.0, 130.0, seed=909, bg=(0.1, 0.3, 0.2))
    sc.scales *= 2.0
    sc.dL_dout_color[:] = (scenes.uniform01(sc.dL_dout_color.size, 91, 9).reshape(sc.dL_dout_color.shape) * 2 - 1)
    return sc


def test_depth_and_alpha_gradients_match_float64_colour_trick():
    from oracle import torch_ref
    sc = _gradient_scene()
    cam = sc.camera
    o, _ = gs_oracle.run_scene(sc, backward=False)
    unstable = o.unstable_pixels(3e-3)
    assert unstable.mean() < 0.05
    rng = np.random.default_rng(77)
    dL = sc.dL_dout_color.copy()
    # weights of the same order as the colour's U(-1, 1), so that the two maps' terms are a sizeable part of every gradient
    dD = (0.5 * rng.uniform(-1, 1, (cam.height, cam.width))).astype(np.float32)
    dA = rng.uniform(-1, 1, (cam.height, cam.width)).astype(np.float32)
    for x in (dL[0], dL[1], dL[2], dD, dA):
        x[unstable] = 0.0
    args, plain = gpu_forward(sc)
    g = gpu_state(sc, plain)
    fwd = depth_forward(sc, args)
    got = depth_backward(sc, args, fwd, _t(dL), _t(dD), _t(dA))

    t64 = lambda a: torch.tensor(np.asarray(a, dtype=np.float64), requires_grad=True)  # noqa: E731
    m, s, r, op, col = t64(sc.means3D), t64(sc.scales), t64(sc.rotations), t64(sc.opacity), t64(sc.colors)
    V = torch.tensor(cam.world_view_transform, dtype=torch.float64)
    common = (torch.tensor(cam.world_view_transform), torch.tensor(cam.full_proj_transform), cam.tanfovx, cam.tanfovy, cam.height,
              cam.width, torch.tensor(g["radii"]), torch.tensor(g["means2D"]), sc.scale_modifier)
    black = torch.zeros(3, dtype=torch.float64)
    img, p1 = torch_ref.render(m, s, r, op, col, torch.tensor(sc.bg, dtype=torch.float64), *common)
    z = m @ V[:3, 2] + V[3, 2]                   # view-space z: view[2] x + view[6] y + view[10] z + view[14]
    img_z, p2 = torch_ref.render(m, s, r, op, z[:, None].expand(-1, 3), black, *common)
    img_1, p3 = torch_ref.render(m, s, r, op, torch.ones(sc.P, 3, dtype=torch.float64), black, *common)
    loss = ((img * torch.tensor(dL, dtype=torch.float64)).sum() + (img_z[0] * torch.tensor(dD, dtype=torch.float64)).sum()
            + (img_1[0] * torch.tensor(dA, dtype=torch.float64)).sum())
    loss.backward()
    ok = ~unstable
    assert float(np.abs(fwd[3].cpu().numpy() - img_z[0].detach().numpy())[ok].max()) < 2e-5 * float(img_z[0].detach().abs().max())
    assert float(np.abs(fwd[4].cpu().numpy() - img_1[0].detach().numpy())[ok].max()) < 2e-5
    truth = dict(dL_dmean3D=m.grad.numpy(), dL_dscale=s.grad.numpy(), dL_drot=r.grad.numpy(), dL_dopacity=op.grad.numpy(),
                 dL_dcolor=col.grad.numpy(), dL_dmean2D=(p1.grad + p2.grad + p3.grad).numpy()[:, :2])
    plain_g = plain_backward(sc, args, plain, _t(dL))
    for k, want in truth.items():
        if k in ("dL_dmean3D", "dL_dopacity"):   # the maps' terms matter: the colour-only backward misses the bar below
            miss = np.abs(plain_g[k].astype(np.float64).reshape(want.shape) - want)
            assert not np.all(miss <= 1e-4 * np.abs(want) + 2e-5 * np.abs(want).max()), k
        have = got[k].astype(np.float64)
        have = have[:, :2] if k == "dL_dmean2D" else have.reshape(want.shape)
        err = np.abs(have - want)
        top = np.abs(want).max()
        assert top > 0
        assert np.all(err <= 1e-4 * np.abs(want) + 2e-5 * top), (k, float(err.max() / top))
        nz = want != 0
        pure = float((err[nz] <= 1e-4 * np.abs(want[nz])).mean())
        assert pure >= 0.95, (k, pure)


@pytest.mark.parametrize("name", ["17@33x17", "c1"])
def test_null_and_zero_map_gradients_give_the_plain_backward(name):
    sc = SCENES[name]()
    cam = sc.camera
    args, plain = gpu_forward(sc)
    dL = _t(sc.dL_dout_color)
    want = plain_backward(sc, args, plain, dL)
    fwd = depth_forward(sc, args)
    zero = torch.zeros(cam.height, cam.width, device=DEV)
    for dD, dA in ((None, None), (zero, zero), (zero, None), (None, zero)):
        got = depth_backward(sc, args, fwd, dL, dD, dA)
        for k in GRAD_NAMES:   # the bar of the resident-vs-synchronising comparisons (atomic summation order)
            if want[k].size:    # (dL_dsh is (P, 0, 3) here)
                assert_grad_close(f"{k} {dD is None} {dA is None}", got[k], want[k])


def _engine_inputs(sc):
    cam = sc.camera
    return [_t(x) for x in (sc.bg, sc.means3D, sc.colors, sc.opacity, sc.scales, sc.rotations, cam.world_view_transform,
                            cam.full_proj_transform, cam.camera_center)]


def test_resident_engine_with_depth_matches_the_sync_path_and_cleans_the_depth_slot():
    from segs_slam_amd.raster_engine import RasterEngine
    sc = scenes.make_scene(30_000, 320, 240, 260.0, 260.0, seed=17, bg=(0.1, 0.2, 0.3))    # test_resident_engine_matches_sync_path
    sc.scales *= 2.0
    cam = sc.camera
    a = _engine_inputs(sc)
    dL = _t(sc.dL_dout_color)
    rng = np.random.default_rng(5)
    dD = _t(rng.uniform(-1, 1, (cam.height, cam.width)) / (cam.height * cam.width))
    dA = _t(rng.uniform(-1, 1, (cam.height, cam.width)) / (cam.height * cam.width))
    outs = []
    for resident in (False, True):
        eng = RasterEngine(sc.P, cam.width, cam.height, DEV, resident=resident, render_depth=True)
        for it in range(3):
            img = eng.forward(*a, cam.tanfovx, cam.tanfovy).clone()
            eng.backward(dL, dD, dA)
        assert eng.check()
        torch.cuda.synchronize()
        assert eng._last_resident == resident
        outs.append((img, eng.out_depth.clone(), eng.out_alpha.clone(), {k: v.cpu().numpy().copy() for k, v in eng.grads.items()}, eng))
    (i0, d0, a0, g0, _), (i1, d1, a1, g1, eng) = outs
    assert torch.equal(i0, i1) and torch.equal(d0, d1) and torch.equal(a0, a1)
    assert float(d0.max()) > 0 and float(a0.max()) > 0
    for k in g0:
        assert_grad_close(k, g1[k], g0[k])
    # a plain backward on the same resident buffers after the depth one starts from clean rows ...
    eng.backward(dL)
    torch.cuda.synchronize()
    plain = RasterEngine(sc.P, cam.width, cam.height, DEV, resident=True)
    for _ in range(3):
        plain.forward(*a, cam.tanfovx, cam.tanfovy)
        plain.backward(dL)
    assert plain.check() and plain._last_resident
    torch.cuda.synchronize()
    for k, v in plain.grads.items():
        assert_grad_close(k, eng.grads[k].cpu().numpy(), v.cpu().numpy())
    # ... and so does a depth backward after it: row dword [9] was cleared by every backward in between
    eng.backward(dL, dD, dA)
    torch.cuda.synchronize()
    for k in g1:
        assert_grad_close(k, eng.grads[k].cpu().numpy(), g1[k])


def test_projected_forward_gives_the_depth_maps_of_the_unfused_forward():
    from segs_slam_amd.raster_engine import RasterEngine
    from tests.test_neural_gpu import _projecting_pair
    a, b, kf, cam = _projecting_pair(1, 4000, 41, 320, 240, False)      # case 1 of test_projecting_forward_equals_forward_plus_k1
    for step in (a, b):
        step.engine = RasterEngine(step.engine.P, cam.width, cam.height, DEV, resident=True, skip_nonpositive_opacity=True,
                                   render_depth=True)
        step._levels[(step.W, step.H)] = (step.engine, step.loss_fn)
    for it in range(3):
        ia, ib = a.render(kf), b.render(kf)
        torch.cuda.synchronize()
        assert a.engine.check() and b.engine.check()
        assert b.engine._last_resident == (it > 0)
        assert torch.equal(ia, ib), it
        assert torch.equal(a.engine.out_depth, b.engine.out_depth), it
        assert torch.equal(a.engine.out_alpha, b.engine.out_alpha), it
    assert float(b.engine.out_alpha.max()) > 0 and float(b.engine.out_depth.max()) > 0


def test_autograd_depth_function_equals_direct_abi_calls():
    from segs_slam_amd.gaussian_rasterizer import GaussianRasterizationSettings, GaussianRasterizer, rasterizeGaussiansWithDepth
    sc = scenes.make_scene(3000, 96, 80, 80.0, 80.0, seed=91, bg=(0.1, 0.0, 0.2))    # test_autograd_module_matches_oracle
    sc.scales *= 3.0
    cam = sc.camera
    rng = np.random.default_rng(3)
    gC = _t(rng.uniform(-1, 1, (3, cam.height, cam.width)))
    gD = _t(rng.uniform(-1, 1, (cam.height, cam.width)))
    gA = _t(rng.uniform(-1, 1, (cam.height, cam.width)))
    args, _ = gpu_forward(sc)
    fwd = depth_forward(sc, args)
    want = depth_backward(sc, args, fwd, gC, gD, gA)
    rs = GaussianRasterizationSettings(cam.height, cam.width, cam.tanfovx, cam.tanfovy, args["bg"], 1.0, args["view"], args["proj"], 0,
                                       args["campos"], False)
    leaf = lambda a: _t(a).requires_grad_(True)  # noqa: E731
    m3, op, sca, rot, col = leaf(sc.means3D), leaf(sc.opacity), leaf(sc.scales), leaf(sc.rotations), leaf(sc.colors)
    means2D = torch.zeros_like(m3, requires_grad=True)
    e = torch.empty(0, device=DEV)
    img, radii, depth, alpha = rasterizeGaussiansWithDepth(m3, means2D, e, col, op, sca, rot, e, rs)
    assert torch.equal(img, fwd[1]) and torch.equal(radii, fwd[2]) and torch.equal(depth, fwd[3]) and torch.equal(alpha, fwd[4])
    ((img * gC).sum() + (depth * gD).sum() + (alpha * gA).sum()).backward()
    for have, k in ((m3, "dL_dmean3D"), (op, "dL_dopacity"), (sca, "dL_dscale"), (rot, "dL_drot"), (col, "dL_dcolor")):
        assert_grad_close(k, have.grad.cpu().numpy(), want[k].reshape(have.shape))
    assert_grad_close("dL_dmean2D", means2D.grad.cpu().numpy(), want["dL_dmean2D"])
    # the module method, and a loss on the depth map alone (the colour's gradient is then zero)
    rast = GaussianRasterizer(rs)
    for t in (m3, op, sca, rot, col):
        t.grad = None
    img2, _, depth2, alpha2 = rast.forward_with_depth(m3, means2D, op, False, True, True, True, False, colors_precomp=col, scales=sca,
                                                      rotations=rot)
    assert torch.equal(depth2, depth) and torch.equal(alpha2, alpha)
    (depth2 * gD).sum().backward()
    only_d = depth_backward(sc, args, fwd, torch.zeros_like(gC), gD, None)
    assert_grad_close("dL_dmean3D depth only", m3.grad.cpu().numpy(), only_d["dL_dmean3D"])
    assert not bool(col.grad.any())
