"""Depth supervision in ScaffoldTrainerStep (depth_loss=DepthLossParams(...)): what an iteration that is handed a
sensor depth adds to the colour-only iteration, and what it leaves alone.  Shapes and keyframe of
tests/test_neural_camera_grad_gpu.py's step test; the loss kernel itself is tested in tests/test_depth_loss_gpu.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import _depth_loss_ref as ref  # noqa: E402
from tests.test_depth_loss_gpu import C_CHAIN, U  # noqa: E402
from tests.test_neural_gpu import CASES, _setup  # noqa: E402

XI = [0.02, -0.03, 0.015, 0.01, -0.02, 0.03]          # the keyframe is moved off the origin, as in the camera-gradient step test
PARAMS = ref.Params(0.8, 0.2, 0.25, False, 0.01, 40.0)
SHAPES = [(2, 37, (64, 72)), (0, 4001, (333, 187))]


def _step(case, A, W, H, depth_loss, pose_grad=False):
    from segs_slam_amd import neural_gaussians as ng, scenes
    from segs_slam_amd.depth_loss import DepthLossParams
    from segs_slam_amd.pose_refine import KeyframePose
    dev = torch.device("cuda:0")
    _, model, _ = _setup(CASES[case], A, 40 + case, dev)
    cam = scenes.make_camera(W, H, 0.9 * W, 0.9 * W, np.eye(3, dtype=np.float32), np.zeros(3, dtype=np.float32))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    kf = ng.Keyframe(t(cam.world_view_transform), t(cam.full_proj_transform), t(cam.camera_center),
                     torch.tensor([0.0, 0.1, 0.2, 1.0, 0.0, 0.0, 0.0], device=dev), cam.tanfovx, cam.tanfovy)
    pose = KeyframePose(kf, 1e-3)
    with torch.no_grad():
        pose.xi.copy_(torch.tensor(XI, dtype=torch.float64))
    kf = pose.keyframe()
    step = ng.ScaffoldTrainerStep(model, W, H, scaling_reg_weight=0.01, pose_grad=pose_grad,
                                  depth_loss=DepthLossParams(*PARAMS) if depth_loss else None)
    return step, kf


def _calibrate(step, kf):
    for _ in range(2):                    # the iterations after this take the projecting forward
        step.render(kf)
        torch.cuda.synchronize()
        assert step.engine.check()


def _sensor_depth(step):
    """A sensor depth that disagrees with the calibrating render by 20 % + 0.3 (no ties), with a band of invalid rows."""
    Z = (1.2 * step.engine.out_depth + 0.3).clone()
    Z[: Z.shape[0] // 8] = 0.0
    Z[-1, ::2] = float("nan")
    return Z


def _target(W, H, dev, seed=1):
    return torch.rand(3, H, W, device=dev, generator=torch.Generator(device=dev).manual_seed(seed))


def _check_terms(step, Z):
    terms = step.depth_terms.cpu().double()
    D, A = step.engine.out_depth.cpu(), step.engine.out_alpha.cpu()
    total, l_depth, l_alpha, n_used, N = ref.value(D, A, Z.cpu(), PARAMS)
    print(f"depth_terms {terms.tolist()}  reference {[float(total), float(l_depth), float(l_alpha), n_used]}  N {N}")
    assert N > 0 and float(terms[3]) == n_used
    for have, want in zip(terms[:3], (total, l_depth, l_alpha)):
        assert abs(float(have) - float(want)) <= C_CHAIN * U * float(want)
    return float(total)


def _calibrated_pair(case, A, W, H):
    """A step with depth supervision and one without, in the same state (same seed), both calibrated."""
    a, kf = _step(case, A, W, H, True)
    b, _ = _step(case, A, W, H, False)
    for s in (a, b):
        _calibrate(s, kf)
    assert torch.equal(a.model.params, b.model.params) and torch.equal(a.engine.out_color, b.engine.out_color)
    return a, b, kf


@pytest.mark.parametrize("case,A,size", SHAPES)
def test_iteration_with_depth_is_the_colour_iteration_plus_the_depth_term(case, A, size):
    """Each comparison starts from a fresh pair: the tile backward adds with float atomics, so two steps that have taken an
    optimizer step are no longer in the same state to the bit, with or without depth supervision."""
    W, H = size
    dev = torch.device("cuda:0")
    gt = _target(W, H, dev)
    # no depth handed over: the colour-only iteration, bit for bit, on the depth engine
    a, b, kf = _calibrated_pair(case, A, W, H)
    assert a.engine.render_depth and not b.engine.render_depth and b.depth_terms is None
    la, lb = a.training_once([kf], [gt], [None]).clone(), b.training_once([kf], [gt]).clone()
    torch.cuda.synchronize()
    assert a.engine._last_resident and b.engine._last_resident
    assert torch.equal(la, lb) and torch.equal(a.engine.out_color, b.engine.out_color) and a.depth_terms is None
    # with a depth: the same image, and the colour loss plus the depth term in one float32 addition
    a, b, kf = _calibrated_pair(case, A, W, H)
    Z = _sensor_depth(a)
    before = a.model.params.clone()
    la, lb = a.training_once([kf], [gt], [Z]).clone(), b.training_once([kf], [gt]).clone()
    torch.cuda.synchronize()
    assert a.engine._last_resident and a.engine.check() and b.engine.check()
    assert torch.equal(a.engine.out_color, b.engine.out_color)
    assert a.depth_terms.data_ptr() == a._depth_fns[(W, H)].out.data_ptr() and tuple(a.depth_terms.shape) == (4,)
    total = _check_terms(a, Z)
    assert total > 0
    assert np.float32(la.item()) == np.float32(lb.item()) + np.float32(a.depth_terms[0].item())
    moved_a, moved_b = (a.model.params - before).abs().max(), (b.model.params - before).abs().max()
    assert float(moved_a) > 0 and float((a.model.params - b.model.params).abs().max()) > 1e-3 * float(moved_b)   # it trained on the depth
    assert a.iteration == b.iteration == 1 and a.lost_steps() == 0


@pytest.mark.parametrize("case,A,size", SHAPES)
def test_pose_gradient_with_depth_and_the_raster_gradients_behind_it(case, A, size):
    from segs_slam_amd.raster_engine import RasterEngine
    W, H = size
    dev = torch.device("cuda:0")
    a, kf = _step(case, A, W, H, True, pose_grad=True)
    gt = _target(W, H, dev)
    _calibrate(a, kf)
    Z = _sensor_depth(a)
    tgt = a._depth_fns[(W, H)].prepare(Z)                            # a prepared target serves as well as the tensor
    # colour-only pose gradient first
    a.pose_gradient(kf, gt)
    torch.cuda.synchronize()
    colour = {k: v.clone() for k, v in a.pose_grads.items()}
    assert a.depth_terms is None
    state = [x.clone() for x in (a.model.params, a.model.exp_avg, a.model.exp_avg_sq)]
    count = a._mlp_count.value()
    loss = a.pose_gradient(kf, gt, tgt).clone()
    torch.cuda.synchronize()
    assert a.engine._last_resident and a.engine.check() and bool(torch.isfinite(loss))
    for x, y in zip(state, (a.model.params, a.model.exp_avg, a.model.exp_avg_sq)):
        assert torch.equal(x, y)
    assert a._mlp_count.value() == count and a.iteration == 0 and float(a.model.grads.abs().max()) == 0.0
    for k, v in a.pose_grads.items():
        assert bool(torch.isfinite(v).all()) and not torch.equal(v, colour[k]), k
    _check_terms(a, Z)
    # the raster gradients: a standalone depth engine on the step's Gaussians, fed the step's colour dL and the REFERENCE's maps
    have = {k: v.clone() for k, v in a.engine.grads.items()}
    have["mean2D"] = a.engine.dL_dmean2D.clone()
    image, depth, alpha = a.engine.out_color.clone(), a.engine.out_depth.clone(), a.engine.out_alpha.clone()
    _, dL = a.loss_fn(image, gt)
    dL = dL.clone()
    wD, wA, _ = ref.gradients(depth.cpu(), alpha.cpu(), Z.cpu(), PARAMS)
    n = a.neural
    n.forward(kf.campos, kf.pose7, a.visible_radii)                  # materialises colours and opacities
    eng = RasterEngine(n.P_capacity, W, H, dev, skip_nonpositive_opacity=True, render_depth=True)
    eng.set_active(n.P)
    image2 = eng.forward(a.bg, n.means3D, n.colors, n.opacity, n.scales, n.rotations, kf.view, kf.proj, kf.campos, kf.tanfovx, kf.tanfovy)
    assert torch.equal(image2, image) and torch.equal(eng.out_depth, depth) and torch.equal(eng.out_alpha, alpha)
    eng.backward(dL, wD.float().to(dev).contiguous(), wA.float().to(dev).contiguous())
    torch.cuda.synchronize()
    want = dict(eng.grads)
    want["mean2D"] = eng.dL_dmean2D
    for k in want:
        h, w = have[k].cpu().double(), want[k].cpu().double()
        top = float(w.abs().max())
        err = (h - w).abs()
        print(f"{k}: worst err / max|want| {float(err.max()) / top:.2e}")
        assert top > 0 and bool((err <= 1e-4 * w.abs() + 2e-5 * top).all()), k
    a.model.grads.zero_()


def test_guards():
    W, H = 64, 72
    dev = torch.device("cuda:0")
    a, kf = _step(2, 37, W, H, True)
    p, _ = _step(2, 37, W, H, True, pose_grad=True)
    b, _ = _step(2, 37, W, H, False)
    gt = _target(W, H, dev)
    with pytest.raises(ValueError, match="depth"):
        a.enable_graph(True)
    b.enable_graph(True)                                             # (the step without depth supervision still takes it)
    b.enable_graph(False)
    bad = torch.ones(H, W + 1, device=dev)
    for call in (lambda: a.training_once([kf], [gt], [bad]), lambda: p.pose_gradient(kf, gt, bad),
                 lambda: b.training_once([kf], [gt], [torch.ones(H, W, device=dev)])):
        with pytest.raises(ValueError):
            call()
    torch.cuda.synchronize()
    # nothing was launched: no iteration counted, the engines never ran
    for s in (a, p, b):
        assert s.iteration == 0 and s.engine._last is None


def test_redo_and_pyramid_levels():
    case, A, (W, H) = 0, 4001, (333, 187)
    dev = torch.device("cuda:0")
    a, kf = _step(case, A, W, H, True)                               # fresh: the first pass of each size calibrates
    g = torch.Generator(device=dev).manual_seed(3)
    depth_of = lambda w, h: 1.5 + torch.rand(h, w, device=dev, generator=g)  # noqa: E731
    gt1, z1 = _target(W, H, dev), depth_of(W, H)
    w2, h2 = W // 2, H // 2
    gt2, z2 = _target(w2, h2, dev, seed=2), depth_of(w2, h2)
    losses = [a.training_once([kf], [gt1], [z1]).clone(), a.training_once([kf], [gt1], [z1]).clone()]
    losses.append(a.training_once([kf], [gt2], [z2]).clone())
    terms = a.depth_terms.clone()
    a.finish()
    torch.cuda.synchronize()
    assert a.lost_steps() == 0 and a.iteration == 3
    assert all(bool(torch.isfinite(x)) for x in losses) and bool(torch.isfinite(terms).all()) and float(terms[0]) > 0
    fns = a._depth_fns
    assert set(fns) == {(W, H), (w2, h2)} and fns[(W, H)] is not fns[(w2, h2)]
    assert (fns[(w2, h2)].H, fns[(w2, h2)].W) == (h2, w2) and all(e.render_depth for e, _ in a._levels.values())
    assert a.depth_terms.data_ptr() == fns[(w2, h2)].out.data_ptr()
