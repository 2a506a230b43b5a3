"""dL/d(camera centre) of the neural-Gaussian generator (segs_neural_backward_camera, include/segs_neural.h)
against the float64 restatement of src/gaussian_renderer.cpp:214-334 (oracle/neural_ref.py).

The reference side takes a (V, 3) camera-centre leaf, one row per visible anchor: it broadcasts in `anc - camera_center`, its row
gradients are the per-anchor contributions -g_a, `want = rows.sum(0)` is the gradient of a (3,) leaf and `S = rows.abs().sum(0)`
the scale of the bar.  The three sums cancel to 0.1 - 7 % of S, so the bar is relative to S and not to the result:
|have_k - want_k| <= 1e-4 S_k, the project's per-Gaussian relative gradient bar carried through the sum."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import neural_ref  # noqa: E402
from tests.test_neural_gpu import CASES, _setup  # noqa: E402

BAR = 1e-4
CAMPOS = (0.1, -0.2, -0.5)
POSE7 = (0.3, -0.1, 0.2, 0.9, 0.1, -0.3, 0.2)
ONE_KERNEL = 1          # SEGS_NEURAL_ONE_KERNEL_BACKWARD


def _reference(rd, tensors, visible, dmask, campos, pose7, grads, reg_w, rdev):
    """Float64 restatement on the device's mask with a (V, 3) camera-centre leaf.  Anchors with a ReLU input within 1e-5 of zero
    get no upstream gradient (`grads`, candidate-domain weights on the CPU, are zeroed IN PLACE on their rows, as
    tests/test_neural_gpu.py::_check_parity does).  Returns (rows (V, 3), dL/danchor (A, 3), kink (A,) bool, reg)."""
    anchor, offset, feat, scaling_log, mlp = tensors
    A = anchor.shape[0]
    V = int(visible.sum())
    leaf = lambda t: t.to(rdev, torch.float64).requires_grad_(True)  # noqa: E731
    r = [leaf(t) for t in (anchor, offset, feat, scaling_log)] + [{k: leaf(v) for k, v in mlp.items()}]
    cam = campos.to(rdev, torch.float64).reshape(1, 3).repeat(V, 1).requires_grad_(True)
    vis_rows = visible.repeat_interleave(10).to(rdev)
    relu_inputs = []
    out = neural_ref.generate_neural_gaussians(rd, *r, cam, pose7.to(rdev, torch.float64), visible.to(rdev), mask=dmask[vis_rows],
                                               relu_inputs=relu_inputs)
    margin = torch.stack([x.detach().abs().min(1).values for x in relu_inputs]).min(0).values
    kink = torch.zeros(A, dtype=torch.bool)
    kink[visible] = (margin < 1e-5).cpu()
    kink_rows = kink.repeat_interleave(10)
    for t in grads:
        t[kink_rows] = 0.0
    xyz, color, opacity, scaling, rot = out[:5]
    c = lambda t: t.to(rdev, torch.float64)[dmask]  # noqa: E731
    gm, gc, go, gs, gr = grads
    reg = reg_w * scaling.prod(1).mean() if scaling.shape[0] else torch.zeros((), dtype=torch.float64, device=rdev)
    loss = ((xyz * c(gm)).sum() + (color * c(gc)).sum() + (opacity * c(go)).sum() + (scaling * c(gs)).sum() + (rot * c(gr)).sum()) + 1e4 * reg
    loss.backward()
    return cam.grad.detach().cpu(), r[0].grad.detach().cpu(), kink, reg


def _stage(case, A, visible, seed, gseed, reg_w=0.01, flags=0, ref_device="cuda:0"):
    """Device forward + camera backward of CASES[case] against the float64 reference.  Returns
    (have (3,), want (3,), S (3,), kinks, visible count, dL/danchor of the reference)."""
    from segs_slam_amd import _capi, neural_gaussians as ng
    dev = torch.device("cuda:0")
    rd, model, tensors = _setup(CASES[case], A, seed, dev)
    g = torch.Generator().manual_seed(gseed)
    campos, pose7 = torch.tensor(CAMPOS), torch.tensor(POSE7)
    radii = torch.where(visible, torch.tensor(3), torch.tensor(0)).to(torch.int32)
    P = A * 10
    grads = [torch.randn(P, n, generator=g) for n in (3, 3, 1, 3, 4)]
    gen = ng.NeuralGaussians(model)
    gen.forward(campos.to(dev), pose7.to(dev), radii.to(dev))
    torch.cuda.synchronize()
    dmask = gen.mask().to(ref_device)
    rows, danchor, kink, _ = _reference(rd, tensors, visible, dmask, campos, pose7, grads, reg_w, torch.device(ref_device))
    model.grads.zero_()
    lib = _capi.lib()
    old = lib.segs_neural_set_flags(flags)
    try:
        gen.backward(*(t.to(dev) for t in grads), scaling_reg_weight=1e4 * reg_w, camera_grad=True)
    finally:
        assert lib.segs_neural_set_flags(old) == flags
    torch.cuda.synchronize()
    have = gen.dL_dcamera_center.cpu().double()
    return have, rows.sum(0), rows.abs().sum(0), int(kink.sum()), int(visible.sum()), danchor


def _assert_within_bar(have, want, S, kinks, V, what):
    ratio = (have - want).abs() / S
    print(f"{what}: visible {V} kinks {kinks}  err/S {[f'{float(x):.2e}' for x in ratio]}  |sum|/S {[f'{float(x):.2e}' for x in want.abs() / S]}")
    assert kinks < 0.02 * V, (kinks, V)
    assert bool((S > 0).all())
    assert bool(((have - want).abs() <= BAR * S).all()), f"{what}: err / S = {ratio.tolist()}"


@pytest.mark.parametrize("case", range(len(CASES)))
@pytest.mark.parametrize("A", [1, 700])
def test_camera_centre_gradient_matches_float64(case, A):
    g = torch.Generator().manual_seed(7 + case)
    visible = torch.rand(A, generator=g) < 0.7
    if A == 1:
        visible[:] = True
    have, want, S, kinks, V, _ = _stage(case, A, visible, 300 + case, 1007 + case, ref_device="cpu")
    _assert_within_bar(have, want, S, kinks, V, f"case {case} A {A}")


def _scattered(n_visible, case):
    """n_visible visible anchors with about 10 % invisible ones scattered among them (the compaction reorders them)."""
    g = torch.Generator().manual_seed(n_visible + 17 * case)
    A = n_visible + max(1, n_visible // 9)
    visible = torch.zeros(A, dtype=torch.bool)
    visible[torch.randperm(A, generator=g)[:n_visible]] = True
    return A, visible


# 31 / 33: the slab of 32 anchors; 129: the second workgroup; 32 769: the second round of the 256 persistent workgroups, where an
# accumulator that does not survive the loop would show.  Case 0: feature bank, case 5: plain; flags 1: the one-kernel family.
COUNT_PARAMS = [(c, n, 0) for n in (31, 33, 129, 32769) for c in (0, 5)] + [(5, 129, ONE_KERNEL), (0, 129, ONE_KERNEL), (5, 32769, ONE_KERNEL)]
# Both families at the counts of tests/test_neural_backward_forms_gpu.py: one anchor; 231 of 256 (the second workgroup's last slab
# has 7 anchors); 32 936 = 32 768 + 128 + 40 (second round: a pair with 8 valid lanes next to two empty pairs, whose lanes carry a
# copy of the last anchor and must add nothing to the workgroup's row).
COUNT_PARAMS += [(c, n, f) for n in (1, 231, 32936) for c in (0, 5) for f in (0, ONE_KERNEL)]


@pytest.mark.parametrize("case,n_visible,flags", COUNT_PARAMS)
def test_camera_centre_gradient_at_kernel_unit_counts(case, n_visible, flags):
    A, visible = _scattered(n_visible, case)
    have, want, S, kinks, V, _ = _stage(case, A, visible, 500 + case, 11 + case, flags=flags)
    _assert_within_bar(have, want, S, kinks, V, f"case {case} visible {n_visible} flags {flags}")


def test_camera_centre_gradient_after_the_projecting_forward():
    """The visible list of segs_neural_forward_projected (which works out prefilter_voxel's radii itself) serves the camera backward
    as segs_neural_forward's does."""
    from segs_slam_amd import neural_gaussians as ng, scenes
    dev = torch.device("cuda:0")
    case, A = 0, 4001
    rd, model, tensors = _setup(CASES[case], A, 40 + case, dev)
    cam = scenes.make_camera(333, 187, 0.9 * 333, 0.9 * 333, np.eye(3, dtype=np.float32), np.zeros(3, dtype=np.float32))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    kf = ng.Keyframe(t(cam.world_view_transform), t(cam.full_proj_transform), t(cam.camera_center),
                     torch.tensor([0.0, 0.1, 0.2, 1.0, 0.0, 0.0, 0.0], device=dev), cam.tanfovx, cam.tanfovy)
    step = ng.ScaffoldTrainerStep(model, cam.width, cam.height)
    for _ in range(2):            # the first render calibrates the resident buffers, the second takes the projecting forward
        step.render(kf)
        torch.cuda.synchronize()
        assert step.engine.check()
    assert step.engine._last_resident
    visible = (step.visible_radii[:A] > 0).cpu()
    V = int(visible.sum())
    assert 0 < V < A
    g = torch.Generator().manual_seed(5)
    grads = [torch.randn(A * 10, n, generator=g) for n in (3, 3, 1, 3, 4)]
    rows, _, kink, _ = _reference(rd, tensors, visible, step.neural.mask(), kf.campos.cpu(), kf.pose7.cpu(), grads, 0.0, dev)
    model.grads.zero_()
    step.neural.backward(*(x.to(dev) for x in grads), camera_grad=True)
    torch.cuda.synchronize()
    _assert_within_bar(step.neural.dL_dcamera_center.cpu().double(), rows.sum(0), rows.abs().sum(0), int(kink.sum()), V, "projected")


@pytest.mark.parametrize("case", [2, 0])          # every add_*_dist; the feature bank
def test_the_bar_sees_a_detached_distance_and_an_included_anchor_path(case, monkeypatch):
    """Reference side only: the two likely mistakes of a kernel -- no gradient through ob_dist, or the xyz = anchor + offset *
    scaling path (danc) left in -- move `want` by more than the bar in at least one component."""
    A = 700
    g = torch.Generator().manual_seed(7 + case)
    visible = torch.rand(A, generator=g) < 0.7
    rd = neural_ref.NeuralDims(**CASES[case])
    tensors = neural_ref.random_model(rd, A, 300 + case)
    campos, pose7 = torch.tensor(CAMPOS), torch.tensor(POSE7)
    cpu = torch.device("cpu")

    def run():
        gg = torch.Generator().manual_seed(1007 + case)
        grads = [torch.randn(A * 10, n, generator=gg) for n in (3, 3, 1, 3, 4)]
        with torch.no_grad():
            out = neural_ref.generate_neural_gaussians(rd, *(x.double() if torch.is_tensor(x) else {k: v.double() for k, v in x.items()} for x in tensors),
                                                       campos.double(), pose7.double(), visible)
        full = torch.zeros(A * 10, dtype=torch.bool)
        full[visible.repeat_interleave(10)] = out[6]
        return _reference(rd, tensors, visible, full, campos, pose7, grads, 0.01, cpu)

    rows, danchor, _, _ = run()
    want, S = rows.sum(0), rows.abs().sum(0)
    norm = torch.linalg.norm
    monkeypatch.setattr(torch.linalg, "norm", lambda *a, **k: norm(*a, **k).detach())
    rows_detached = run()[0]
    monkeypatch.undo()
    assert bool(((rows_detached.sum(0) - want).abs() > BAR * S).any())
    with_danc = -danchor[visible].sum(0)
    assert bool(((with_danc - want).abs() > BAR * S).any())


def _plain_and_camera(case, A, visible, flags, null_pointer=False):
    """model.grads after segs_neural_backward (twice, from zero each time) and after segs_neural_backward_camera."""
    from segs_slam_amd import _capi, neural_gaussians as ng
    from segs_slam_amd.neural_gaussians import _p
    dev = torch.device("cuda:0")
    lib = _capi.lib()
    rd, model, _ = _setup(CASES[case], A, 500 + case, dev)
    g = torch.Generator().manual_seed(3)
    grads = [torch.randn(A * 10, n, generator=g).to(dev) for n in (3, 3, 1, 3, 4)]
    radii = torch.where(visible, torch.tensor(3), torch.tensor(0)).to(torch.int32).to(dev)
    gen = ng.NeuralGaussians(model)
    gen.forward(torch.tensor(CAMPOS, device=dev), torch.tensor(POSE7, device=dev), radii)
    outs = []
    old = lib.segs_neural_set_flags(flags)
    try:
        for kind in ("plain", "plain", "camera"):
            model.grads.zero_()
            if kind == "plain":
                gen.backward(*grads, scaling_reg_weight=0.01)
            elif not null_pointer:
                gen.backward(*grads, scaling_reg_weight=0.01, camera_grad=True)
            else:
                m = model
                st = lib.segs_neural_backward_camera(
                    C.byref(m._cdims), m.A, _p(m.param("anchor")), _p(m.param("offset")), _p(m.param("anchor_feat")), _p(m.param("scaling")),
                    _p(m.mlp_params), _p(gen._last[0]), _p(gen._last[1]), *(_p(x) for x in grads), _p(m.grad("anchor")), _p(m.grad("offset")),
                    _p(m.grad("anchor_feat")), _p(m.grad("scaling")), _p(m.mlp_grads), 0.01, _p(gen.scaling_reg), None, _p(gen.temp), gen._stream())
                _capi.check(st, "segs_neural_backward_camera")
            torch.cuda.synchronize()
            outs.append(model.grads.clone())
    finally:
        assert lib.segs_neural_set_flags(old) == flags
    return outs, A * (3 + 30 + 32 + 6)


@pytest.mark.parametrize("case,flags,null_pointer", [(0, 0, False), (5, 0, False), (5, ONE_KERNEL, False), (0, ONE_KERNEL, False), (5, 0, True)])
def test_the_camera_backward_leaves_every_other_gradient_as_it_was(case, flags, null_pointer):
    A, visible = _scattered(33_000, case)
    (p0, p1, cam), n_anchor = _plain_and_camera(case, A, visible, flags, null_pointer)
    assert float(p0.abs().max()) > 0
    assert torch.equal(p0[:n_anchor], cam[:n_anchor])            # the four per-anchor tensors
    if torch.equal(p0, p1):                                      # two plain calls give the same bits: so must the camera form
        assert torch.equal(p0, cam)
    else:
        scale = float(p0[n_anchor:].abs().max())
        assert float((p0[n_anchor:] - cam[n_anchor:]).abs().max()) <= 1e-6 * scale


def test_no_visible_anchor_gives_exactly_zero():
    from segs_slam_amd import neural_gaussians as ng
    dev = torch.device("cuda:0")
    for case in (0, 2):           # appearance_finish_kernel / no finishing kernel at all (no appearance, no regulariser)
        rd, model, _ = _setup(CASES[case], 300, 5, dev)
        gen = ng.NeuralGaussians(model)
        gen.forward(torch.zeros(3, device=dev), torch.zeros(7, device=dev), torch.zeros(300, dtype=torch.int32, device=dev))
        gen.dL_dcamera_center = torch.full((3,), 5.0, device=dev)
        z = torch.zeros(3000, 4, device=dev)
        gen.backward(z[:, :3].contiguous(), z[:, :3].contiguous(), z[:, :1].contiguous(), z[:, :3].contiguous(), z, camera_grad=True)
        torch.cuda.synchronize()
        assert gen.dL_dcamera_center.tolist() == [0.0, 0.0, 0.0]
        assert float(model.grads.abs().max()) == 0.0


@pytest.mark.parametrize("case", [0, 4])          # case 4: appearance_dim 0 and no regulariser -- no finishing kernel runs
def test_the_output_is_overwritten_and_repeats_bit_for_bit(case):
    from segs_slam_amd import neural_gaussians as ng
    dev = torch.device("cuda:0")
    A, visible = _scattered(33_000, case)
    rd, model, _ = _setup(CASES[case], A, 500 + case, dev)
    g = torch.Generator().manual_seed(3)
    grads = [torch.randn(A * 10, n, generator=g).to(dev) for n in (3, 3, 1, 3, 4)]
    gen = ng.NeuralGaussians(model)
    gen.forward(torch.tensor(CAMPOS, device=dev), torch.tensor(POSE7, device=dev),
                torch.where(visible, torch.tensor(3), torch.tensor(0)).to(torch.int32).to(dev))
    model.grads.zero_()
    gen.backward(*grads, camera_grad=True)
    first, g1 = gen.dL_dcamera_center.clone(), model.grad("anchor_feat").clone()
    buf = gen.dL_dcamera_center.data_ptr()
    gen.backward(*grads, camera_grad=True)
    torch.cuda.synchronize()
    assert gen.dL_dcamera_center.data_ptr() == buf               # made once
    assert float(first.abs().min()) > 0
    assert torch.equal(gen.dL_dcamera_center, first)             # not doubled, and the same bits
    assert torch.equal(model.grad("anchor_feat"), 2 * g1)        # while the model's gradients accumulate


# ---- the step ---------------------------------------------------------------------------------------------------------------------
def _step_and_keyframe(case, A, W, H, seed, pose_grad, xi=None):
    """A ScaffoldTrainerStep over CASES[case] and a keyframe at the origin looking down +z (moved by `xi` through
    pose_refine.KeyframePose when given) -> (step, keyframe, KeyframePose or None, model tensors, reference dims)."""
    from segs_slam_amd import neural_gaussians as ng, scenes
    from segs_slam_amd.pose_refine import KeyframePose
    dev = torch.device("cuda:0")
    rd, model, tensors = _setup(CASES[case], A, seed, dev)
    cam = scenes.make_camera(W, H, 0.9 * W, 0.9 * W, np.eye(3, dtype=np.float32), np.zeros(3, dtype=np.float32))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    kf = ng.Keyframe(t(cam.world_view_transform), t(cam.full_proj_transform), t(cam.camera_center),
                     torch.tensor([0.0, 0.1, 0.2, 1.0, 0.0, 0.0, 0.0], device=dev), cam.tanfovx, cam.tanfovy)
    pose = None
    if xi is not None:
        pose = KeyframePose(kf, 1e-3)
        with torch.no_grad():
            pose.xi.copy_(torch.tensor(xi, dtype=torch.float64))
        kf = pose.keyframe()
    step = ng.ScaffoldTrainerStep(model, W, H, scaling_reg_weight=0.01, pose_grad=pose_grad)
    return step, kf, pose, tensors, rd, cam


def _oracle_scene(step, kf, cam, dL):
    """The Gaussians the step rasterized (the kept candidates, compacted as the reference compacts them) as a CPU-oracle scene seen
    through the keyframe's float32 matrices."""
    from segs_slam_amd import scenes
    n = step.neural
    mask = n.mask()
    c = lambda x: x[:n.P][mask].cpu().numpy()  # noqa: E731
    camera = scenes.Camera(cam.width, cam.height, cam.fovx, cam.fovy, kf.view.cpu().numpy(), cam.projection_matrix, kf.proj.cpu().numpy(),
                           kf.campos.cpu().numpy())
    return scenes.Scene("step", camera, c(n.means3D), c(n.scales), c(n.rotations), c(n.opacity), c(n.colors), step.bg.cpu().numpy(),
                        np.ascontiguousarray(dL)), mask


def _raster_S(sc, dL):
    """S_k of the 32 matrix entries: the absolute sum of the per-Gaussian contributions (closed form of test_camera_grad_cpu.py fed
    the CPU oracle's dL_dmean2D / dL_dconic) -> (oracle, S (32,))."""
    from oracle import gs_oracle
    from tests import test_camera_grad_cpu as ref
    o, _ = gs_oracle.run_scene(sc, backward=False)
    g2, gc, _ = ref.inputs_for(sc, o, dL)
    return o, np.abs(ref.scene_contributions(sc, o, g2, gc)).sum(0)


@pytest.mark.parametrize("case,A,size", [(2, 37, (64, 72)), (0, 4001, (333, 187))])
def test_step_pose_gradients_are_the_camera_forms_of_both_backwards(case, A, size):
    """ScaffoldTrainerStep(pose_grad=True): what `pose_grads` holds, what pose_gradient() leaves alone, and that the iteration
    itself is unchanged."""
    from segs_slam_amd import neural_gaussians as ng
    from segs_slam_amd.raster_engine import RasterEngine
    from tests import test_camera_grad_cpu as ref
    dev = torch.device("cuda:0")
    W, H = size
    # The keyframe is moved a little off the origin.  At view = identity the contribution of every single Gaussian to
    # dL/dview[8] and dL/dview[9] vanishes analytically (dt_i p_z and J^T dM2 cancel inside the Gaussian), S_k of those two
    # entries is 1e-19 in float64 and no scale for anything; off the identity every live entry has a per-Gaussian scale.
    xi = [0.02, -0.03, 0.015, 0.01, -0.02, 0.03]
    a, kf, _, _, _, cam = _step_and_keyframe(case, A, W, H, 40 + case, True, xi=xi)
    b = _step_and_keyframe(case, A, W, H, 40 + case, False, xi=xi)[0]
    gt = torch.rand(3, H, W, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    with pytest.raises(ValueError):
        a.enable_graph(True)
    with pytest.raises(ValueError):
        b.pose_gradient(kf, gt)
    assert b.pose_grads is None and all(e.camera_grad for e, _ in a._levels.values()) and not b.engine.camera_grad
    for s in (a, b):                      # calibrate the resident buffers: the iterations below take the projecting forward
        for _ in range(2):
            s.render(kf)
            torch.cuda.synchronize()
            assert s.engine.check()
    # pose_gradient: no optimizer step
    state = [x.clone() for x in (a.model.params, a.model.exp_avg, a.model.exp_avg_sq)]
    count = a._mlp_count.value()
    loss_p = a.pose_gradient(kf, gt).clone()
    torch.cuda.synchronize()
    assert a.engine._last_resident and a.engine.check()
    for x, y in zip(state, (a.model.params, a.model.exp_avg, a.model.exp_avg_sq)):
        assert torch.equal(x, y)
    assert a._mlp_count.value() == count and a.iteration == 0 and float(a.model.grads.abs().max()) == 0.0
    pg = {k: v.clone() for k, v in a.pose_grads.items()}
    assert {k: tuple(v.shape) for k, v in pg.items()} == {"viewmatrix": (4, 4), "projmatrix": (4, 4), "camera_center": (3,)}
    assert a.pose_grads["viewmatrix"].data_ptr() == a.engine.dL_dviewmatrix.data_ptr()
    assert a.pose_grads["camera_center"].data_ptr() == a.neural.dL_dcamera_center.data_ptr()
    assert all(float(v.abs().max()) > 0 for v in pg.values())
    # camera centre: the standalone camera backward on the step's own raster gradients (same forward state: the same bits)
    g = a.engine.grads
    a.neural.dL_dcamera_center.fill_(7.0)
    a.neural.backward(g["means3D"], g["colors"], g["opacity"], g["scales"], g["rotations"], a.scaling_reg_weight, camera_grad=True)
    torch.cuda.synchronize()
    assert torch.equal(a.neural.dL_dcamera_center, pg["camera_center"])
    a.model.grads.zero_()
    # the two matrices: a standalone engine on the step's Gaussians and the step's dL, within 1e-6 S (the tile backward's atomics)
    image = a.engine.out_color.clone()
    _, dL = a.loss_fn(image, gt)
    dL = dL.clone()
    n = a.neural
    n.forward(kf.campos, kf.pose7, a.visible_radii)            # materialises colours and opacities (the projecting forward does not)
    eng = RasterEngine(n.P_capacity, W, H, dev, skip_nonpositive_opacity=True, camera_grad=True)
    eng.set_active(n.P)
    image2 = eng.forward(a.bg, n.means3D, n.colors, n.opacity, n.scales, n.rotations, kf.view, kf.proj, kf.campos, kf.tanfovx, kf.tanfovy)
    assert torch.equal(image2, image)
    eng.backward(dL)
    torch.cuda.synchronize()
    sc, _ = _oracle_scene(a, kf, cam, dL.cpu().numpy())
    _, S = _raster_S(sc, sc.dL_dout_color)
    have = torch.cat([pg["viewmatrix"].reshape(-1), pg["projmatrix"].reshape(-1)]).cpu().numpy()
    alone = torch.cat([eng.dL_dviewmatrix.reshape(-1), eng.dL_dprojmatrix.reshape(-1)]).cpu().numpy()
    print("have ", np.array2string(have, precision=4), "\nalone", np.array2string(alone, precision=4), "\nS    ", np.array2string(S, precision=4))
    ratio = ref.worst_ratio(have, alone, S)
    print(f"step vs standalone engine, case {case} A {A}: worst |diff| / S = {ratio:.3e}")
    assert ratio <= 1e-6
    # an iteration with pose gradients is the iteration without them: same loss, same image, from the same state
    la, lb = a.training_once([kf], [gt]).clone(), b.training_once([kf], [gt]).clone()
    torch.cuda.synchronize()
    assert torch.equal(la, lb) and torch.equal(la, loss_p) and torch.equal(a.engine.out_color, b.engine.out_color)
    assert torch.equal(a.engine.out_color, image)
    assert a.pose_grads is not None and b.pose_grads is None and a.iteration == 1


def test_six_dof_pose_gradient_end_to_end():
    """xi.grad of KeyframePose.accumulate(pose_grads) against float64: the render's camera partial at the device's Gaussians
    (torch_ref through V(xi), PV(xi), the device's dL) plus the generator's partial through c(xi) with the device's
    candidate-domain gradients as fixed weights; their sum is the total derivative.  Bar: the 1e-4 S_k of the 16 + 16 + 3 inputs
    carried through the chain's Jacobian."""
    from segs_slam_amd.pose_refine import pose_chain
    from tests import test_camera_grad_cpu as ref
    dev = torch.device("cuda:0")
    case, A, W, H = 0, 200, 96, 64
    xi0 = [0.02, -0.03, 0.015, 0.01, -0.02, 0.03]
    step, kf, pose, tensors, rd, cam = _step_and_keyframe(case, A, W, H, 40 + case, True, xi=xi0)
    step.fuse_projection = False          # colours and opacities are materialised for the oracle scene
    for _ in range(2):
        step.render(kf)
        torch.cuda.synchronize()
        assert step.engine.check()
    # the loss: fixed random weights on the image, zero where the tile membership of a pixel is within rounding
    from oracle import gs_oracle
    rng = np.random.default_rng(5)
    dL = rng.uniform(-1, 1, (3, H, W)).astype(np.float32)
    sc, mask = _oracle_scene(step, kf, cam, dL)
    o, _ = gs_oracle.run_scene(sc, backward=False)
    unstable = o.unstable_pixels(3e-3)
    assert unstable.mean() < 0.05 and (o.get("radii") > 0).sum() > 50
    dL[:, unstable] = 0.0
    sc.dL_dout_color = dL
    assert np.array_equal(step.engine.radii[:step.neural.P][mask].cpu().numpy(), o.get("radii"))
    # device: raster backward with camera gradients, then the generator's; anchors at a ReLU kink get no upstream gradient
    g = {k: v.clone() for k, v in step.engine.backward(torch.from_numpy(dL).to(dev)).items()}
    visible = (step.visible_radii[:A] > 0).cpu()
    grads = [g[k][:A * 10].cpu().reshape(A * 10, -1) for k in ("means3D", "colors", "opacity", "scales", "rotations")]
    rows, _, kink, _ = _reference(rd, tensors, visible, step.neural.mask(), kf.campos.cpu(), kf.pose7.cpu(), grads, 0.0, dev)
    assert int(kink.sum()) < 0.02 * int(visible.sum())
    step.model.grads.zero_()
    step.neural.backward(*(x.to(dev).contiguous() for x in grads), camera_grad=True)
    torch.cuda.synchronize()
    pose_grads = {"viewmatrix": step.engine.dL_dviewmatrix, "projmatrix": step.engine.dL_dprojmatrix, "camera_center": step.neural.dL_dcamera_center}
    pose.accumulate(pose_grads)
    have = pose.xi.grad.cpu().numpy()
    # float64
    x64 = torch.tensor(xi0, dtype=torch.float64, requires_grad=True)
    V0, Pm = pose.V0.cpu(), pose.Pm.cpu()
    V64, PV64, c64 = pose_chain(x64, V0, Pm)
    colour, _ = ref.render_losses(sc, o, V64, PV64, dL)
    want_c, S_c = rows.sum(0), rows.abs().sum(0)
    (want,) = torch.autograd.grad(colour + (c64 * want_c).sum(), x64)
    want = want.numpy()
    jac = torch.autograd.functional.jacobian(lambda x: torch.cat([m.reshape(-1) for m in pose_chain(x, V0, Pm)]), x64.detach()).numpy()
    g2, gc, _ = ref.inputs_for(sc, o, dL)
    S = np.concatenate([np.abs(ref.scene_contributions(sc, o, g2, gc)).sum(0), S_c.numpy()])
    bar = (np.abs(jac) * (BAR * S)[:, None]).sum(0)
    print("six-dof pose gradient: |have - want| / bar =", np.array2string(np.abs(have - want) / bar, precision=3), " want =", want)
    assert np.all(np.abs(want) > 0) and np.all(np.abs(have - want) <= bar), (have, want, bar)
