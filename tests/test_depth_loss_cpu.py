"""Host-side checks of the depth-supervision loss (include/segs_train.h): the float64 reference the GPU tests
compare against is consistent with autograd, the library's size queries answer without a GPU, and the host object validates
its parameters."""
import pytest
import torch

from tests import _depth_loss_ref as ref


def _inputs(H, W, seed, normalize):
    """Random maps without ties: |d - Z| >= 0.25 d on every pixel, opacities off the silhouette threshold."""
    g = torch.Generator().manual_seed(seed)
    A = 0.05 + 0.95 * torch.rand(H, W, generator=g, dtype=torch.float64)
    D = A * (0.5 + 4.5 * torch.rand(H, W, generator=g, dtype=torch.float64))
    d = D / A if normalize else D
    r = 0.25 + 0.25 * torch.rand(H, W, generator=g, dtype=torch.float64)
    Z = d * torch.where(torch.rand(H, W, generator=g) < 0.5, 1 + r, 1 - r)
    flat = Z.view(-1)
    flat[0], flat[5], flat[11], flat[17], flat[23] = float("nan"), float("inf"), 0.0, -1.0, 50.0     # invalid (max_depth 10)
    return D, A, Z


@pytest.mark.parametrize("p", [ref.Params(1.0, 0.0, 0.0, False, 0.01, 10.0), ref.Params(0.7, 0.3, 0.5, False, 0.01, 10.0),
                               ref.Params(1.0, 0.1, 0.5, True, 0.01, 10.0), ref.Params(0.5, 0.2, 0.25, True, 0.0, 0.0)])
def test_closed_form_gradients_equal_autograd(p):
    D, A, Z = _inputs(19, 23, 3, p.normalize)
    D.requires_grad_(True)
    A.requires_grad_(True)
    total, l_depth, l_alpha, n_used, N = ref.value(D, A, Z, p)
    assert 0 < n_used <= N < D.numel() and float(l_depth.detach()) > 0 and float(l_alpha.detach()) > 0
    if p.alpha_min > 0:
        assert n_used < N
    gD, gA = torch.autograd.grad(total, (D, A))
    cD, cA, s = ref.gradients(D.detach(), A.detach(), Z, p)
    assert int((s != 0).sum()) == n_used
    for have, want in ((cD, gD), (cA, gA)):
        assert float((have - want).abs().max()) <= 1e-12 * float(want.abs().max())
    # and the gradient is what a finite difference of the value sees
    i = (7, 9)
    eps = 1e-6
    for which, grad in ((0, gD), (1, gA)):
        args = [D.detach().clone(), A.detach().clone()]
        args[which][i] += eps
        up = ref.value(args[0], args[1], Z, p)[0]
        args[which][i] -= 2 * eps
        down = ref.value(args[0], args[1], Z, p)[0]
        assert abs(float((up - down) / (2 * eps)) - float(grad[i])) <= 1e-6 * abs(float(grad[i])) + 1e-12


def test_size_queries_answer_without_a_gpu():
    from segs_slam_amd import _capi
    _capi.build()
    lib = _capi.lib()
    prev_t = prev_b = 0
    for H, W in ((1, 1), (17, 33), (32, 32), (25, 41), (187, 333), (480, 640), (680, 1200), (1080, 1920)):
        t, b = lib.segs_depth_target_floats(H, W), lib.segs_depth_loss_temp_bytes(H, W)
        assert t > H * W and b > 0
        assert t >= prev_t and b >= prev_b
        prev_t, prev_b = t, b
    assert lib.segs_depth_target_floats(0, 5) == 0 and lib.segs_depth_loss_temp_bytes(5, 0) == 0


def test_parameter_validation_on_the_host():
    from segs_slam_amd.depth_loss import DepthLossParams, FusedDepthLoss
    DepthLossParams(1.0)
    DepthLossParams(1.0, 0.1, 0.99, True, 0.0, 40.0)
    with pytest.raises(ValueError):
        DepthLossParams(1.0, normalize=True)
    with pytest.raises(ValueError):
        DepthLossParams(1.0, alpha_min=-0.5, normalize=True)
    with pytest.raises(ValueError):
        DepthLossParams(1.0, min_depth=-1e-3)
    with pytest.raises(RuntimeError):                     # no CPU path
        FusedDepthLoss(8, 8, "cpu", DepthLossParams(1.0))


def test_mapper_step_takes_its_depth_range_from_the_configuration():
    """make_mapper_step(depth_loss_lambda=...) reads RGBD.min_depth / RGBD.max_depth; checked on the parameter object alone (the
    step itself needs a GPU)."""
    import inspect
    from segs_slam_amd import mapper_config as mc, neural_gaussians as ng
    assert inspect.signature(mc.make_mapper_step).parameters["depth_loss_lambda"].default is None
    assert inspect.signature(ng.ScaffoldTrainerStep.__init__).parameters["depth_loss"].default is None
    assert inspect.signature(ng.ScaffoldTrainerStep.training_once).parameters["gt_depths"].default is None
    assert inspect.signature(ng.ScaffoldTrainerStep.pose_gradient).parameters["gt_depth"].default is None
    cfg = mc.load_committed_config("cfg/gaussian_mapper/RGB-D/Replica/office0.yaml")
    assert float(cfg.raw["RGBD.min_depth"]) >= 0 and "RGBD.max_depth" in cfg.raw
