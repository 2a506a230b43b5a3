"""The pose chain of segs_slam_amd/pose_refine.py on the CPU: view = V0 @ D(xi), proj = view @ Pm, campos = inv(view)[3, :3]."""
import numpy as np
import torch


def _keyframe(seed=0):
    from segs_slam_amd import neural_gaussians as ng
    rng = np.random.default_rng(seed)
    q = rng.standard_normal(4)
    t = rng.standard_normal(3) * 0.5
    return ng.Keyframe.from_pose(q, t, 640, 480, 525.0, 520.0, "cpu")


def test_zero_xi_returns_the_keyframe():
    from segs_slam_amd.pose_refine import KeyframePose
    kf = _keyframe()
    out = KeyframePose(kf, 1e-3).keyframe()
    # float32 rounding of entries up to |proj| ~ 2.5 and of the inverse's products: a few ulp of the largest entry
    for name in ("view", "proj", "campos"):
        a, b = getattr(out, name), getattr(kf, name)
        assert a.dtype == torch.float32 and a.is_contiguous() and not a.requires_grad and a.shape == b.shape
        assert float((a - b).abs().max()) <= 4 * 2.0 ** -23 * max(1.0, float(b.abs().max())), name
    assert out.pose7 is kf.pose7 and out.tanfovx == kf.tanfovx and out.tanfovy == kf.tanfovy


def test_accumulate_equals_float64_autograd_of_the_chain():
    from segs_slam_amd.pose_refine import KeyframePose, pose_chain
    kf = _keyframe(1)
    pose = KeyframePose(kf, 1e-3)
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        pose.xi.copy_(torch.tensor([0.02, -0.03, 0.015, 0.01, -0.02, 0.03], dtype=torch.float64))
    grads = {"viewmatrix": torch.randn(4, 4, generator=g), "projmatrix": torch.randn(4, 4, generator=g),
             "camera_center": torch.randn(3, generator=g)}
    pose.accumulate(grads)
    x = pose.xi.detach().clone().requires_grad_(True)
    V0 = kf.view.double()
    view, proj, campos = pose_chain(x, V0, torch.linalg.inv(V0) @ kf.proj.double())
    ((view * grads["viewmatrix"].double()).sum() + (proj * grads["projmatrix"].double()).sum()
     + (campos * grads["camera_center"].double()).sum()).backward()
    assert float(x.grad.abs().min()) > 0
    assert torch.allclose(pose.xi.grad, x.grad, rtol=1e-12, atol=0)
    pose.accumulate(grads)                              # a second view of the same keyframe adds up
    assert torch.allclose(pose.xi.grad, 2 * x.grad, rtol=1e-12, atol=0)
    # and the chain's own derivative is right: central differences of the same scalar
    def scalar(v):
        a, b, c = pose_chain(v, V0, torch.linalg.inv(V0) @ kf.proj.double())
        return float((a * grads["viewmatrix"].double()).sum() + (b * grads["projmatrix"].double()).sum() + (c * grads["camera_center"].double()).sum())
    for j in range(6):
        e = torch.zeros(6, dtype=torch.float64)
        e[j] = 1e-6
        fd = (scalar(x.detach() + e) - scalar(x.detach() - e)) / 2e-6
        assert abs(fd - float(x.grad[j])) <= 1e-6 * max(1.0, abs(float(x.grad[j]))), j


def test_campos_is_minus_rt_t_of_the_moved_pose():
    from segs_slam_amd.pose_refine import KeyframePose
    kf = _keyframe(2)
    pose = KeyframePose(kf, 1e-3)
    with torch.no_grad():
        pose.xi.copy_(torch.tensor([0.3, -0.2, 0.1, 0.4, -0.5, 0.6], dtype=torch.float64))
    out = pose.keyframe()
    V = out.view.double()                 # transposed layout: V = [[R^T, 0], [t, 1]] maps world rows to camera rows
    Rt, t = V[:3, :3], V[3, :3]           # x_cam = x_world @ R^T + t  ->  centre = -t @ R
    centre = -(t @ Rt.T)
    assert torch.allclose(out.campos.double(), centre, atol=1e-6)
    assert torch.allclose(Rt @ Rt.T, torch.eye(3, dtype=torch.float64), atol=1e-6)      # still a rotation
    assert float((out.view - kf.view).abs().max()) > 0.1                                # and it moved
    assert torch.allclose(out.proj.double(), V @ pose.Pm, atol=1e-5)


def test_refiner_moves_only_the_poses_that_received_a_gradient():
    from segs_slam_amd.pose_refine import PoseRefiner
    ref = PoseRefiner(lr=1e-2)
    for k in (3, 7, 9):
        ref.add(k, _keyframe(k))
    g = torch.Generator().manual_seed(1)
    grads = {"viewmatrix": torch.randn(4, 4, generator=g), "projmatrix": torch.randn(4, 4, generator=g),
             "camera_center": torch.randn(3, generator=g)}
    ref.accumulate(7, grads)
    ref.step()
    assert float(ref[7].xi.detach().abs().min()) > 0
    assert float(ref[3].xi.detach().abs().max()) == 0 and float(ref[9].xi.detach().abs().max()) == 0
    assert all(ref[k].xi.grad is None for k in (3, 7, 9))
    before = ref[7].xi.detach().clone()
    ref.accumulate(3, grads)
    ref.step()
    assert torch.equal(ref[7].xi.detach(), before) and float(ref[3].xi.detach().abs().min()) > 0
    # Adam's first step is lr * sign(gradient)
    assert torch.allclose(before.abs(), torch.full((6,), 1e-2, dtype=torch.float64), rtol=1e-6)
    kf = ref.keyframe(7)
    assert kf.view.dtype == torch.float32 and float((kf.view - ref[7].base.view).abs().max()) > 0
