"""Pose chain of the Scaffold step's camera gradients (off the hot path, plain torch).

ScaffoldTrainerStep(pose_grad=True) leaves three device gradients per iteration: dL/dviewmatrix, dL/dprojmatrix (the rasterizer,
DESIGN.md 3e) and dL/dcamera_center (the neural-Gaussian generator, segs_neural_backward_camera).  A keyframe's pose enters the
step only through those three tensors, so a 6-dof update needs nothing but the chain rule through the small graph

    view = V0 @ D(xi),    proj = view @ Pm,    campos = inv(view)[3, :3]

where xi = (axis-angle, translation) moves the camera frame, D(xi) = [[R^T, 0], [t, 1]] with R = exp(skew(xi[:3])) in the
transposed layout the rasterizer takes, and Pm = inv(V0) @ proj0 is the keyframe's projection matrix.  pose7, which only the
appearance embedding reads, stays what the keyframe had: the reference builds it from host floats (src/gaussian_renderer.cpp:258-264)
and no gradient reaches the pose through it.
"""
from __future__ import annotations

from typing import Dict, Iterable, Optional

import torch

from .neural_gaussians import Keyframe


def delta(xi: torch.Tensor) -> torch.Tensor:
    """(4, 4) transposed-layout motion of the camera frame: [[R^T, 0], [t, 1]], R = exp(skew(xi[:3])) (Rodrigues, safe at 0)."""
    w, t = xi[:3], xi[3:]
    th2 = (w * w).sum()
    th = torch.sqrt(th2 + 1e-20)
    z = torch.zeros((), dtype=xi.dtype, device=xi.device)
    K = torch.stack([torch.stack([z, -w[2], w[1]]), torch.stack([w[2], z, -w[0]]), torch.stack([-w[1], w[0], z])])
    R = torch.eye(3, dtype=xi.dtype, device=xi.device) + (torch.sin(th) / th) * K + ((1 - torch.cos(th)) / (th2 + 1e-20)) * (K @ K)
    D = torch.nn.functional.pad(R.T, (0, 1, 0, 1)) + torch.nn.functional.pad(t[None, :], (0, 1, 3, 0))
    corner = torch.zeros((4, 4), dtype=xi.dtype, device=xi.device)
    corner[3, 3] = 1
    return D + corner


def pose_chain(xi: torch.Tensor, V0: torch.Tensor, Pm: torch.Tensor):
    """(view, proj, campos) of the pose V0 moved by xi; differentiable, any dtype."""
    view = V0 @ delta(xi)
    return view, view @ Pm, torch.linalg.inv(view)[3, :3]


class KeyframePose:
    """A keyframe whose pose is V0 @ D(xi) with a trainable 6-dof xi (float64, on the keyframe's device, zero at the start)."""

    def __init__(self, kf: Keyframe, lr: float = 1e-4):
        self.base = kf
        self.lr = float(lr)
        dev = kf.view.device
        self.V0 = kf.view.detach().to(torch.float64)
        self.Pm = torch.linalg.inv(self.V0) @ kf.proj.detach().to(torch.float64)     # recovered once
        self.xi = torch.zeros(6, dtype=torch.float64, device=dev, requires_grad=True)

    def matrices(self):
        """(view, proj, campos) in float64, attached to xi."""
        return pose_chain(self.xi, self.V0, self.Pm)

    def keyframe(self) -> Keyframe:
        """The keyframe at the current xi: detached contiguous float32 view / proj / campos; pose7 and the tangents unchanged."""
        with torch.no_grad():
            view, proj, campos = self.matrices()
        f = lambda x: x.to(torch.float32).contiguous()  # noqa: E731
        return Keyframe(f(view), f(proj), f(campos), self.base.pose7, self.base.tanfovx, self.base.tanfovy)

    def accumulate(self, pose_grads: Dict[str, torch.Tensor]) -> None:
        """xi.grad += the three gradients of ScaffoldTrainerStep.pose_grads pushed through the chain at the current xi.  The
        gradients are read when this is called: call it before the step's next iteration overwrites them."""
        view, proj, campos = self.matrices()
        g = lambda k: pose_grads[k].detach().to(view.device, torch.float64)  # noqa: E731
        scalar = (view * g("viewmatrix")).sum() + (proj * g("projmatrix")).sum() + (campos * g("camera_center")).sum()
        (grad,) = torch.autograd.grad(scalar, self.xi)
        self.xi.grad = grad if self.xi.grad is None else self.xi.grad + grad


class PoseRefiner:
    """Keyframe poses by id and one Adam over their xi.  step() moves the poses that received a gradient since the last step
    (a pose whose xi.grad is None is skipped by torch's Adam: neither it nor its moments change)."""

    def __init__(self, lr: float = 1e-4):
        self.lr = float(lr)
        self.poses: Dict[object, KeyframePose] = {}
        self.adam: Optional[torch.optim.Adam] = None

    def add(self, key, kf: Keyframe, lr: Optional[float] = None) -> KeyframePose:
        pose = self.poses[key] = KeyframePose(kf, self.lr if lr is None else lr)
        group = {"params": [pose.xi], "lr": pose.lr}
        if self.adam is None:
            self.adam = torch.optim.Adam([group])
        else:
            self.adam.add_param_group(group)
        return pose

    def __getitem__(self, key) -> KeyframePose:
        return self.poses[key]

    def keyframe(self, key) -> Keyframe:
        return self.poses[key].keyframe()

    def accumulate(self, key, pose_grads: Dict[str, torch.Tensor]) -> None:
        self.poses[key].accumulate(pose_grads)

    def step(self, keys: Optional[Iterable] = None) -> None:
        """One Adam step, then the gradients are dropped (set to None).  keys: only these poses keep their gradient for the step."""
        if self.adam is None:
            return
        if keys is not None:
            keep = set(keys)
            for k, p in self.poses.items():
                if k not in keep:
                    p.xi.grad = None
        self.adam.step()
        self.adam.zero_grad(set_to_none=True)
