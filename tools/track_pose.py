#!/usr/bin/env python3
"""Synthetic pose recovery through the camera gradient: render a seeded scene (colour + depth) at a pose, perturb the pose, and let
Adam move a 6-dof pose (axis-angle + translation of the camera frame) back by an L1 colour + depth loss through
GaussianRasterizer.forward_with_camera_grad.  Prints the pose error per iteration.

The scenes are seeded random Gaussians of a few pixels each, unrelated in colour and depth to their neighbours, so the image only
pulls the pose back from close by; the defaults keep 5000 Gaussians, enlarge them (--scale-mult) and start 0.2 degrees and 4 mm
off, from where the pose comes back to 0.01 degrees and 0.01 mm (profiles/track_pose_c1.txt).  From 0.5 degrees and 1 cm the
starting loss is a hundred times larger and Adam walks away: that start is outside the basin of this scene.

--scaffold tracks against an anchor map instead (neural_gaussians.synthetic_model): the Gaussians are then MLP outputs of the
view direction, so the pose gradient has a third part, dL/dcamera_center of the generator.  The target is the
map's own render at the true pose: its image (L1/SSIM) and its depth map as the sensor depth (the fused depth loss of DESIGN.md
3g, weight --lambda-depth; --silhouette counts only pixels the current render covers to 0.99).  ScaffoldTrainerStep.pose_gradient
gives the three device gradients and pose_refine.PoseRefiner takes them to the 6-dof pose.  Same columns; the depth column is
L_depth of the step's depth_terms.

usage (GPU box): python tools/track_pose.py [--workload c1] [--gaussians 5000] [--iters 200] [--rot-deg 0.2] [--shift 0.004]
                                            [--scale-mult 6] [--lr 1e-4]
                                            [--scaffold [--anchors 4000] [--lambda-depth 1.0] [--silhouette]]"""
import argparse
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from segs_slam_amd import scenes  # noqa: E402
from segs_slam_amd.gaussian_rasterizer import GaussianRasterizationSettings, GaussianRasterizer  # noqa: E402


def delta(xi):
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


def pose_errors(V_true, V):
    E = (torch.linalg.inv(V_true.double()) @ V.double()).cpu().numpy()     # the residual camera motion, transposed layout
    ang = math.degrees(math.acos(max(-1.0, min(1.0, (np.trace(E[:3, :3]) - 1) / 2))))
    return ang, float(np.linalg.norm(E[3, :3]))


def start_offset(opt):
    axis = np.array([0.3, -0.8, 0.5]) / np.linalg.norm([0.3, -0.8, 0.5])
    return np.concatenate([axis * math.radians(opt.rot_deg), np.array([1.0, -0.5, 0.7]) / np.linalg.norm([1.0, -0.5, 0.7]) * opt.shift])


def main_scaffold(opt):
    from segs_slam_amd import neural_gaussians as ng
    from segs_slam_amd.depth_loss import DepthLossParams
    from segs_slam_amd.pose_refine import PoseRefiner
    dev = "cuda:0"
    cam = scenes.make_config_camera(opt.workload)
    model = ng.synthetic_model(opt.anchors, ng.ModelDims(appearance_dim=16, use_feat_bank=False), cam, dev, seed=0)
    depth_loss = DepthLossParams(opt.lambda_depth, alpha_min=0.99 if opt.silhouette else 0.0)
    step = ng.ScaffoldTrainerStep(model, cam.width, cam.height, pose_grad=True, depth_loss=depth_loss)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    V_true, Pm = t(cam.world_view_transform), t(cam.projection_matrix)
    pose7 = torch.tensor([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0], device=dev)

    def keyframe(V):
        return ng.Keyframe(V.contiguous(), (V @ Pm).contiguous(), torch.linalg.inv(V)[3, :3].contiguous(), pose7, cam.tanfovx, cam.tanfovy)

    gt = step.render(keyframe(V_true)).clone()
    gt_depth = step._depth_fn().prepare(step.engine.out_depth)       # pixels no Gaussian reaches (depth 0) are invalid
    V_start = V_true @ delta(torch.tensor(start_offset(opt), dtype=torch.float32, device=dev))
    refiner = PoseRefiner(lr=opt.lr)
    pose = refiner.add(0, keyframe(V_start))
    print(f"# track_pose --scaffold: {opt.workload} A={model.A} x 10 offsets {cam.width}x{cam.height}, start off by {opt.rot_deg} deg / "
          f"{opt.shift} m, Adam lr {opt.lr}, lambda_depth {opt.lambda_depth}{', silhouette 0.99' if opt.silhouette else ''}")
    print("# iter  loss  colour_l1  depth_l1  rotation_error_deg  translation_error_m")
    for it in range(opt.iters + 1):
        kf = refiner.keyframe(0)
        loss = step.pose_gradient(kf, gt, gt_depth)
        l_col = (step.engine.out_color - gt).abs().mean()
        ang, sh = pose_errors(V_true, kf.view)
        print(f"{it:4d}  {float(loss):.6f}  {float(l_col):.6f}  {float(step.depth_terms[1]):.6f}  {ang:.4f}  {sh:.5f}")
        if it == opt.iters:
            break
        pose.accumulate(step.pose_grads)
        refiner.step()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c1")
    ap.add_argument("--gaussians", type=int, default=5000, help="Gaussians of the workload's scene that are kept")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rot-deg", type=float, default=0.2)
    ap.add_argument("--shift", type=float, default=0.004)
    ap.add_argument("--scale-mult", type=float, default=6.0)
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--scaffold", action="store_true", help="track against an anchor map (neural Gaussians) through pose_gradient")
    ap.add_argument("--anchors", type=int, default=4000, help="--scaffold: anchors of the synthetic map")
    ap.add_argument("--lambda-depth", type=float, default=1.0, help="--scaffold: weight of the depth term")
    ap.add_argument("--silhouette", action="store_true", help="--scaffold: depth term only where the render's opacity is >= 0.99")
    opt = ap.parse_args()
    if opt.scaffold:
        return main_scaffold(opt)
    dev = "cuda:0"
    sc = scenes.make_config_scene(opt.workload, P=opt.gaussians)
    sc.scales *= opt.scale_mult
    cam = sc.camera
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    m3, col, op, sca, rot = (t(x) for x in (sc.means3D, sc.colors, sc.opacity, sc.scales, sc.rotations))
    V_true, Pm = t(cam.world_view_transform), t(cam.projection_matrix)
    rs = GaussianRasterizationSettings(cam.height, cam.width, cam.tanfovx, cam.tanfovy, t(sc.bg), 1.0, V_true, V_true @ Pm, 0,
                                       t(cam.camera_center), False)
    rast = GaussianRasterizer(rs)

    def render(V):
        return rast.forward_with_camera_grad(m3, torch.zeros_like(m3), op, True, True, False, col, scales=sca, rotations=rot,
                                             viewmatrix=V, projmatrix=V @ Pm)

    with torch.no_grad():
        img_gt, _, depth_gt, _ = render(V_true)
    # the starting pose: the true one moved by a fixed rotation and shift; the optimised xi acts on top of it
    off = start_offset(opt)
    V_start = V_true @ delta(torch.tensor(off, dtype=torch.float32, device=dev))
    xi = torch.zeros(6, device=dev, requires_grad=True)
    adam = torch.optim.Adam([xi], lr=opt.lr)
    print(f"# track_pose: {opt.workload} P={sc.P} {cam.width}x{cam.height}, scales x{opt.scale_mult}, start off by {opt.rot_deg} deg / "
          f"{opt.shift} m, Adam lr {opt.lr}")
    print("# iter  loss  colour_l1  depth_l1  rotation_error_deg  translation_error_m")

    def errors(V):
        return pose_errors(V_true, V)

    for it in range(opt.iters + 1):
        V = V_start @ delta(xi)
        img, _, depth, _ = render(V)
        l_col, l_dep = (img - img_gt).abs().mean(), (depth - depth_gt).abs().mean()
        loss = l_col + l_dep
        ang, sh = errors(V.detach())
        print(f"{it:4d}  {float(loss.detach()):.6f}  {float(l_col.detach()):.6f}  {float(l_dep.detach()):.6f}  {ang:.4f}  {sh:.5f}")
        if it == opt.iters:
            break
        adam.zero_grad()
        loss.backward()
        adam.step()


if __name__ == "__main__":
    main()
