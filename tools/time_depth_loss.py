#!/usr/bin/env python3
"""Cost of depth supervision, measured on the GPU in ONE process:

 * the Replica-size mapper step (bench.py's `replica_step` block: cfg values of RGB-D/Replica/office0.yaml, 50 k anchors x 10
   offsets, 1200x680, frequency regulariser on, statistics every iteration) with and without depth supervision, timed in
   alternating blocks with one HIP-event pair per step: p10 / p50 / p90 of the per-step device time;
 * segs_depth_target and segs_depth_loss alone at 1200x680 and 640x480 (HIP events around batches of calls), next to the fused
   L1 + SSIM loss call at the same size.

usage (GPU box): python tools/time_depth_loss.py [--anchors 50000] [--steps 200] [--out profiles/depth_supervision_step.txt]"""
import argparse
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from segs_slam_amd import mapper_config as mc, neural_gaussians as ng, scenes  # noqa: E402
from segs_slam_amd.depth_loss import DepthLossParams, FusedDepthLoss  # noqa: E402
from segs_slam_amd.gaussian_trainer import FusedL1SSIM  # noqa: E402


def percentiles(ms):
    p10, p50, p90 = np.percentile(np.asarray(ms), [10, 50, 90])
    return f"p10 {p10:.3f}  p50 {p50:.3f}  p90 {p90:.3f} ms  (n = {len(ms)})"


def timed_block(step, kf, gt, depths, n):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(n + 1)]
    ev[0].record()
    for i in range(n):
        step.training_once([kf], [gt], depths)
        ev[i + 1].record()
    torch.cuda.synchronize()
    return [ev[i].elapsed_time(ev[i + 1]) for i in range(n)]


def replica_steps(dev, anchors, steps, warmup, block, lam):
    cfg = mc.load_committed_config("cfg/gaussian_mapper/RGB-D/Replica/office0.yaml")
    cam = scenes.make_config_camera("c2")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    kf = ng.Keyframe(t(cam.world_view_transform), t(cam.full_proj_transform), t(cam.camera_center),
                     torch.tensor([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0], device=dev), cam.tanfovx, cam.tanfovy)
    g = torch.Generator(device=dev).manual_seed(0)
    gt = torch.rand(3, cam.height, cam.width, device=dev, generator=g)
    z = 1.0 + 5.0 * torch.rand(cam.height, cam.width, device=dev, generator=g)        # the synthetic map's depth range
    z[torch.rand(cam.height, cam.width, device=dev, generator=g) < 0.1] = 0.0          # 10 % holes, as a sensor has
    runs = {}
    for label, with_depth in (("colour only", False), ("with depth", True)):
        model = ng.synthetic_model(anchors, cfg.model, cam, dev, seed=0)
        step = mc.make_mapper_step(cfg, model, cam.width, cam.height, depth_loss_lambda=lam if with_depth else None)
        step.keyframe_for = lambda s, n: 0
        step.iteration = 10_000                       # inside the frequency regulariser's window
        step.densifier.p.update_from = 10 ** 9        # statistics every iteration, no adjust_anchor inside the window
        depths = [step._depth_fn().prepare(z)] if with_depth else None
        for _ in range(warmup):
            step.training_once([kf], [gt], depths)
        torch.cuda.synchronize()
        runs[label] = (step, depths, [])
    for _ in range(max(1, steps // block)):           # alternate, so that both see the same machine
        for label, (step, depths, ms) in runs.items():
            ms += timed_block(step, kf, gt, depths, block)
    lines = [f"Replica-size mapper step, {anchors} anchors x 10 offsets, {cam.width}x{cam.height}, lambda_depth {lam}, "
             f"{warmup} warm-up iterations each, alternating blocks of {block} steps, per-step HIP events:"]
    for label, (step, depths, ms) in runs.items():
        step.finish()
        lines.append(f"  {label:12s} {percentiles(ms)}   dropped {step.dropped_steps()} redone {step.redone_steps}"
                     + (f"   depth_terms {[round(float(x), 5) for x in step.depth_terms]}" if step.depth_terms is not None else ""))
    a, b = np.median(runs["colour only"][2]), np.median(runs["with depth"][2])
    lines.append(f"  p50 ratio with / without: {b / a:.3f}")
    return lines


def event_time_us(fn, calls=200, rounds=5):
    for _ in range(20):
        fn()
    out = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / calls * 1e3)
    return min(out), float(np.median(out))


def kernels_alone(dev):
    lines = ["Kernels alone (HIP events around 200 back-to-back calls, best / median of 5 rounds, us per call; back-to-back calls",
             "include the launch gaps of a one- or two-kernel call):"]
    for W, H in ((1200, 680), (640, 480)):
        g = torch.Generator(device=dev).manual_seed(1)
        A = torch.rand(H, W, device=dev, generator=g)
        D = A * (1.0 + 5.0 * torch.rand(H, W, device=dev, generator=g))
        Z = 1.0 + 5.0 * torch.rand(H, W, device=dev, generator=g)
        img, gt = torch.rand(3, H, W, device=dev, generator=g), torch.rand(3, H, W, device=dev, generator=g)
        ssim = FusedL1SSIM(H, W, dev, 0.2)
        best, med = event_time_us(lambda: ssim(img, gt))
        lines.append(f"  {W}x{H}: fused L1 + SSIM loss call (2 kernels, ~180 B/pixel)   best {best:.1f}  median {med:.1f}")
        for label, p in (("plain", DepthLossParams(1.0, 0.1)), ("normalize + silhouette", DepthLossParams(1.0, 0.1, 0.99, True))):
            fn = FusedDepthLoss(H, W, dev, p)
            tgt = fn.prepare(Z)
            best, med = event_time_us(lambda: fn(D, A, tgt))
            lines.append(f"  {W}x{H}: segs_depth_loss ({label}; 2 launches, 24 B/pixel = {24 * W * H / 1e6:.1f} MB)   best {best:.1f}  median {med:.1f}"
                         f"   -> {24 * W * H / best / 1e6:.2f} TB/s at best")
        fn = FusedDepthLoss(H, W, dev, DepthLossParams(1.0, min_depth=0.01, max_depth=40.0))
        blk = fn.prepare(Z).block
        call = lambda: fn._lib.segs_depth_target(C.c_void_p(Z.data_ptr()), H, W, 0.01, 40.0, C.c_void_p(blk.data_ptr()), fn._stream())  # noqa: E731
        best, med = event_time_us(call)
        lines.append(f"  {W}x{H}: segs_depth_target (memset + 1 kernel, 8 B/pixel)   best {best:.1f}  median {med:.1f}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--anchors", type=int, default=50_000)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=60)
    ap.add_argument("--block", type=int, default=25)
    ap.add_argument("--lambda-depth", type=float, default=0.5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    lines = [f"# tools/time_depth_loss.py on {torch.cuda.get_device_name(0)}"]
    lines += kernels_alone(dev)
    lines += replica_steps(dev, a.anchors, a.steps, a.warmup, a.block, a.lambda_depth)
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
