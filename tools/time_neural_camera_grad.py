#!/usr/bin/env python3
"""Cost of dL/dcamera_center in the neural backward: HIP-event times of segs_neural_backward and
segs_neural_backward_camera on the same forward state, in one process, alternating, at the anchor-level mapper step's size
(config 5: 300 k anchors x 10 offsets, 1200x680, appearance_dim 16, no feature bank) and for the feature-bank model.

The candidate-domain gradients are those of one real iteration (render, L1/SSIM, rasterizer backward); only the neural backward is
timed.  Per call: one event pair; after the warm-up the two forms alternate so that clock and cache state are shared.  Prints and
writes per-form median / p10 / p90 / min in microseconds and the ratio of the medians.

usage (GPU box): python tools/time_neural_camera_grad.py [--anchors 300000] [--steps 200] [--warmup 30] [--out FILE.json]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from segs_slam_amd import _capi, neural_gaussians as ng, scenes  # noqa: E402


def measure(dims, anchors, steps, warmup, flags=0):
    dev = torch.device("cuda:0")
    cam = scenes.make_config_camera("c5")
    model = ng.synthetic_model(anchors, dims, cam, dev, seed=0)
    step = ng.ScaffoldTrainerStep(model, cam.width, cam.height, scaling_reg_weight=0.01)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    kf = ng.Keyframe(t(cam.world_view_transform), t(cam.full_proj_transform), t(cam.camera_center),
                     torch.tensor([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0], device=dev), cam.tanfovx, cam.tanfovy)
    gt = torch.rand(3, cam.height, cam.width, device=dev)
    for _ in range(3):                      # calibrate the resident rasterizer, then the projecting forward
        image = step.render(kf)
        torch.cuda.synchronize()
        step.engine.check(raise_on_overflow=False)
    _, dL = step.loss_fn(image, gt)
    g = step.engine.backward(dL)
    args = (g["means3D"], g["colors"], g["opacity"], g["scales"], g["rotations"], step.scaling_reg_weight)
    visible = int((step.visible_radii[:model.A] > 0).sum())
    lib = _capi.lib()
    old = lib.segs_neural_set_flags(flags)
    times = {False: [], True: []}
    try:
        for i in range(warmup + steps):
            for cam_grad in ((False, True) if i % 2 == 0 else (True, False)):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                step.neural.backward(*args, camera_grad=cam_grad)
                b.record()
                b.synchronize()
                if i >= warmup:
                    times[cam_grad].append(a.elapsed_time(b) * 1e3)
            if i % 16 == 15:
                model.grads.zero_()         # (the gradients accumulate: keep them finite)
    finally:
        lib.segs_neural_set_flags(old)
    out = {"anchors": anchors, "visible_anchors": visible, "steps": steps, "warmup": warmup}
    for cam_grad, name in ((False, "plain_us"), (True, "camera_us")):
        v = np.asarray(times[cam_grad])
        out[name] = {"median": float(np.median(v)), "p10": float(np.percentile(v, 10)), "p90": float(np.percentile(v, 90)),
                     "min": float(v.min())}
    out["camera_over_plain_median"] = out["camera_us"]["median"] / out["plain_us"]["median"]
    out["dL_dcamera_center"] = step.neural.dL_dcamera_center.tolist()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--anchors", type=int, default=300_000)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--out", default=None)
    opt = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "what": "segs_neural_backward vs segs_neural_backward_camera, HIP events per call, "
           "alternating in one process; 1200x680"}
    shapes = (("c5_plain_pair", ng.ModelDims(appearance_dim=16, use_feat_bank=False), 0),
              ("bank_pair", ng.ModelDims(appearance_dim=32, use_feat_bank=True), 0),
              ("c5_plain_one_kernel", ng.ModelDims(appearance_dim=16, use_feat_bank=False), 1),
              ("bank_one_kernel", ng.ModelDims(appearance_dim=32, use_feat_bank=True), 1))
    for name, dims, flags in shapes:
        res[name] = measure(dims, opt.anchors, opt.steps, opt.warmup, flags)
        r = res[name]
        print(f"{name}: visible {r['visible_anchors']}  plain {r['plain_us']['median']:.1f} us (p10 {r['plain_us']['p10']:.1f}, p90 "
              f"{r['plain_us']['p90']:.1f})  camera {r['camera_us']['median']:.1f} us (p10 {r['camera_us']['p10']:.1f}, p90 "
              f"{r['camera_us']['p90']:.1f})  ratio {r['camera_over_plain_median']:.3f}", flush=True)
    if opt.out:
        with open(opt.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
