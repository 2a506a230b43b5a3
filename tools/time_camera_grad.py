#!/usr/bin/env python3
"""Cost of the camera gradient: the resident rasterizer's backward (RasterEngine, the training path) with and without the
segs_camera_grads struct, per workload, timed with HIP events; plus the K_PREPROCESS_BWD profile slot alone (segs_profile_*), which
covers the per-Gaussian backward and, in the camera form, the kernel that sums its partial rows.  Prints one JSON line.

usage (GPU box): python tools/time_camera_grad.py [workload ...] [--steps N] [--warmup N]     (default: 1080p_3m c1)"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from segs_slam_amd import scenes  # noqa: E402
from segs_slam_amd.raster_engine import KernelProfile, RasterEngine  # noqa: E402

SLOT = ("preprocess_bwd_kernel",)


def time_backward(eng, a, cam, dL, camera, steps, warmup):
    def step(events=None):
        eng.forward(*a, cam.tanfovx, cam.tanfovy)
        if events is not None:
            events[0].record()
        eng.backward(dL, camera_grad=camera)
        if events is not None:
            events[1].record()
    for _ in range(warmup):
        step()
    assert eng.check() and eng._last_resident
    torch.cuda.synchronize()
    pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for ev in pairs:
        step(ev)
    torch.cuda.synchronize()
    assert eng.check()
    ms = sorted(e0.elapsed_time(e1) for e0, e1 in pairs)
    with KernelProfile(SLOT) as kp:
        for _ in range(steps):
            step()
        torch.cuda.synchronize()
    return ms[len(ms) // 2], kp.result[SLOT[0]]["avg_ms"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("workloads", nargs="*", default=["1080p_3m", "c1"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    opt = ap.parse_args()
    dev = "cuda:0"
    out = {"metric": "resident backward ms (median) and its preprocess_bwd_kernel profile slot, plain vs camera_grad",
           "steps": opt.steps, "workloads": {}}
    for name in opt.workloads:
        sc = scenes.make_config_scene(name)
        cam = sc.camera
        t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
        a = [t(x) for x in (sc.bg, sc.means3D, sc.colors, sc.opacity, sc.scales, sc.rotations, cam.world_view_transform,
                            cam.full_proj_transform, cam.camera_center)]
        dL = t(sc.dL_dout_color)
        eng = RasterEngine(sc.P, cam.width, cam.height, dev, resident=True, camera_grad=True)   # one set of buffers for both forms
        res = {}
        for label, camera in (("plain", False), ("camera", True), ("plain_again", False)):
            ms, slot = time_backward(eng, a, cam, dL, camera, opt.steps, opt.warmup)
            res[label] = {"backward_ms": round(ms, 4), "preprocess_bwd_slot_ms": round(slot, 4)}
        res["backward_ratio"] = round(res["camera"]["backward_ms"] / res["plain"]["backward_ms"], 4)
        res["slot_ratio"] = round(res["camera"]["preprocess_bwd_slot_ms"] / res["plain"]["preprocess_bwd_slot_ms"], 4)
        res["partial_rows"] = (sc.P + 255) // 256
        out["workloads"][name] = res
        del eng, a, dL, sc
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
