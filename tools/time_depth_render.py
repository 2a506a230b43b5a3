#!/usr/bin/env python3
"""Cost of the depth and alpha maps: the resident rasterizer's forward + backward (RasterEngine, the training path) with and without
render_depth, per workload, timed with HIP events; plus the two tile kernels alone (segs_profile_*).  Prints one JSON line.

usage (GPU box): python tools/time_depth_render.py [workload ...] [--steps N] [--warmup N]     (default: 1080p_3m c2)"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from segs_slam_amd import scenes  # noqa: E402
from segs_slam_amd.raster_engine import KernelProfile, RasterEngine  # noqa: E402

TILE_KERNELS = ("render_fwd_kernel", "render_bwd_kernel")   # profile labels: they cover the depth forms on the depth calls too


def time_engine(eng, a, cam, dL, dD, dA, steps, warmup):
    def step():
        eng.forward(*a, cam.tanfovx, cam.tanfovy)
        if dD is None:
            eng.backward(dL)
        else:
            eng.backward(dL, dD, dA)
    for _ in range(warmup):
        step()
    assert eng.check() and eng._last_resident
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        step()
    t1.record()
    torch.cuda.synchronize()
    assert eng.check()
    with KernelProfile(TILE_KERNELS) as kp:
        for _ in range(steps):
            step()
        torch.cuda.synchronize()
    tiles = {k: round(v["avg_ms"], 4) for k, v in kp.result.items()}
    return t0.elapsed_time(t1) / steps, tiles


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("workloads", nargs="*", default=["1080p_3m", "c2"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    opt = ap.parse_args()
    dev = "cuda:0"
    out = {"metric": "resident forward+backward ms per step, plain vs render_depth", "steps": opt.steps, "workloads": {}}
    for name in opt.workloads:
        sc = scenes.make_config_scene(name)
        cam = sc.camera
        t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
        a = [t(x) for x in (sc.bg, sc.means3D, sc.colors, sc.opacity, sc.scales, sc.rotations, cam.world_view_transform,
                            cam.full_proj_transform, cam.camera_center)]
        dL = t(sc.dL_dout_color)
        g = torch.Generator(device="cpu").manual_seed(1)
        dD = (torch.rand(cam.height, cam.width, generator=g) * 2 - 1).div(cam.height * cam.width).to(dev)
        dA = (torch.rand(cam.height, cam.width, generator=g) * 2 - 1).div(cam.height * cam.width).to(dev)
        res = {}
        for label, depth in (("plain", False), ("depth", True)):
            eng = RasterEngine(sc.P, cam.width, cam.height, dev, resident=True, render_depth=depth)
            ms, tiles = time_engine(eng, a, cam, dL, dD if depth else None, dA if depth else None, opt.steps, opt.warmup)
            res[label] = {"step_ms": round(ms, 4), "tile_kernels_ms": tiles,
                          "tile_total_ms": round(sum(tiles.values()), 4)}
            del eng
            torch.cuda.empty_cache()
        res["step_ratio"] = round(res["depth"]["step_ms"] / res["plain"]["step_ms"], 4)
        res["tile_ratio"] = round(res["depth"]["tile_total_ms"] / res["plain"]["tile_total_ms"], 4)
        out["workloads"][name] = res
        del a, dL, dD, dA, sc
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
