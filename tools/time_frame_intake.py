#!/usr/bin/env python3
"""Cost of one frame's intake, measured on the GPU: FrameIntake.rgb with 2 sub-levels and FrameIntake.depth at 640x480
(TUM freiburg2's camera) and 1200x680 (Replica room0's).

 * each call: one HIP event pair per call, after warm-up calls of the same shape, all shapes in one process;
 * next to each figure, for comparison only, the same work as torch ops on the same device: the uint8 -> float conversion and the
   permute, grid_sample on a grid computed beforehand (8 bytes per pixel, read on every call), interpolate per level; for the depth
   the conversion, the scale and grid_sample (the plain remap: torch has no hole-aware form);
 * the bytes the design moves (`design_bytes`, from the shapes) and the time they take at the HBM rate measured for this chip
   (6.29 TB/s, float4 copy) -- the floor of a memory-bound design, not a prediction.

usage (GPU box): python tools/time_frame_intake.py [--out profiles/frame_intake_time.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

HBM_BYTES_PER_S = 6.29e12
SUB_LEVELS = 2
CAMERAS = (("TUM freiburg2", "cfg/ORB_SLAM3/RGB-D/TUM/tum_freiburg2_xyz.yaml"), ("Replica room0", "cfg/ORB_SLAM3/RGB-D/Replica/room0.yaml"))


def design_bytes(in_w, in_h, out_w, out_h, sizes):
    """Bytes each call has to move once (taps that a cache serves again are not counted)."""
    n_in, n_out = in_w * in_h, out_w * out_h
    levels = sum(w * h for w, h in sizes)
    rgb = {"undistort_in": 3 * n_in, "undistort_out": 12 * n_out + n_out, "levels_in": 12 * n_out, "levels_out": 12 * levels}
    rgb["total"] = sum(rgb.values())
    depth = {"in": 2 * n_in, "out": 4 * n_out}
    depth["total"] = sum(depth.values())
    return {"rgb": rgb, "depth": depth}


def pct(ms):
    p10, p50, p90 = np.percentile(np.asarray(ms, dtype=np.float64), [10, 50, 90])
    return {"p10": float(p10), "p50": float(p50), "p90": float(p90), "n": len(ms)}


def timed(fn, calls, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(calls + 1)]
    ev[0].record()
    for i in range(calls):
        fn()
        ev[i + 1].record()
    torch.cuda.synchronize()
    return pct([ev[i].elapsed_time(ev[i + 1]) for i in range(calls)])


def run(calls, warmup):
    import torch
    import torch.nn.functional as Fn
    from segs_slam_amd.frame_intake import CameraModel, FrameIntake
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    with open(os.path.join(ROOT, "tests", "golden", "orbslam_camera_values.json")) as f:
        table = json.load(f)
    runs = []
    for label, key in CAMERAS:
        cam = CameraModel.from_settings(table[key])
        it = FrameIntake(cam, dev, num_sub_levels=SUB_LEVELS)
        W, H = cam.width, cam.height
        g = torch.Generator().manual_seed(W)
        frame = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, generator=g).to(dev)
        raw = torch.randint(300, 30000, (H, W), dtype=torch.int16, generator=g).to(dev)
        r = {"camera": label, "source": [W, H], "output": [it.W, it.H], "sub_levels": [list(s) for s in it.sizes]}
        r["rgb_ms_hip_events"] = timed(lambda: it.rgb(frame, want_gray=True), calls, warmup)
        r["depth_ms_hip_events"] = timed(lambda: it.depth(raw), calls, warmup)

        # the same work as torch ops: the grid is made once, outside the timed calls
        m = it.debug_map()
        grid = torch.stack([2 * m[..., 0] / max(W - 1, 1) - 1, 2 * m[..., 1] / max(H - 1, 1) - 1], dim=-1)[None].contiguous()
        sizes = [(h, w) for w, h in it.sizes]

        def torch_rgb():
            src = frame.permute(2, 0, 1).float().div_(255.0)[None]
            img = Fn.grid_sample(src, grid, mode="bilinear", padding_mode="zeros", align_corners=True)
            return img, [Fn.interpolate(img, size=s, mode="bilinear", align_corners=False) for s in sizes]

        def torch_depth():
            src = raw.float().mul_(cam.inv_depth_factor)[None, None]
            return Fn.grid_sample(src, grid, mode="bilinear", padding_mode="zeros", align_corners=True)

        r["torch_ops_rgb_ms_hip_events"] = timed(torch_rgb, calls, warmup)
        r["torch_ops_depth_ms_hip_events"] = timed(torch_depth, calls, warmup)
        r["torch_ops_grid_bytes"] = int(grid.numel() * 4)
        img, _ = torch_rgb()
        r["max_abs_difference_from_torch_ops_image"] = float((img[0] - it.rgb(frame).image).abs().max().item())
        b = design_bytes(W, H, it.W, it.H, it.sizes)
        r["design_bytes"] = b
        r["design_bytes_over_hbm_rate_ms"] = {k: v["total"] / HBM_BYTES_PER_S * 1e3 for k, v in b.items()}
        runs.append(r)
        print(json.dumps(r), flush=True)
    return runs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    res = {"tool": "tools/time_frame_intake.py", "device": torch.cuda.get_device_name(0) if torch.cuda.is_available() else None,
           "method": "one HIP event pair per call after warm-up calls of the same shape, one process; rgb() = undistortion with grey + "
                     "2 sub-levels (2 launches), depth() = hole-aware (1 launch); torch ops on the same device for comparison only",
           "hbm_bytes_per_s": HBM_BYTES_PER_S, "runs": run(a.calls, a.warmup)}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
