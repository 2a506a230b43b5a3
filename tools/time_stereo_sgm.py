#!/usr/bin/env python3
"""Cost of one stereo depth frame, measured on the GPU: StereoSGM.compute_depth on a synthetic rectified pair at
752x480 (EuRoC) and 1241x376 (KITTI), 128 disparities, 4 and 8 paths.

 * the whole call: one HIP event pair per call, after warm-up calls of the same shape, all shapes in one process;
 * per kernel (--kernel-stats): the same calls run once more in a child process of their own under
   `rocprofv3 --kernel-trace --stats`, whose per-kernel table is read back (tracing slows the host, so the whole-call
   figures never come from that run);
 * next to both, the bytes the design moves (computed from the shapes by `design_bytes` below) and the time those bytes take
   at the HBM rate measured for this chip (6.29 TB/s, float4 copy) -- the floor of a memory-bound design, not a prediction.

usage (GPU box): python tools/time_stereo_sgm.py [--kernel-stats] [--out profiles/stereo_sgm_time.json]"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

HBM_BYTES_PER_S = 6.29e12
KERNELS = ("sgm_path_kernel", "census_kernel", "winner_kernel", "right_view_kernel", "median_kernel", "check_output_kernel",
           "rgb_to_gray_kernel")
SHAPES = (("EuRoC", 752, 480, 435.2, 0.11), ("KITTI", 1241, 376, 718.9, 0.54))
D = 128


def design_bytes(W, H, D, paths, median=True):
    """Bytes each launch has to move once (re-reads that a cache serves are not counted): n = W H pixels."""
    n = W * H
    per_path_first = 8 * n + 2 * n * D                 # both census maps in, S out
    per_path_next = 8 * n + 4 * n * D                  # ... S in and out
    b = {"census_kernel": 2 * n + 8 * n,
         "sgm_path_kernel": per_path_first + (paths - 1) * per_path_next,
         "winner_kernel": 2 * n * D + 2 * n,
         "right_view_kernel": 2 * n * D + 2 * n,
         "median_kernel": 4 * n if median else 0,
         "check_output_kernel": 2 * n + 2 * n + 2 * n + 4 * n}
    b["total"] = sum(b.values())
    return b


def pct(ms):
    p10, p50, p90 = np.percentile(np.asarray(ms, dtype=np.float64), [10, 50, 90])
    return {"p10": float(p10), "p50": float(p50), "p90": float(p90), "n": len(ms)}


def make_pair(W, H, dev, seed=0):
    """Noise with a disparity that grows towards the bottom of the image (a ground plane), 3 to 60 pixels."""
    import torch
    rng = np.random.default_rng(seed)
    left = rng.integers(0, 256, (H, W + 64), dtype=np.uint8)
    right = np.empty((H, W), dtype=np.uint8)
    for y in range(H):
        d = 3 + (57 * y) // max(H - 1, 1)
        right[y] = left[y, d:d + W]
    return torch.from_numpy(np.ascontiguousarray(left[:, :W])).to(dev), torch.from_numpy(right).to(dev)


def run_calls(calls, warmup, timed, only=None):
    import torch
    from segs_slam_amd import stereo
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    runs = []
    for name, W, H, fx, baseline in SHAPES:
        left, right = make_pair(W, H, dev)
        for paths in (4, 8):
            if only is not None and only != f"{name}:{paths}":
                continue
            sgm = stereo.StereoSGM(H, W, dev, num_disparities=D, paths=paths)
            for _ in range(warmup):
                depth = sgm.compute_depth(left, right, fx, baseline)
            torch.cuda.synchronize()
            r = {"shape": name, "image": [W, H], "num_disparities": D, "paths": paths, "temp_bytes": int(sgm.temp.numel()),
                 "valid_fraction": float((depth > 0).float().mean().item())}
            if timed:
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(calls + 1)]
                ev[0].record()
                for i in range(calls):
                    sgm.compute_depth(left, right, fx, baseline)
                    ev[i + 1].record()
                torch.cuda.synchronize()
                r["compute_depth_ms_hip_events"] = pct([ev[i].elapsed_time(ev[i + 1]) for i in range(calls)])
            else:
                for _ in range(calls):
                    sgm.compute_depth(left, right, fx, baseline)
                torch.cuda.synchronize()
            b = design_bytes(W, H, D, paths)
            r["design_bytes"] = b
            r["design_bytes_over_hbm_rate_ms"] = {k: v / HBM_BYTES_PER_S * 1e3 for k, v in b.items()}
            runs.append(r)
            print(json.dumps(r), flush=True)
            del sgm
    return runs


def kernel_stats(calls, warmup):
    """One fresh child process per shape and path count under rocprofv3 (started before this process touches the GPU): average
    time per launch of every kernel of csrc/stereo_sgm.hip."""
    out = []
    for name, W, H, _, _ in SHAPES:
        for paths in (4, 8):
            with tempfile.TemporaryDirectory() as d:
                cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "run", "--",
                       sys.executable, os.path.abspath(__file__), "--child", f"{name}:{paths}", "--calls", str(calls),
                       "--warmup", str(warmup)]
                subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=400)
                files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
                if not files:
                    raise RuntimeError("rocprofv3 wrote no kernel_stats.csv")
                rows = []
                with open(files[0]) as f:
                    for r in csv.DictReader(f):
                        if any(k in r["Name"] for k in KERNELS):
                            rows.append({"kernel": r["Name"], "launches": int(r["Calls"]), "average_us": float(r["AverageNs"]) / 1e3,
                                         "total_ms": float(r["TotalDurationNs"]) / 1e6})
            per_call = sum(r["total_ms"] for r in rows) / (calls + warmup)
            entry = {"shape": name, "image": [W, H], "paths": paths, "kernels": rows, "kernel_ms_per_call": per_call}
            print(json.dumps(entry), flush=True)
            out.append(entry)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--kernel-stats", action="store_true")
    ap.add_argument("--child", default=None, metavar="SHAPE:PATHS", help="the traced run: that configuration's calls alone")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child:
        run_calls(a.calls, a.warmup, timed=False, only=a.child)
        return
    stats = kernel_stats(a.calls, a.warmup) if a.kernel_stats else None
    import torch
    res = {"tool": "tools/time_stereo_sgm.py", "device": torch.cuda.get_device_name(0) if torch.cuda.is_available() else None,
           "method": "whole call: one HIP event pair per compute_depth after warm-up, one process; per kernel: rocprofv3 --kernel-trace "
                     "--stats of one child process per configuration making the same calls",
           "hbm_bytes_per_s": HBM_BYTES_PER_S, "runs": run_calls(a.calls, a.warmup, timed=True)}
    if stats is not None:
        res["kernel_stats"] = stats
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
