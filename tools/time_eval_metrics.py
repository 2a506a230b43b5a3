#!/usr/bin/env python3
"""Cost of the keyframe evaluation, measured on the GPU in ONE process.

At 640x480 and 1200x680, three ways to the numbers of one keyframe are timed in alternation, each after its own warm-up, with one
HIP event pair around a window of at least 0.3 s of back-to-back calls (per-call time = window / calls; median and range over the
rounds):

 * `measure`      FusedImageMetrics.measure (row mask on): three launches, nothing read back;
 * `torch chain`  the reference's op chain on the same device: mask, loss_utils.ssim, psnr, psnr_gaussian_splatting and the
                  three .item() readbacks (src/gaussian_mapper.cpp:1811-1818);
 * `fused loss`   FusedL1SSIM.__call__, which also writes a gradient and three derivative maps.

Then `KeyframeEvaluator.evaluate_all` over 32 keyframes of a small synthetic map at 1200x680 against 32 x (render + torch chain),
by the host clock around work that ends in a synchronise, alternated as well.

usage (GPU box): python tools/time_eval_metrics.py [--out profiles/eval_metrics_time.json]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from segs_slam_amd import evaluation as ev, loss_utils, mapper_config as mc, neural_gaussians as ng, scenes  # noqa: E402
from segs_slam_amd.gaussian_trainer import FusedL1SSIM  # noqa: E402

SIZES = ((480, 640), (680, 1200))       # (H, W)
WINDOW_S = 0.3


def torch_chain(image, gt):
    mask = (gt != 0).any(-1).to(torch.float32).unsqueeze(-1)
    x, t = image * mask, gt * mask
    return loss_utils.ssim(x, t).item(), loss_utils.psnr(x, t).item(), loss_utils.psnr_gaussian_splatting(x, t).item()


def window(fn, calls):
    """ms per call of `calls` back-to-back calls between one event pair."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def alternate(arms, rounds, warmup=20):
    """{name: per-call ms of each round}; the call count of an arm is fixed once from a pilot so that a window lasts WINDOW_S."""
    calls = {}
    for name, fn in arms.items():
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        pilot = window(fn, 20)
        calls[name] = max(20, int(np.ceil(WINDOW_S * 1e3 / pilot)))
    out = {name: [] for name in arms}
    for _ in range(rounds):
        for name, fn in arms.items():
            out[name].append(window(fn, calls[name]))
    return out, calls


def summary(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms)), "rounds": [float(v) for v in ms]}


def per_keyframe(dev, rounds):
    res = {}
    for H, W in SIZES:
        g = torch.Generator(device=dev).manual_seed(H)
        gt = torch.rand(3, H, W, device=dev, generator=g)
        image = (gt + 0.1 * torch.randn(3, H, W, device=dev, generator=g)).clamp(0, 1).contiguous()
        fm = ev.FusedImageMetrics(H, W, dev, 4)
        loss = FusedL1SSIM(H, W, dev, 0.2)
        arms = {"measure": lambda: fm.measure(image, gt, 1, row_mask=True),
                "torch chain": lambda: torch_chain(image, gt),
                "fused loss": lambda: loss(image, gt)}
        ms, calls = alternate(arms, rounds)
        row = fm.results()[1]
        chain = torch_chain(image, gt)
        res[f"{W}x{H}"] = {name: dict(summary(v), calls_per_window=calls[name]) for name, v in ms.items()}
        res[f"{W}x{H}"]["values"] = {"measure (ssim, psnr, psnr_gs)": [float(v) for v in row[:3]], "torch chain": [float(v) for v in chain]}
        for name, v in ms.items():
            print(f"{W}x{H}  {name:12s} median {np.median(v) * 1e3:8.1f} us  range {np.min(v) * 1e3:.1f} .. {np.max(v) * 1e3:.1f} us  "
                  f"({calls[name]} calls per window, {len(v)} rounds)")
    return res


def whole_set(dev, rounds, anchors, n_kf):
    cfg = mc.load_committed_config("cfg/gaussian_mapper/RGB-D/Replica/office0.yaml")
    cam = scenes.make_config_camera("c2")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    kf = ng.Keyframe(t(cam.world_view_transform), t(cam.full_proj_transform), t(cam.camera_center),
                     torch.tensor([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0], device=dev), cam.tanfovx, cam.tanfovy)
    model = ng.synthetic_model(anchors, cfg.model, cam, dev, seed=0)
    step = mc.make_mapper_step(cfg, model, cam.width, cam.height)
    g = torch.Generator(device=dev).manual_seed(1)
    gts = [torch.rand(3, cam.height, cam.width, device=dev, generator=g) for _ in range(4)]
    items = [(i, kf, gts[i % 4]) for i in range(n_kf)]
    evaluator = ev.KeyframeEvaluator(step, ev.RecordParams())

    def fused():
        return evaluator.evaluate_all(items)

    def chain():
        out = []
        for _, k, gt in items:
            out.append(torch_chain(step.render(k), gt))
        torch.cuda.synchronize()
        return out

    for fn in (fused, chain):           # warm-up: calibrates the rasterizer's resident buffers, loads the code objects
        fn()
        fn()
    times = {"evaluate_all": [], "render + torch chain": []}
    for _ in range(rounds):
        for name, fn in (("evaluate_all", fused), ("render + torch chain", chain)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
    rep = fused()
    res = {name: summary(v) for name, v in times.items()}
    res.update(keyframes=n_kf, anchors=anchors, size=f"{cam.width}x{cam.height}", render_ms_mean=rep.render_ms_mean)
    for name, v in times.items():
        print(f"{n_kf} keyframes, {anchors} anchors, {cam.width}x{cam.height}  {name:22s} median {np.median(v):7.2f} ms  "
              f"range {np.min(v):.2f} .. {np.max(v):.2f} ms")
    print(f"mean render time inside evaluate_all: {rep.render_ms_mean:.3f} ms per keyframe")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--anchors", type=int, default=20000)
    ap.add_argument("--keyframes", type=int, default=32)
    ap.add_argument("--out", default="profiles/eval_metrics_time.json")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_eval_metrics.py measures on the GPU; none is available")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "window_s": WINDOW_S, "per_keyframe": per_keyframe(dev, a.rounds),
           "whole_set": whole_set(dev, a.rounds, a.anchors, a.keyframes)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
