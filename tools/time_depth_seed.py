#!/usr/bin/env python3
"""Cost of seeding anchors from a depth frame, measured on the GPU in ONE process, at 1200x680 with stride 4
and stride 2, on two maps: the config-5 map (300 k anchors x 10 offsets, ScanNet model dimensions) and the Replica-size map
(50 k anchors, cfg values of RGB-D/Replica/office0.yaml):

 * the bare segs_depth_seed call against the map's rendered depth / opacity (HIP events around batches of back-to-back calls;
   the call appends nothing, so every call sees the same map);
 * one ScaffoldTrainerStep.seed_keyframe -- forward, segs_depth_seed, the host read of the counts and the append -- by the host
   clock around the synchronising call (p50 of a few calls, each on a fresh copy of the map state: the model's row count is
   put back after every call);
 * one mapper iteration (training_once) of the same step at the same size, per-step HIP events.

usage (GPU box): python tools/time_depth_seed.py [--out profiles/depth_seed_time.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from segs_slam_amd import _capi, mapper_config as mc, neural_gaussians as ng, scenes  # noqa: E402
from segs_slam_amd.densify import AnchorDensifier, DensifyParams, DepthSeedParams, cam_to_world_of  # noqa: E402


def p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def pct(ms):
    p10, p50, p90 = np.percentile(np.asarray(ms, dtype=np.float64), [10, 50, 90])
    return {"p10": float(p10), "p50": float(p50), "p90": float(p90), "n": len(ms)}


def make_step(which, dev, seed_params):
    if which == "config5":
        cam = scenes.make_config_camera("c5")
        dims = ng.ModelDims(appearance_dim=16, use_feat_bank=False)
        model = ng.synthetic_model(300_000, dims, cam, dev, seed=0)
        step = ng.ScaffoldTrainerStep(model, cam.width, cam.height, depth_seed=seed_params)
        step.enable_densification(AnchorDensifier(model, DensifyParams(voxel_size=0.01, update_until=0)))
    else:
        cfg = mc.load_committed_config("cfg/gaussian_mapper/RGB-D/Replica/office0.yaml")
        cam = scenes.make_config_camera("c2")
        cfg.densify.update_until = 0
        cfg.densify.voxel_size = 0.01
        model = ng.synthetic_model(50_000, cfg.model, cam, dev, seed=0)
        step = mc.make_mapper_step(cfg, model, cam.width, cam.height, depth_seed=seed_params)
    step.keyframe_for = lambda s, n: 0
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    kf = ng.Keyframe(t(cam.world_view_transform), t(cam.full_proj_transform), t(cam.camera_center),
                     torch.tensor([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0], device=dev), cam.tanfovx, cam.tanfovy)
    return step, kf, cam


def bare_call_us(step, kf, target, sp, calls=50, rounds=5):
    m, lib = step.model, step._lib
    H, W = target.shape
    depth, alpha = step.engine.out_depth, step.engine.out_alpha
    n_lat = len(range(sp.stride // 2, H, sp.stride)) * len(range(sp.stride // 2, W, sp.stride))
    temp = torch.empty(lib.segs_depth_seed_temp_bytes(m.A, H, W, sp.stride), dtype=torch.uint8, device=m.device)
    out = torch.empty((n_lat, 3), dtype=torch.float32, device=m.device)
    words = torch.zeros(8, dtype=torch.int32, device=m.device)
    cp = _capi.DepthSeedParamsC(sp.stride, sp.alpha_max, int(sp.use_front), sp.front_abs, sp.front_rel, step.densifier.p.voxel_size)
    M = cam_to_world_of(kf.view)
    stream = C.c_void_p(torch.cuda.current_stream(m.device).cuda_stream)

    def call():
        _capi.check(lib.segs_depth_seed(m.A, p(m.param("anchor")), H, W, p(target), p(depth), p(alpha), float(kf.tanfovx),
                                        float(kf.tanfovy), M, C.byref(cp), n_lat, p(out), C.c_void_p(words.data_ptr() + 24), p(words),
                                        p(temp), stream), "segs_depth_seed")
    for _ in range(5):
        call()
    res = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            call()
        e1.record()
        torch.cuda.synchronize()
        res.append(e0.elapsed_time(e1) / calls * 1e3)
    return {"best_us": float(min(res)), "median_us": float(np.median(res)), "calls_per_round": calls, "rounds": rounds,
            "lattice_pixels": n_lat, "temp_bytes": int(temp.numel()), "counts": dict(zip(
                ("valid lattice pixels", "unobserved", "in front", "out of range", "distinct voxels", "new anchors"), words[:6].tolist()))}


def measure(which, dev, stride, steps, warmup, seeds):
    sp = DepthSeedParams(stride=stride)
    step, kf, cam = make_step(which, dev, sp)
    m = step.model
    g = torch.Generator(device=dev).manual_seed(0)
    gt = torch.rand(3, cam.height, cam.width, device=dev, generator=g)
    z = 1.0 + 5.0 * torch.rand(cam.height, cam.width, device=dev, generator=g)        # the synthetic map's depth range
    z[torch.rand(cam.height, cam.width, device=dev, generator=g) < 0.1] = 0.0          # 10 % holes, as a sensor has
    for _ in range(warmup):
        step.training_once([kf], [gt])
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    ev[0].record()
    for i in range(steps):
        step.training_once([kf], [gt])
        ev[i + 1].record()
    step.finish()
    torch.cuda.synchronize()
    iteration_ms = [ev[i].elapsed_time(ev[i + 1]) for i in range(steps)]
    target = step._seed_target(z)
    step.render(kf)
    torch.cuda.synchronize()
    bare = bare_call_us(step, kf, target, sp)
    # whole seed_keyframe calls: the row count is put back after each, so that every call seeds the same map; the first call
    # (which grows the buckets) is reported apart from the later ones (which append inside the grown buckets)
    A0 = m.A
    wall, counts = [], None
    for _ in range(seeds + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        counts = step.seed_keyframe(kf, z)
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        m.A = A0
    return {"map": which, "anchors": A0, "image": [cam.width, cam.height], "stride": stride, "voxel_size": step.densifier.p.voxel_size,
            "segs_depth_seed_alone": bare, "seed_keyframe_counts": counts,
            "seed_keyframe_first_call_ms_host_clock": float(wall[0]), "seed_keyframe_ms_host_clock": pct(wall[1:]),
            "mapper_iteration_ms_hip_events": pct(iteration_ms),
            "seed_keyframe_p50_over_iteration_p50": float(np.median(wall[1:]) / np.median(iteration_ms))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--seeds", type=int, default=7)
    ap.add_argument("--maps", default="replica,config5")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    res = {"tool": "tools/time_depth_seed.py", "device": torch.cuda.get_device_name(0),
           "method": "bare call: HIP events around back-to-back calls; seed_keyframe: host clock around the synchronising call; "
                     "iteration: one HIP event per training_once; all in one process", "runs": []}
    for which in a.maps.split(","):
        for stride in (4, 2):
            r = measure(which, dev, stride, a.steps, a.warmup, a.seeds)
            print(json.dumps(r))
            res["runs"].append(r)
            if a.out:                                  # written after every run: a later run that fails keeps the earlier ones
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "w") as f:
                    json.dump(res, f, indent=1)
                    f.write("\n")


if __name__ == "__main__":
    main()
