#!/usr/bin/env python3
"""Generates tests/golden/loss_reference_scales.npz: the REFERENCE's multi_scale_loss pieces at the other shipped scale counts.

Mapper.scale_num is 3 in most shipped configurations (tests/golden/loss_reference.npz covers that) but 2, 4 and 5 in others;
scale i is 1 / 2^i for i < scale_num.  This evaluates oracle/ref/loss_driver.cpp::ref_multi_scale_loss (the reference's own
high_frequency_loss on the two interpolate calls per scale, LibTorch CPU autograd) for n in {2, 4, 5} on the img / gt of
every case of loss_reference.npz, read back from that file so both fixtures share their inputs.

Keys: case{k}_n{n}_multi_scale = [sum, loss of scale 0, ..., loss of scale n-1] (float32, like the three-scale fixture) and
case{k}_n{n}_dL_multi_scale = the gradient w.r.t. img, stored where every level is at least 1 x 1 (every case: the 16 x 16
one meets a 1 x 1 level at scale 1/16), except the largest case's at n = 2 and 4 -- they would take the file past 0.5 MB, and
its n = 5 gradient runs through the same first four levels.  Runs only where the reference tree exists (`make -C oracle ref`).
Re-running it reproduces the committed file byte for byte."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SCALE_COUNTS = (2, 4, 5)

subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "ref", "-s"])
import torch  # noqa: E402,F401  (loads libtorch before the driver)
lib = C.CDLL(os.path.join(ROOT, "oracle", "_ref", "libloss_ref.so"))
lib.ref_multi_scale_loss.restype = C.c_int
lib.ref_multi_scale_loss.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]

src = np.load(os.path.join(GOLDEN, "loss_reference.npz"))
cases = sorted({k.split("_")[0] for k in src.files})
largest = max(src[f"{c}_img"].shape[1] * src[f"{c}_img"].shape[2] for c in cases)
out = {}
for case in cases:
    img, gt = np.ascontiguousarray(src[f"{case}_img"]), np.ascontiguousarray(src[f"{case}_gt"])
    _, H, W = img.shape
    for n in SCALE_COUNTS:
        scales = np.array([1.0 / 2 ** i for i in range(n)], np.float32)
        ms = np.zeros(n + 1, np.float32)
        dM = np.zeros((3, H, W), np.float32)
        assert lib.ref_multi_scale_loss(img.ctypes.data, gt.ctypes.data, H, W, scales.ctypes.data, n, ms.ctypes.data, dM.ctypes.data) == 0
        out[f"{case}_n{n}_multi_scale"] = ms
        smallest = min(math.floor(H * float(scales[-1])), math.floor(W * float(scales[-1])))
        if smallest >= 1 and not (H * W == largest and n < 5):
            out[f"{case}_n{n}_dL_multi_scale"] = dM
        print(case, H, W, n, ms)
np.savez_compressed(os.path.join(GOLDEN, "loss_reference_scales.npz"), **out)
