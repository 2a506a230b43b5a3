"""The two forms of the neural backward (csrc/neural.hip): neural_bwd_pair_kernel, which every shipped path runs, and
neural_bwd_kernel under SEGS_NEURAL_ONE_KERNEL_BACKWARD.  Both are callers of ONE copy of the per-slab gradients and of the
per-element write-out (request_*, output_gradients_*, relu_mask / input_gradients, the slab-tail helpers, store_partial_element,
store_small_sum, cam_fold); they keep their own dH chain, feature-bank epilogue, tile stores and weight-gradient schedule.

The tests hold the two forms against each other at the visible-anchor counts where their slab bookkeeping differs from the
40 001-anchor test of tests/test_neural_gpu.py: one anchor; 231 of 256 (one compaction workgroup, so the visible list is in
anchor order on every run; two backward workgroups, the second with slabs of 32 / 32 / 32 / 7); 32 936 = 32 768 + 128 + 40 (the
second round of the 256 persistent workgroups, where workgroup 1's pair 1 has 8 valid lanes and its pairs 2 and 3 are empty: the
"copy of the last anchor, stores nothing" lanes).  The float64 bars of the camera entry point at the same counts are in
tests/test_neural_camera_grad_gpu.py.

Against ANOTHER BUILD of the library (the parent commit's, which cannot be built from a checkout of this one) this module runs as
a script, once per library:
    SEGS_RASTER_LIB=/path/to/libsegs_raster.so python -m tests.test_neural_backward_forms_gpu dump a.npz
    python -m tests.test_neural_backward_forms_gpu dump b.npz && python -m tests.test_neural_backward_forms_gpu compare a.npz b.npz
The dump runs CASES[1] (plain, appearance 16), CASES[0] (feature bank), CASES[2] (every add_*_dist, no finishing kernel) and
CASES[3] (bank + dist) under flags 0 and SEGS_NEURAL_ONE_KERNEL_BACKWARD, through segs_neural_backward and
segs_neural_backward_camera, with scaling_reg_weight 0 and 0.01, at the three counts.  At one anchor and at 231 of 256 the whole
gradient bucket (MLP block included) and dL/dcamera_center are kept as raw bits and must be equal as int32.  At 32 936 the four
per-anchor segments are kept as bits; the MLP block and dL/dcamera_center depend on the order of the atomically compacted list
and are compared at 1e-5 x max|.| (the bound of test_wave_pair_backward_equals_the_one_kernel_backward), next to the difference
of two runs of the SAME build, which the dump records.  scaling_reg is a float atomic per wave: 1e-5 relative (_check_parity)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import neural_ref  # noqa: E402
from tests.test_neural_camera_grad_gpu import CAMPOS, ONE_KERNEL, POSE7, _scattered  # noqa: E402
from tests.test_neural_gpu import CASES  # noqa: E402

VISIBLE_COUNTS = [1, 231, 32936]
ORDERED = 2048          # up to one compaction workgroup of visible anchors the list is in anchor order: sums repeat bit for bit


@functools.lru_cache(maxsize=2)
def _inputs(case, n_visible):
    """CPU tensors of one (model, count): the model, the visibility and the candidate-domain gradients."""
    A, visible = _scattered(n_visible, case)
    rd = neural_ref.NeuralDims(**CASES[case])
    tensors = neural_ref.random_model(rd, A, 91 + case)
    g = torch.Generator().manual_seed(5 + n_visible)
    grads = [torch.randn(A * 10, n, generator=g) for n in (3, 3, 1, 3, 4)]
    return A, visible, tensors, grads


def _run(case, n_visible, flags, camera, reg_w, repeats=1):
    """model.grads (numpy, per repeat), dL/dcamera_center and scaling_reg of the last repeat, the per-anchor length."""
    from segs_slam_amd import _capi, neural_gaussians as ng
    dev = torch.device("cuda:0")
    A, visible, (anchor, offset, feat, scaling_log, mlp), grads = _inputs(case, n_visible)
    model = ng.ScaffoldModel(A, ng.ModelDims(**CASES[case]), dev)
    model.load(anchor, offset, feat, scaling_log, mlp)
    gen = ng.NeuralGaussians(model)
    radii = torch.where(visible, torch.tensor(3), torch.tensor(0)).to(torch.int32).to(dev)
    gen.forward(torch.tensor(CAMPOS, device=dev), torch.tensor(POSE7, device=dev), radii)
    dgrads = [x.to(dev) for x in grads]
    lib = _capi.lib()
    outs = []
    old = lib.segs_neural_set_flags(flags)
    try:
        for _ in range(repeats):
            model.grads.zero_()
            gen.backward(*dgrads, scaling_reg_weight=reg_w, camera_grad=camera)
            torch.cuda.synchronize()
            outs.append(model.grads.cpu().numpy().copy())
    finally:
        assert lib.segs_neural_set_flags(old) == flags
    cam = gen.dL_dcamera_center.cpu().numpy().copy() if camera else None
    reg = gen.scaling_reg.cpu().numpy().copy() if reg_w else None
    return outs, cam, reg, A * (3 + 30 + 32 + 6)


@pytest.mark.parametrize("n_visible", VISIBLE_COUNTS)
@pytest.mark.parametrize("case", [1, 0])        # plain model (ScanNet dimensions), feature-bank model (Replica dimensions)
def test_wave_pair_backward_equals_the_one_kernel_backward_at_visible_counts(case, n_visible):
    """test_wave_pair_backward_equals_the_one_kernel_backward (tests/test_neural_gpu.py) with its assertions at the counts above:
    per-anchor gradients bit-identical for the plain model and equal to rounding for the feature bank (its pairs form dL/dfeat
    through partial sums), MLP block within 1e-5 of its largest entry.

    The MLP block keeps the 1e-5 bound at 231 of 256 too, although the visible list is in anchor order there and both forms keep
    the same per-wave accumulators and the same (w0 + w1) + (w2 + w3) fold.  Measured on the parent of the change that made the
    helpers shared, and the same after it (profiles/r11_neural_bwd_shared.txt): with one anchor the block is bit-identical; at
    231 the plain model's second-layer weights, every bias and every feature column of the first layers are bit-identical, and
    12-23 entries per first-layer weight differ in the last bit (6.6e-9 of the block's largest entry), all of them in the view /
    dist columns 32..35.  Those are the sums wgrad_chain_tail keeps on the VALU (tl[] += av * t).  The likely cause (not
    read from the assembly): whether a product and its addition become one fused operation there is the compiler's choice per
    kernel; with a single anchor, where the sum starts from zero, both choices round once, which fits the equal bits there.  The weight-gradient schedule is one of the parts the two forms do not share."""
    (pair,), _, _, n_anchor = _run(case, n_visible, 0, False, 0.01)
    (one,), _, _, _ = _run(case, n_visible, ONE_KERNEL, False, 0.01)
    assert np.isfinite(pair).all() and np.abs(pair).max() > 0
    a, b = pair[:n_anchor], one[:n_anchor]
    print(f"case {case} visible {n_visible}: per-anchor equal {np.array_equal(a, b)}, MLP block equal "
          f"{np.array_equal(pair[n_anchor:], one[n_anchor:])}, MLP max diff / max "
          f"{np.abs(pair[n_anchor:] - one[n_anchor:]).max() / np.abs(pair[n_anchor:]).max():.2e}")
    if not CASES[case]["use_feat_bank"]:
        assert np.array_equal(a, b)
    else:
        assert np.abs(a - b).max() <= 2e-6 * np.abs(b).max() and np.mean(a != b) < 0.5
    a, b = pair[n_anchor:], one[n_anchor:]
    assert np.abs(a).max() > 0 and np.abs(a - b).max() <= 1e-5 * np.abs(a).max()


# ------------------------------------------------------------------------------------------- two builds of the library
DUMP_CASES = [1, 0, 2, 3]


def dump(path):
    out = {}
    bits = lambda x: np.ascontiguousarray(x).view(np.int32)  # noqa: E731
    for case in DUMP_CASES:
        for n_visible in VISIBLE_COUNTS:
            for flags in (0, ONE_KERNEL):
                for camera in (False, True):
                    for reg_w in (0.0, 0.01):
                        key = f"case{case}/visible{n_visible}/flags{flags}/{'camera' if camera else 'plain'}/reg{reg_w}"
                        ordered = n_visible <= ORDERED
                        outs, cam, reg, n_anchor = _run(case, n_visible, flags, camera, reg_w, repeats=1 if ordered else 2)
                        if ordered:
                            out[key + "/bucket:bits"] = bits(outs[0])
                            if camera:
                                out[key + "/camera_center:bits"] = bits(cam)
                        else:
                            out[key + "/per_anchor:bits"] = bits(outs[0][:n_anchor])
                            out[key + "/mlp:order"] = outs[0][n_anchor:]
                            out[key + "/mlp:rerun"] = outs[1][n_anchor:]
                            if camera:
                                out[key + "/camera_center:order"] = cam
                        if reg_w:
                            out[key + "/scaling_reg:reg"] = reg
    np.savez(path, **out)
    print("wrote", len(out), "arrays to", path)
    return 0


def compare(path_a, path_b):
    a, b = np.load(path_a), np.load(path_b)
    assert sorted(a.files) == sorted(b.files), sorted(set(a.files) ^ set(b.files))
    bad, n_bits, n_tol, worst, worst_same = 0, 0, 0, 0.0, 0.0
    for k in sorted(a.files):
        x, y = a[k], b[k]
        assert x.shape == y.shape and x.dtype == y.dtype, (k, x.dtype, y.dtype, x.shape, y.shape)
        kind = k.rsplit(":", 1)[1]
        if kind == "rerun":             # the second run of each build: the scale the order-dependent sums are read against
            continue
        if kind == "bits":
            n_bits += 1
            if not np.array_equal(x, y):
                at = int(np.flatnonzero(x != y)[0])
                print(f"DIFFERENT: {k}, {int((x != y).sum())} of {x.size}, first at {at}: {x.view(np.float32)[at]} against {y.view(np.float32)[at]}")
                bad += 1
            continue
        n_tol += 1
        scale = max(float(np.abs(x).max()), 1e-30)
        ratio = float(np.abs(x - y).max()) / scale
        worst = max(worst, ratio)
        if kind == "order" and k.endswith("/mlp:order"):
            for z in (a, b):
                again = z[k[:-len("order")] + "rerun"]
                worst_same = max(worst_same, float(np.abs(z[k] - again).max()) / scale)
        if ratio > 1e-5:
            print(f"DIFFERENT: {k}: max |a - b| / max |a| = {ratio:.3e}")
            bad += 1
    print(f"{n_bits} arrays compared as int32, {n_tol} at 1e-5 (worst {worst:.2e} of the largest entry; two runs of one build differ "
          f"by up to {worst_same:.2e} in the MLP block);", "all equal" if not bad else f"{bad} DIFFERENT")
    return 1 if bad else 0


if __name__ == "__main__":
    import sys
    sys.exit(dump(sys.argv[2]) if sys.argv[1] == "dump" else compare(sys.argv[2], sys.argv[3]))
