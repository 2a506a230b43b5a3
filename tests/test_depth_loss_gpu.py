"""segs_depth_target / segs_depth_loss (include/segs_train.h, csrc/depth_loss.hip) alone, against the float64
restatement tests/_depth_loss_ref.py on synthetic maps.

Inputs.  A in [0.05, 1], D = A z with z in [0.5, 5]; the compared depth is d = D (normalize = 0) or the float64 quotient D / A
(normalize = 1), and Z = float32(d (1 +- r)) with r in [0.25, 0.5].  So |d - Z| >= 0.25 d >= 1e-3 max(Z, 1) (d >= 0.025, Z <= 7.5)
and the sign of d - Z is the same in both precisions on EVERY pixel: nothing is left out of a comparison.  In normalize = 0 mode a
few pixels carry Z == D bit for bit (the difference is exactly 0 in both precisions: s = 0).  All pixel classes of the definition
are planted in every input (`_plant`).

Bars (u = 2^-24, one float32 rounding).
 * gradients, normalize = 0: the device forms float32(lambda) / float32(n) -- n < 2^24 is exact, the IEEE quotient is one rounding
   of the number whose float32 rounding the reference takes -- so at most 1 ulp apart; the bar is the issue's 2 ulp, sign exact,
   every other entry exactly 0.
 * gradients, normalize = 1: dL/dD = s (lambda/n) / A is two roundings; dL/dA = -(dL/dD) (D/A) - lambda_alpha/n is four roundings
   in its first term t1, one in the second t2 and one in the difference.  With lambda_alpha = 0.1 lambda_depth, d >= 0.5 and
   A <= 1, |t2| <= 0.2 |t1|, so the difference keeps >= 0.8 |t1| and the relative error is <= (4 + 0.2 + 1.2) u / 0.8 < 7 u,
   inside the issue's 1e-6 (16.8 u).
 * values: all terms are non-negative, so a chain of c roundings gives a relative error <= c u (1 + O(u)).  The chain built in
   csrc/depth_loss.hip, longest path: the term itself 5 (normalize: the quotient's rounding u d <= 4 u |d - Z| as r >= 0.25, then
   the subtraction; 1 otherwise), a thread's 4 pixels 4, the wave's shuffle tree 6, the four waves 2, in the second launch
   ceil(workgroups / 256) = 1 serial add per thread at these sizes, again 6 + 2, the division by n 1, and for the total two
   products and one sum 3:  c = 5 + 4 + 6 + 2 + 1 + 6 + 2 + 1 + 3 = 30.
 * N and the number of used pixels are integers: exact."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import _depth_loss_ref as ref  # noqa: E402

C_CHAIN = 30
U = 2.0 ** -24
SPAN = 1024                     # pixels per workgroup of depth_loss_kernel (256 threads x 4)
INVALID_ARGUMENT = -1           # SEGS_ERR_INVALID_ARGUMENT (include/segs_raster.h)
MIN_DEPTH, MAX_DEPTH = 0.01, 10.0

# (H, W): less than one workgroup with W % 4 == 1; 64 x 64; exactly one span; one span plus a pixel; many workgroups
SIZES = [(17, 33), (64, 64), (32, 32), (25, 41), (187, 333)]
CONFIGS = {
    "plain": ref.Params(1.0, 0.0, 0.0, False, MIN_DEPTH, MAX_DEPTH),
    "silhouette": ref.Params(0.7, 0.3, 0.5, False, MIN_DEPTH, MAX_DEPTH),
    "normalize": ref.Params(1.0, 0.1, 0.5, True, MIN_DEPTH, MAX_DEPTH),
    "unbounded": ref.Params(1.0, 0.25, 0.0, False, MIN_DEPTH, 0.0),           # max_depth = 0: no upper bound
}


def _plant(D, A, Z, p):
    """Every pixel class, at fixed places of the flat maps (first and last pixel included)."""
    n = D.numel()
    D, A, Z = D.view(-1), A.view(-1), Z.view(-1)
    at = [0, 3, 7, 31, 64, 65, 130, n // 2, n - 2, n - 1, n // 3, n // 3 + 1, 200, 201, 202]
    assert len(set(at)) == len(at) and max(at) < n
    Z[at[0]], Z[at[1]], Z[at[2]], Z[at[3]], Z[at[4]] = float("nan"), float("inf"), float("-inf"), 0.0, -1.5
    Z[at[5]] = MIN_DEPTH                                 # exactly the bounds: invalid (strict comparisons)
    Z[at[6]] = MAX_DEPTH if p.max_depth > 0 else 1000.0  # without an upper bound a far pixel is valid
    D[at[7]], A[at[7]], Z[at[7]] = 0.0, 0.0, 1.0         # a pixel no Gaussian reaches
    D[at[9]], A[at[9]], Z[at[9]] = 0.0, 0.0, 2.0
    if p.alpha_min > 0:
        a = np.float32(p.alpha_min)
        for i, av in ((at[10], a), (at[11], np.nextafter(a, np.float32(0)))):      # on the threshold (used), one ulp below (not)
            z = float(D[i] / A[i])
            A[i] = float(av)
            D[i] = A[i] * z
            dd = D[i].double() / A[i].double() if p.normalize else D[i].double()
            Z[i] = (dd * 1.4).float()
    if not p.normalize:
        for i in at[12:15]:                              # ties, bit for bit, on pixels that are used
            A[i] = 0.9
            Z[i] = D[i]


def _inputs(H, W, p, seed=0):
    g = torch.Generator().manual_seed(1000 * H + W + seed)
    A = (0.05 + 0.95 * torch.rand(H, W, generator=g, dtype=torch.float64)).float()
    D = (A.double() * (0.5 + 4.5 * torch.rand(H, W, generator=g, dtype=torch.float64))).float()
    d = D.double() / A.double() if p.normalize else D.double()
    r = 0.25 + 0.25 * torch.rand(H, W, generator=g, dtype=torch.float64)
    Z = (d * torch.where(torch.rand(H, W, generator=g) < 0.5, 1 + r, 1 - r)).float()
    _plant(D, A, Z, p)
    return D, A, Z


def _run(D, A, Z, p, misalign=0, loss_word=None, calls=1, fill=7.0):
    """The two entry points through ctypes on buffers that start `misalign` floats into their storage.  Returns CPU tensors."""
    from segs_slam_amd import _capi
    lib = _capi.lib()
    dev = torch.device("cuda:0")
    H, W = D.shape
    n = H * W

    def place(t, extra=0):
        store = torch.zeros(n + extra + misalign, dtype=torch.float32, device=dev)
        v = store[misalign:]
        v[:n] = t.reshape(-1).to(dev)
        assert v.data_ptr() % 16 == (4 * misalign) % 16
        return v

    tf = lib.segs_depth_target_floats(H, W)
    d_, a_, z_ = place(D), place(A), place(Z)
    tgt = torch.full((tf + misalign,), fill, dtype=torch.float32, device=dev)[misalign:]
    gD = torch.full((n + misalign,), fill, dtype=torch.float32, device=dev)[misalign:]
    gA = torch.full((n + misalign,), fill, dtype=torch.float32, device=dev)[misalign:]
    out = torch.full((4,), fill, dtype=torch.float32, device=dev)
    word = None if loss_word is None else torch.tensor([loss_word], dtype=torch.float32, device=dev)
    temp = torch.empty(lib.segs_depth_loss_temp_bytes(H, W), dtype=torch.uint8, device=dev)
    cp = _capi.DepthLossParamsC(p.lambda_depth, p.lambda_alpha, p.alpha_min, int(p.normalize))
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    st_t = lib.segs_depth_target(ptr(z_), H, W, p.min_depth, p.max_depth, ptr(tgt), None)
    results = []
    st = None
    if st_t == 0:
        for _ in range(calls):
            st = lib.segs_depth_loss(ptr(d_), ptr(a_), ptr(tgt), H, W, C.byref(cp), ptr(gD), ptr(gA), ptr(out),
                                     None if word is None else ptr(word), ptr(temp), None)
            torch.cuda.synchronize()
            results.append(dict(gD=gD[:n].cpu().view(H, W).clone(), gA=gA[:n].cpu().view(H, W).clone(), out=out.cpu().clone()))
    torch.cuda.synchronize()
    return dict(status_target=st_t, status=st, target=tgt[:n].cpu().view(H, W), N=int(tgt[n:n + 1].view(torch.int32).item()),
                word=None if word is None else word.cpu(), calls=results, raw_target=tgt.cpu())


def _check(D, A, Z, p, got):
    res = got["calls"][0]
    total, l_depth, l_alpha, n_used, N = ref.value(D, A, Z, p)
    wD, wA, s = ref.gradients(D, A, Z, p)
    valid, used = ref.masks(A, Z, p)
    H, W = D.shape
    assert -(-H * W // SPAN) <= 256              # one serial add per thread in the second launch: C_CHAIN holds
    # the target map and N
    assert got["N"] == N and 0 < N < D.numel()
    assert torch.equal(got["target"], ref.target_map(Z, p))
    assert float(res["out"][3]) == n_used and 0 < n_used
    # gradients
    hD, hA = res["gD"].double(), res["gA"].double()
    assert bool(torch.isfinite(hD).all()) and bool(torch.isfinite(hA).all())
    assert bool((hD[~used] == 0).all()) and bool((hA[~valid] == 0).all())
    n = max(N, 1)
    if not p.normalize:
        gd = np.float32(ref.f32(p.lambda_depth) / n)
        ga = np.float32(ref.f32(p.lambda_alpha) / n)
        assert bool(torch.equal(torch.sign(hD), s))                          # the exact sign, 0 on the planted ties
        assert int(((s == 0) & used).sum()) == 3
        err = (hD.abs() - float(gd))[s != 0].abs()
        print(f"dL/dD: worst {float(err.max() / np.spacing(gd)):.2f} ulp of {gd}")
        assert float(err.max()) <= 2 * float(np.spacing(gd))
        assert float((hA[valid] + float(ga)).abs().max()) <= 2 * float(np.spacing(ga)) if ga > 0 else bool((hA == 0).all())
        assert bool((hA[valid] <= 0).all())
    else:
        for name, have, want in (("dL/dD", hD, wD), ("dL/dA", hA, wA)):
            rel = ((have - want).abs() / want.abs())[want != 0]
            print(f"{name}: worst relative error {float(rel.max()):.2e} ({float(rel.max()) / U:.1f} u)")
            assert bool((have[want == 0] == 0).all())
            assert float(rel.max()) <= 1e-6
    # values
    for name, have, want in (("total", res["out"][0], total), ("L_depth", res["out"][1], l_depth), ("L_alpha", res["out"][2], l_alpha)):
        rel = abs(float(have) - float(want)) / float(want)
        print(f"{name}: {float(have):.8g} vs {float(want):.10g}: {rel / U:.2f} u (bar {C_CHAIN} u)")
        assert float(want) > 0 and rel <= C_CHAIN * U
    assert float(res["out"][0]) >= 0


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[1]}x{s[0]}")
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_kernel_matches_float64(cfg, size):
    p = CONFIGS[cfg]
    D, A, Z = _inputs(*size, p)
    got = _run(D, A, Z, p, calls=2)
    assert got["status_target"] == 0 and got["status"] == 0
    _check(D, A, Z, p, got)
    # both maps were overwritten in full (they held 7.0), and the second call gives the same bits
    assert not bool((got["calls"][0]["gD"] == 7.0).any()) and not bool((got["calls"][0]["gA"] == 7.0).any())
    for k in ("gD", "gA", "out"):
        assert torch.equal(got["calls"][0][k], got["calls"][1][k]), k
    # the words behind N stay the target's own
    assert got["raw_target"].numel() == D.numel() + 4


@pytest.mark.parametrize("cfg", ["silhouette", "normalize"])
def test_pointers_that_are_only_four_byte_aligned(cfg):
    p = CONFIGS[cfg]
    for size in ((25, 41), (187, 333)):
        D, A, Z = _inputs(*size, p, seed=5)
        got = _run(D, A, Z, p, misalign=1)
        assert got["status_target"] == 0 and got["status"] == 0
        _check(D, A, Z, p, got)
        aligned = _run(D, A, Z, p)
        # the same gradients as the vector form (the sums are folded in another order there: values agree within the bar only)
        assert torch.equal(got["calls"][0]["gD"], aligned["calls"][0]["gD"]) and torch.equal(got["calls"][0]["gA"], aligned["calls"][0]["gA"])
        assert torch.equal(got["target"], aligned["target"]) and got["N"] == aligned["N"]


def test_loss_word_grows_by_the_total_with_one_float32_addition():
    p = CONFIGS["silhouette"]
    D, A, Z = _inputs(25, 41, p, seed=9)
    start = 0.62512344
    got = _run(D, A, Z, p, loss_word=start, calls=2)
    total = np.float32(got["calls"][0]["out"][0].item())
    once = np.float32(start) + total
    assert total > 0 and np.float32(got["word"].item()) == np.float32(once + total)      # two calls: two additions


def test_no_valid_pixel_gives_zero_everywhere():
    for cfg in ("plain", "normalize"):
        p = CONFIGS[cfg]
        D, A, _ = _inputs(25, 41, p)
        Z = torch.zeros_like(D)
        Z.view(-1)[::3] = float("nan")
        Z.view(-1)[1::3] = MAX_DEPTH + 1
        got = _run(D, A, Z, p, loss_word=1.5)
        res = got["calls"][0]
        assert got["status"] == 0 and got["N"] == 0 and bool((got["target"] == 0).all())
        assert res["out"].tolist() == [0.0, 0.0, 0.0, 0.0] and float(got["word"]) == 1.5
        assert bool((res["gD"] == 0).all()) and bool((res["gA"] == 0).all())


def test_invalid_arguments_leave_the_outputs_untouched():
    p = CONFIGS["plain"]
    D, A, Z = _inputs(17, 33, p)
    bad = _run(D, A, Z, p._replace(normalize=True, alpha_min=0.0), loss_word=2.0)       # normalize without a threshold
    assert bad["status_target"] == 0 and bad["status"] == INVALID_ARGUMENT
    res = bad["calls"][0]
    assert bool((res["gD"] == 7.0).all()) and bool((res["gA"] == 7.0).all()) and bool((res["out"] == 7.0).all())
    assert float(bad["word"]) == 2.0
    neg = _run(D, A, Z, p._replace(min_depth=-0.5))                                     # negative min_depth
    assert neg["status_target"] == INVALID_ARGUMENT and bool((neg["raw_target"] == 7.0).all())
    from segs_slam_amd import _capi
    assert b"min_depth" in _capi.lib().segs_last_error()


def test_host_object_prepares_caches_and_refuses_cpu_tensors():
    from segs_slam_amd.depth_loss import DepthLossParams, DepthTarget, FusedDepthLoss
    dev = torch.device("cuda:0")
    p = CONFIGS["silhouette"]
    H, W = 25, 41
    D, A, Z = _inputs(H, W, p)
    fn = FusedDepthLoss(H, W, dev, DepthLossParams(*p))
    d, a, z = D.to(dev), A.to(dev), Z.to(dev)
    tgt = fn.prepare(z)
    assert isinstance(tgt, DepthTarget) and tgt.shape == (H, W) and tgt.block.numel() == H * W + 4
    word = torch.zeros(1, device=dev)
    value, gD, gA = fn(d, a, tgt, word)
    first = (value.clone(), gD.clone(), gA.clone(), fn.out.clone())
    assert tgt.n_valid() == ref.value(D, A, Z, p)[4] and torch.equal(word[0], value)
    value2, gD2, gA2 = fn(d, a, z)                      # a raw tensor: prepared through the cache, the same bits
    assert gD2.data_ptr() == gD.data_ptr() and gA2.data_ptr() == gA.data_ptr()          # the buffers are made once
    for x, y in zip(first, (value2, gD2, gA2, fn.out)):
        assert torch.equal(x, y)
    assert len(fn._targets) == 1
    fn(d, a, z)
    assert len(fn._targets) == 1                        # a hit
    others = [z.clone() for _ in range(12)]
    for o in others:
        fn(d, a, o)
    assert len(fn._targets) == FusedDepthLoss.MAX_CACHED_TARGETS == 8
    z.add_(0.0)                                         # a new version of the same storage is a new target
    fn(d, a, z)
    assert (z.data_ptr(), z._version) in fn._targets
    with pytest.raises(RuntimeError):
        fn(D, A, tgt)
    with pytest.raises(RuntimeError):
        fn.prepare(Z)
    with pytest.raises(ValueError):
        fn.prepare(torch.zeros(H + 1, W, device=dev))
    with pytest.raises(ValueError):
        fn(d, a, DepthTarget(torch.zeros((H + 1) * W + 4, device=dev), H + 1, W))
