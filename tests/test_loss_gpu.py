"""The fused L1 + SSIM loss (csrc/loss.hip, segs_l1_ssim_loss) against a float64 reference, per input class and at the sizes
where its tiling can go wrong (tests/_loss_ref.py holds the reference, the yardstick and the inputs).

Bars, per case, float32 kernel output against the float64 chain:
    dL      : max|dL - g64| <= 4 e_ref(dL) + 4 * 2^-23 * max|g64|
    scalars : |out[i] - ref64[i]| <= 4 e_ref(scalar_i) + 2e-6
where e_ref is the distance of the reference's own float32 op chain from float64 on the same input.  The factor 4 is a margin over
that chain, not over the kernel: both are float32 evaluations of the same cancellation-limited expression (E[x^2] - mu^2); the kernel
rounds twice (separable 11 + 11 taps) where the chain rounds once over 121 taps, and sums in another order.  The measured ratios
are in profiles/loss_error_vs_float64.txt; SEGS_LOSS_ERROR_TABLE=<file> makes a GPU run of this module write that table.

`zero_rows`: the exact-zero band of dL starts more than TEN rows from a non-zero row, not five -- dS(q)/dx(p) is non-zero for a zero
pixel p whenever the window of q (within 5 rows of p) reaches a non-zero row (within 5 rows of q); the float64 chain has 1e-6 of its
largest entry at distance 6 and exact zeros from distance 11 on (test_zero_rows_band_of_the_reference_starts_after_ten_rows).

Left out of the parametrisation (LEFT_OUT): `equal` at 1x1, lambda 0.2.  The float32 chain happens to return an exactly zero gradient
there, so e_ref = 0, max|g64| = 0 and the bar is 0; the kernel returns 8.03e-9 (3e-8 of the gradient of an unequal 1x1 pair).  Cause:
with x1 == x2 the terms of dL cancel analytically (-2 x / B2 from D11 against +2 x / B2 from D12, and the four terms of Dm), but
ssim_fwd_kernel forms them through differently rounded quotients (S / B2 against 2 A1 * fl(1 / (B1 B2))), so a rounding residue of
each stays.  From 5x5 on the chain itself leaves such a residue (e_ref 6e-11 .. 2e-9) and the kernel is within the bar."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from . import _loss_ref as R

DEV = "cuda:0"
GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "loss_reference.npz"))

SMALL = [(1, 1), (5, 5), (11, 10), (3, 70), (16, 32), (17, 33), (32, 64), (33, 65), (37, 53)]
FLIP = {(1, 16352): 16, (1, 16384): 32, (480, 1024): 16, (481, 1024): 32}      # both sides of the tile rule -> selected variant
SHIPPED = [(480, 640), (480, 752), (680, 1200), (1080, 1920)]
CASES = ([(c, H, W, 0.2) for H, W in SMALL for c in R.CLASSES]
         + [(c, H, W, lam) for lam in (0.0, 1.0) for H, W in ((33, 65), (37, 53)) for c in R.CLASSES]
         + [(c, H, W, 0.2) for H, W in FLIP for c in ("noise", "smooth")]
         + [(c, H, W, 0.2) for H, W in SHIPPED for c in ("smooth", "zero_rows")])
LEFT_OUT = {("equal", 1, 1, 0.2): "bar 0 (e_ref(dL) 0, max|g64| 0), kernel(dL) 8.031e-09: inexact cancellation of the D11 / D12 terms, see tests/test_loss_gpu.py"}
CASES = [c for c in CASES if c not in LEFT_OUT]
_ROWS = []


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _partial_bytes(lib, H, W):
    return lib.segs_l1_ssim_temp_bytes(H, W) - 3 * 3 * H * W * 4


def _run(img, gt, lam, temp_byte=0xFF):
    """One call through FusedL1SSIM with `temp` pre-filled; (out[3], dL, workgroup slots written) as numpy / int."""
    from segs_slam_amd.gaussian_trainer import FusedL1SSIM
    _, H, W = img.shape
    fused = FusedL1SSIM(H, W, DEV, lam)
    fused.temp.fill_(temp_byte)
    fused.dL.fill_(float("nan"))
    fused(img.to(DEV), gt.to(DEV))
    torch.cuda.synchronize()
    slots = fused.temp[:_partial_bytes(fused._lib, H, W)].view(torch.int64)
    fill = int.from_bytes(bytes([temp_byte]) * 8, "little", signed=True)
    return fused.out.cpu().numpy(), fused.dL.cpu().numpy(), int((slots != fill).sum())


def _ulp_distance(a, b):
    a, b = np.float32(a), np.float32(b)
    return abs(float(a) - float(b)) / float(np.spacing(max(abs(a), abs(b), np.float32(2.0 ** -126))))


# ---- the reference itself (no GPU) -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,W", [(33, 65), (48, 97), (37, 53)])
def test_float32_chain_is_close_to_float64_on_noise(H, W):
    """On noise the reference's float32 chain is within 1e-6 of the gradient's largest entry and 1e-7 on SSIM of the float64 one."""
    _, _, ref = R.case("noise", H, W)
    assert ref.e_dL <= 1e-6 * ref.gmax, (ref.e_dL, ref.gmax)
    assert ref.e_out[2] <= 1e-7, ref.e_out


@pytest.mark.parametrize("cls", ["smooth", "const"])
@pytest.mark.parametrize("H,W", [(33, 65), (48, 97)])
def test_float32_chain_loses_digits_on_smooth_inputs(cls, H, W):
    """Why the bars are relative to e_ref: on smooth or constant pairs the chain itself misses the older fixed bar (2e-5 of the
    largest entry) by cancellation in E[x^2] - mu^2."""
    _, _, ref = R.case(cls, H, W)
    assert ref.e_dL > 2e-5 * ref.gmax, (ref.e_dL, ref.gmax)


@pytest.mark.parametrize("case", sorted({k.split("_")[0] for k in GOLD.files}))
def test_helper_reproduces_reference_fixture(case):
    """tests/_loss_ref.py::loss_chain against tests/golden/loss_reference.npz (the reference's own compiled code): in float32 to the
    bars of test_python_mirror_reproduces_reference_loss, in float64 to those of the fixture's GPU test."""
    img, gt, lam = torch.from_numpy(GOLD[f"{case}_img"]), torch.from_numpy(GOLD[f"{case}_gt"]), float(GOLD[f"{case}_lambda"])
    out32, g32 = R.loss_chain(img, gt, lam, torch.float32)
    np.testing.assert_allclose(out32, GOLD[f"{case}_loss_l1_ssim"], atol=2e-7)
    np.testing.assert_allclose(g32, GOLD[f"{case}_dL_dimg"], rtol=1e-5, atol=1e-10)
    out64, g64 = R.loss_chain(img, gt, lam, torch.float64)
    np.testing.assert_allclose(out64, GOLD[f"{case}_loss_l1_ssim"], atol=2e-6)
    np.testing.assert_allclose(g64, GOLD[f"{case}_dL_dimg"], rtol=1e-4, atol=1e-9)


def test_zero_rows_band_of_the_reference_starts_after_ten_rows():
    img, gt, ref = R.case("zero_rows", 150, 40)
    lo, hi = R.zero_row_range(150)
    assert not img[:, lo:hi].any() and not gt[:, lo:hi].any() and hi - lo > 4 * R.HALO + 2
    assert np.abs(ref.g64[:, lo + R.HALO]).max() > 1e-4 * ref.gmax            # 6 rows from the last non-zero row: not zero
    assert not ref.g64[:, lo + 2 * R.HALO:hi - 2 * R.HALO].any()


def test_tile_rule_is_the_one_restated_here():
    """segs_l1_ssim_tile_rows (host only) against the rule restated in tests/_loss_ref.py, on both sides of the threshold."""
    from segs_slam_amd import _capi
    lib = _capi.lib()
    for (H, W), want in FLIP.items():
        assert R.tile_rows_rule(H, W) == want == lib.segs_l1_ssim_tile_rows(H, W), (H, W)
    for H, W in SMALL + SHIPPED + [(1079, 1920), (512, 1024), (511, 1024), (16, 16384), (33, 16352)]:
        assert lib.segs_l1_ssim_tile_rows(H, W) == R.tile_rows_rule(H, W), (H, W)
    assert lib.segs_l1_ssim_tile_rows(0, 5) == 0 == lib.segs_l1_ssim_tile_rows(5, 0)


# ---- the kernel -----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module", autouse=True)
def _error_table():
    yield
    path = os.environ.get("SEGS_LOSS_ERROR_TABLE")
    if path and _ROWS:
        with open(path, "w") as f:
            f.write("# fused L1 + SSIM (csrc/loss.hip) against the float64 chain; e_ref = the float32 chain against the same\n")
            f.write("# dL columns: max abs error over dL/dimage; ssim columns: abs error of the SSIM scalar\n")
            f.write("%-28s %6s %11s %11s %11s %8s %11s %11s %5s\n" % ("case", "lambda", "max|g64|", "e_ref(dL)", "kernel(dL)", "ratio",
                                                                 "e_ref(ssim)", "kernel(ssim)", "pass"))
            for r in _ROWS:
                f.write("%-28s %6.1f %11.3e %11.3e %11.3e %8s %11.3e %11.3e %5s\n" % r)
            for (c, H, W, lam), why in LEFT_OUT.items():
                f.write(f"# left out of the test: {c}-{H}x{W} lambda {lam:g}: {why}\n")


@pytest.mark.gpu
@pytest.mark.parametrize("cls,H,W,lam", CASES, ids=[f"{c}-{H}x{W}-l{lam:g}" for c, H, W, lam in CASES])
def test_fused_loss_against_float64(cls, H, W, lam):
    from segs_slam_amd import _capi
    img, gt, ref = R.case(cls, H, W, lam)
    out, dL, slots = _run(img, gt, lam)
    # which kernel variant ran: the rule restated, and the number of per-workgroup slots the forward kernel wrote
    ty = R.tile_rows_rule(H, W)
    assert _capi.lib().segs_l1_ssim_tile_rows(H, W) == ty == FLIP.get((H, W), ty)
    assert slots == 3 * ((W + R.TILE_W - 1) // R.TILE_W) * ((H + ty - 1) // ty)
    assert np.isfinite(dL).all() and np.isfinite(out).all()
    err = float(np.abs(dL.astype(np.float64) - ref.g64).max())
    serr = np.abs(out.astype(np.float64) - ref.out64)
    ok = err <= ref.dL_bar() and bool((serr <= ref.scalar_bars()).all())
    ratio = "%8.2f" % (err / ref.e_dL) if ref.e_dL > 0 else ("%8s" % ("0/0" if err == 0 else "inf"))
    _ROWS.append((f"{cls}-{H}x{W}", lam, ref.gmax, ref.e_dL, err, ratio, ref.e_out[2], serr[2], "yes" if ok else "NO"))
    print(f"{cls} {H}x{W} lambda={lam}: dL err {err:.3e} bar {ref.dL_bar():.3e} (e_ref {ref.e_dL:.3e}, max|g64| {ref.gmax:.3e}); "
          f"scalars err {serr} bars {ref.scalar_bars()}")
    assert err <= ref.dL_bar(), (err, ref.dL_bar(), ref.e_dL, ref.gmax)
    assert (serr <= ref.scalar_bars()).all(), (serr, ref.scalar_bars())
    # the loss word is the combination of the other two, formed in float32
    f = np.float32
    assert _ulp_distance(out[0], (f(1) - f(lam)) * out[1] + f(lam) * (f(1) - out[2])) <= 2
    if cls == "black":
        assert out.tolist() == [0.0, 0.0, 1.0] and not dL.any()
    if cls == "equal":
        assert out[1] == 0.0
    if cls == "zero_rows":
        lo, hi = R.zero_row_range(H)
        assert not dL[:, lo + 2 * R.HALO:hi - 2 * R.HALO].any()
        if hi - lo > 4 * R.HALO:
            assert np.abs(dL[:, lo + R.HALO]).max() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", SMALL)
def test_equal_images_get_nothing_from_the_l1_term(H, W):
    """image == target: l1 is exactly 0 and, sign(0) being 0, the L1 part adds nothing -- with lambda = 0 (the L1 term alone) the
    loss and every dL entry are exactly zero."""
    img, gt = R.make_pair("equal", H, W)
    out, dL, _ = _run(img, gt, 0.0)
    assert out[1] == 0.0 and out[0] == 0.0 and not dL.any()


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", [(17, 33), (37, 53), (480, 1024), (481, 1024)])
def test_scratch_contents_and_earlier_calls_do_not_matter(H, W):
    """`temp` is torch.empty and reused: 0xFF-filled or zeroed, first or second call, default stream or another -- same bits."""
    from segs_slam_amd.gaussian_trainer import FusedL1SSIM
    img, gt = (t.to(DEV) for t in R.make_pair("noise", H, W))
    img2, gt2 = (t.to(DEV) for t in R.make_pair("smooth", H, W, seed=1))
    results = {}
    for name, byte in (("ff", 0xFF), ("zero", 0x00)):
        fused = FusedL1SSIM(H, W, DEV, 0.2)
        fused.temp.fill_(byte)
        fused(img, gt)
        first = (fused.out.clone(), fused.dL.clone())
        fused(img, gt)
        again = (fused.out.clone(), fused.dL.clone())
        fused(img2, gt2)
        second = (fused.out.clone(), fused.dL.clone())
        results[name] = (first, again, second)
    fresh = FusedL1SSIM(H, W, DEV, 0.2)
    fresh.temp.zero_()
    fresh(img2, gt2)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    streamed = FusedL1SSIM(H, W, DEV, 0.2)
    with torch.cuda.stream(side):
        streamed(img, gt)
    side.synchronize()
    torch.cuda.synchronize()
    same = lambda a, b: torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))  # noqa: E731
    assert torch.isfinite(results["ff"][0][1]).all()
    assert same(results["ff"][0], results["zero"][0])              # scratch contents
    assert same(results["ff"][0], results["ff"][1])                # fixed-order reduction: two identical calls
    assert same(results["ff"][2], (fresh.out, fresh.dL)) and same(results["zero"][2], (fresh.out, fresh.dL))   # after another image
    assert same(results["ff"][0], (streamed.out, streamed.dL))     # another stream
    assert not same(results["ff"][0], results["ff"][2])


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", [(17, 33), (37, 53)])
def test_no_access_next_to_the_buffers(H, W):
    """img, gt and dL in the middle of larger allocations: NaN around the inputs changes nothing, the words around dL keep their
    pattern, and every dL entry is written (pre-filled with NaN)."""
    from segs_slam_amd import _capi
    lib = _capi.lib()
    n, pad = 3 * H * W, 1031
    img, gt = R.make_pair("noise", H, W)
    want_out, want_dL, _ = _run(img, gt, 0.2)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    bufs = []
    for src in (img, gt):
        big = torch.full((n + 2 * pad,), float("nan"), device=DEV)
        big[pad:pad + n] = src.reshape(-1).to(DEV)
        bufs.append(big)
    pattern = (torch.arange(n + 2 * pad, dtype=torch.int32, device=DEV) * 7919 + 0x3F000001)
    big_dL = pattern.clone().view(torch.float32)
    big_dL[pad:pad + n] = float("nan")
    temp = torch.full((lib.segs_l1_ssim_temp_bytes(H, W) + 2 * 4096,), 0xA5, dtype=torch.uint8, device=DEV)
    big_out = torch.full((3 + 2 * 64,), 7.25, device=DEV)
    st = lib.segs_l1_ssim_loss(_ptr(bufs[0][pad:]), _ptr(bufs[1][pad:]), H, W, 0.2, _ptr(big_out[64:]), _ptr(big_dL[pad:]),
                               _ptr(temp[4096:]), stream)
    _capi.check(st, "segs_l1_ssim_loss")
    torch.cuda.synchronize()
    got = big_dL.cpu()
    pat = pattern.cpu()
    assert torch.equal(got[:pad].view(torch.int32), pat[:pad]) and torch.equal(got[pad + n:].view(torch.int32), pat[pad + n:])
    inner = got[pad:pad + n].numpy().reshape(3, H, W)
    assert np.isfinite(inner).all()
    assert np.array_equal(inner.view(np.int32), want_dL.view(np.int32))
    assert np.array_equal(big_out[64:67].cpu().numpy().view(np.int32), want_out.view(np.int32))
    assert (big_out[:64] == 7.25).all() and (big_out[67:] == 7.25).all()
    assert (temp[:4096] == 0xA5).all() and (temp[-4096:] == 0xA5).all()


@pytest.mark.gpu
def test_bad_arguments_are_refused_and_touch_nothing():
    from segs_slam_amd import _capi
    lib = _capi.lib()
    H, W = 17, 33
    img, gt = (t.to(DEV) for t in R.make_pair("noise", H, W))
    dL = torch.full((3, H, W), 3.5, device=DEV)
    out = torch.full((3,), 3.5, device=DEV)
    temp = torch.zeros(lib.segs_l1_ssim_temp_bytes(H, W), dtype=torch.uint8, device=DEV)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for args in ((_ptr(img), _ptr(gt), 0, W), (_ptr(img), _ptr(gt), H, 0), (_ptr(img), _ptr(gt), -1, W), (None, _ptr(gt), H, W),
                 (_ptr(img), None, H, W)):
        assert lib.segs_l1_ssim_loss(*args, 0.2, _ptr(out), _ptr(dL), _ptr(temp), stream) == -1      # SEGS_ERR_INVALID_ARGUMENT
    for o, d, t in ((None, dL, temp), (out, None, temp), (out, dL, None)):
        assert lib.segs_l1_ssim_loss(_ptr(img), _ptr(gt), H, W, 0.2, _ptr(o), _ptr(d), _ptr(t), stream) == -1
    torch.cuda.synchronize()
    assert (dL == 3.5).all() and (out == 3.5).all() and not temp.any()
