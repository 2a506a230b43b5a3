"""Shared by tests/test_eval_metrics_cpu.py and tests/test_eval_metrics_gpu.py: the float64 reference of the keyframe metrics
(include/segs_eval.h), the float32 yardstick, the inputs, the bars, and the NumPy restatement of the byte conversion.

Reference: the chain of GaussianMapper::renderAndRecordKeyframe (src/gaussian_mapper.cpp:1811-1818) -- mask_rgb = (gt != 0).any(-1)
of the CHW target, both images multiplied by it, then segs_slam_amd.loss_utils.ssim / psnr / psnr_gaussian_splatting (the mirrors of
include/loss_utils.h) -- on CPU tensors cast to float64, the way tests/_loss_ref.loss_chain does it.  The SAME chain in float32 is
the yardstick e: how far the reference's own op chain is from float64 on that input."""
import functools

import numpy as np
import torch

from tests import _loss_ref

COLUMNS = ("ssim", "psnr", "psnr_gs", "mse", "mse_r", "mse_g", "mse_b", "l1")
CLASSES = ("noise", "smooth", "const", "equal", "black", "out_of_range", "impulse", "masked")
SMALL_SHAPES = [(1, 1), (5, 7), (17, 33), (33, 65), (37, 53), (48, 97)]     # (H, W)
TY32_SHAPE = (481, 1024)          # the smallest camera-like size with 32-row tiles
U = 2.0 ** -24
# segs_eval.h: the longest chain of float32 additions from a term to a sum over the three channels is 28 (<= 32, the issue's figure)
SUM_CHAIN = 32


def masked_rows(H):
    """(band lo, band hi, row whose target is zero except at x = W - 1 [channel 0], row zero except at x = 0 [channel 2])."""
    return H // 3, H // 2, (2 * H) // 3, H - 1


def make_pair(cls, H, W, seed=0):
    """(image, target), float32 CPU (3, H, W).  The classes of tests/_loss_ref.make_pair, and `masked`: a noise pair whose target
    has rows H//3:H//2 zeroed in channel 1 only, one row that is zero except at x = W - 1 and one that is zero except at x = 0,
    while the image is non-zero everywhere."""
    if cls != "masked":
        return _loss_ref.make_pair(cls, H, W, seed)
    img, gt = _loss_ref.make_pair("noise", H, W, seed)
    img = (0.05 + 0.9 * img).contiguous()
    gt = gt.clone()
    lo, hi, ra, rb = masked_rows(H)
    gt[1, lo:hi] = 0.0
    gt[0, ra] = 0.0
    gt[0, ra, W - 1] = 0.5
    gt[2, rb] = 0.0
    gt[2, rb, 0] = 0.25
    assert bool((img != 0).all())
    return img, gt.contiguous()


def row_flags(gt):
    """The per-(channel, row) mask, (3, H) bool: exactly (gt != 0).any(-1)."""
    return (gt != 0).any(-1)


def chain(img, gt, row_mask, dtype):
    """The reference chain in `dtype` on the CPU -> the eight numbers of a table row as float64 (COLUMNS)."""
    from segs_slam_amd import loss_utils
    x, t = img.detach().to("cpu", dtype), gt.detach().to("cpu", dtype)
    if row_mask:
        m = row_flags(t).to(dtype).unsqueeze(-1)
        x, t = x * m, t * m
    sq = torch.pow(x - t, 2)
    mse_c = sq.view(3, -1).mean(1)
    out = [loss_utils.ssim(x, t), loss_utils.psnr(x, t), loss_utils.psnr_gaussian_splatting(x, t), sq.mean(), mse_c[0], mse_c[1],
           mse_c[2], loss_utils.l1_loss(x, t)]
    return np.array([float(v) for v in out], dtype=np.float64)


class Reference:
    """out64: the float64 chain; e: |float32 chain - float64 chain| (inf where the two disagree about being finite)."""

    def __init__(self, img, gt, row_mask):
        self.out64 = chain(img, gt, row_mask, torch.float64)
        self.out32 = chain(img, gt, row_mask, torch.float32)
        with np.errstate(invalid="ignore"):
            e = np.abs(self.out32 - self.out64)
        self.e = np.where(self.out32 == self.out64, 0.0, e)          # (inf - inf)
        self.out64.setflags(write=False)

    def rel_bar(self, k):
        """Relative bar of a sum column (mse, mse_c, l1): 4 e_rel + SUM_CHAIN * 2^-24."""
        v = abs(self.out64[k])
        return 4.0 * (self.e[k] / v if v > 0 else 0.0) + SUM_CHAIN * U

    def bars(self):
        """Absolute bars of the eight columns.  ssim: tests/_loss_ref.Reference.scalar_bars.  mse, mse_c, l1: rel_bar * |value|.
        psnr, psnr_gs (dB): 4.35 * (the relative bar of their mean squared errors) + 4 * 2^-24 * |value|; a value that is +inf
        in float64 must be exactly +inf (bar 0)."""
        b = np.zeros(8)
        b[0] = 4.0 * self.e[0] + 2e-6
        for k in (3, 4, 5, 6, 7):
            b[k] = self.rel_bar(k) * abs(self.out64[k])
        for k, rel in ((1, self.rel_bar(3)), (2, max(self.rel_bar(c) for c in (4, 5, 6)))):
            b[k] = 4.35 * rel + 4.0 * U * abs(self.out64[k]) if np.isfinite(self.out64[k]) else 0.0
        return b

    def misses(self, row):
        """Columns of `row` (eight numbers) outside the bars: [(name, got, want, bar)]; empty = inside."""
        row = np.asarray(row, dtype=np.float64)
        bars = self.bars()
        bad = []
        for k, name in enumerate(COLUMNS):
            want = self.out64[k]
            ok = (row[k] == want) if not np.isfinite(want) else (np.isfinite(row[k]) and abs(row[k] - want) <= bars[k])
            if not ok:
                bad.append((name, float(row[k]), float(want), float(bars[k])))
        return bad

    def ratio(self, row):
        """max over the finite columns of |row - out64| / bar."""
        row = np.asarray(row, dtype=np.float64)
        bars = self.bars()
        fin = np.isfinite(self.out64) & (bars > 0)
        return float(np.max(np.abs(row[fin] - self.out64[fin]) / bars[fin])) if fin.any() else 0.0


def _case(cls, H, W, row_mask, seed):
    img, gt = make_pair(cls, H, W, seed)
    return img, gt, Reference(img, gt, row_mask)


_cached_case = functools.lru_cache(maxsize=None)(_case)


def case(cls, H, W, row_mask, seed=0):
    """(image, target, Reference); the small ones are computed once per session and shared."""
    return (_cached_case if H * W <= 64 * 1024 else _case)(cls, H, W, bool(row_mask), seed)


# ---- recorded images -----------------------------------------------------------------------------------------------------------
def to_bytes(v):
    """segs_eval.h, THE BYTES, restated in NumPy float32: p = v * 255.0f; r = rint(p) (ties to even); 0 for a NaN or r <= 0,
    255 for r >= 255."""
    v = np.asarray(v, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.rint(v * np.float32(255.0))
    r = np.where(np.isnan(r), np.float32(0.0), r)
    return np.clip(r, 0.0, 255.0).astype(np.uint8)


def images(img, gt, row_mask):
    """{"image", "gt", "loss"}: uint8 (H, W, 3) RGB arrays of the masked render, the masked target and |their difference|, every
    product and the difference in float32."""
    x, t = img.detach().cpu().numpy().astype(np.float32), gt.detach().cpu().numpy().astype(np.float32)
    if row_mask:
        m = (t != 0).any(-1).astype(np.float32)[..., None]
        with np.errstate(invalid="ignore"):
            x, t = x * m, t * m
    with np.errstate(invalid="ignore"):
        d = np.abs(x - t)
    hwc = lambda a: np.ascontiguousarray(np.transpose(to_bytes(a), (1, 2, 0)))  # noqa: E731
    return {"image": hwc(x), "gt": hwc(t), "loss": hwc(d)}
