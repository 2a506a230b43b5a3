"""NumPy restatement of the stereo matcher's specification (stages 1-8), written from that text and independent of
the kernels: integer arithmetic in int64, one function per stage, loops over image lines only (vectorised over the rest).

    st = sgm(left_u8, right_u8, D=64, dmin=0, P1=10, P2=120, u=5, paths=4, lr_max_diff=1, median=True, fb16=None)
    st["census_left"], st["census_right"], st["S"], st["raw_winner"], st["raw_median"], st["disp_right"], st["disp16"], st["depth"]
"""
import numpy as np

INVALID = 0xFFFF
FAR = 1 << 40


def rgb_to_gray_u8(rgb):
    """Stage 1: (3, H, W) float32 -> (H, W) uint8; every operation in float32, in the stated order."""
    rgb = np.asarray(rgb, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        g = (np.float32(0.299) * rgb[0] + np.float32(0.587) * rgb[1]) + np.float32(0.114) * rgb[2]
        q = np.rint(g * np.float32(255.0))                      # half to even, like rintf
    q = np.where(np.isnan(q), np.float32(0.0), q)
    return np.minimum(np.maximum(q, np.float32(0.0)), np.float32(255.0)).astype(np.uint8)


CENSUS_OFFSETS = [(dy, dx) for dy in (-3, -2, -1) for dx in range(-4, 5)] + [(0, dx) for dx in range(-4, 0)]


def census(img):
    """Stage 2: centre-symmetric 9 x 7 census, 31 bits; 0 on the border and for an image smaller than the window."""
    img = np.asarray(img).astype(np.int64)
    H, W = img.shape
    out = np.zeros((H, W), dtype=np.uint32)
    if H < 7 or W < 9:
        return out
    assert len(CENSUS_OFFSETS) == 31
    for bit, (dy, dx) in enumerate(CENSUS_OFFSETS):
        a = img[3 + dy:H - 3 + dy, 4 + dx:W - 4 + dx]
        b = img[3 - dy:H - 3 - dy, 4 - dx:W - 4 - dx]
        out[3:H - 3, 4:W - 4] |= (a > b).astype(np.uint32) << np.uint32(bit)
    return out


def _popcount(x):
    return np.unpackbits(np.ascontiguousarray(x).view(np.uint8).reshape(x.shape + (4,)), axis=-1).sum(-1).astype(np.int64)


def cost_volume(cl, cr, D, dmin):
    """Stage 3: C(x, y, d) = popcount(cl(x, y) ^ cr(x - d - dmin, y)); cr reads as 0 left of the image."""
    H, W = cl.shape
    C = np.zeros((H, W, D), dtype=np.int64)
    for d in range(D):
        s = d + dmin
        r = np.zeros_like(cr)
        if s < W:
            r[:, s:] = cr[:, :W - s]
        C[:, :, d] = _popcount(cl ^ r)
    return C


def _step(prev, P1, P2):
    """min(L(d), L(d-1) + P1, L(d+1) + P1, m + P2) - m along the last axis; d +- 1 outside [0, D) left out."""
    m = prev.min(axis=-1, keepdims=True)
    lo = np.full_like(prev, FAR)
    hi = np.full_like(prev, FAR)
    lo[..., 1:] = prev[..., :-1] + P1
    hi[..., :-1] = prev[..., 1:] + P1
    return np.minimum(np.minimum(prev, m + P2), np.minimum(lo, hi)) - m


def aggregate(C, dx, dy, P1, P2):
    """Stage 4, one direction r = (dx, dy): L_r(p) = C(p) where p - r lies outside the image, else C(p) + step(L_r(p - r))."""
    H, W, D = C.shape
    L = np.zeros_like(C)
    if dy == 0:
        xs = range(W) if dx > 0 else range(W - 1, -1, -1)
        for x in xs:
            px = x - dx
            L[:, x] = C[:, x] + (_step(L[:, px], P1, P2) if 0 <= px < W else 0)
        return L
    ys = range(H) if dy > 0 else range(H - 1, -1, -1)
    for y in ys:
        py = y - dy
        if not 0 <= py < H:
            L[y] = C[y]
            continue
        add = _step(L[py], P1, P2)                               # indexed by the predecessor's column
        cur = C[y].copy()
        if dx == 0:
            cur += add
        elif dx > 0:
            cur[1:] += add[:-1]                                  # column 0 has no predecessor
        else:
            cur[:-1] += add[1:]                                  # column W - 1 has none
        L[y] = cur
    return L


DIRECTIONS = [(1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, -1), (1, -1), (-1, 1)]


def floor_frac(num, den):
    """Stage 5's sub-pixel offset: floor((16 num + den) / (2 den)) for den > 0, else 0 (mathematical floor)."""
    num, den = np.asarray(num, dtype=np.int64), np.asarray(den, dtype=np.int64)
    safe = np.where(den > 0, den, 1)
    return np.where(den > 0, np.floor_divide(16 * num + safe, 2 * safe), 0)


def winner(S, u):
    """Stage 5: raw = 16 d* + frac (uint16), 0xFFFF where the uniqueness test fails."""
    H, W, D = S.shape
    best = S.argmin(axis=-1)                                     # the lowest d on ties
    sbest = np.take_along_axis(S, best[..., None], -1)[..., 0]
    d = np.arange(D)[None, None, :]
    invalid = np.zeros((H, W), dtype=bool)
    if u > 0:
        far = np.abs(d - best[..., None]) > 1
        invalid = (far & (S * (100 - u) < sbest[..., None] * 100)).any(-1)
    inner = (best > 0) & (best < D - 1)
    lo = np.take_along_axis(S, np.clip(best - 1, 0, D - 1)[..., None], -1)[..., 0]
    hi = np.take_along_axis(S, np.clip(best + 1, 0, D - 1)[..., None], -1)[..., 0]
    frac = np.where(inner, floor_frac(lo - hi, lo - 2 * sbest + hi), 0)
    raw = 16 * best + frac
    return np.where(invalid, INVALID, raw).astype(np.uint16)


def median3x3(raw):
    """Stage 6: the 5th smallest of the 3 x 3 values (0xFFFF ordered as a number); the border keeps its value."""
    H, W = raw.shape
    out = raw.copy()
    if H < 3 or W < 3:
        return out
    stack = np.stack([raw[1 + dy:H - 1 + dy, 1 + dx:W - 1 + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1)], axis=-1)
    out[1:-1, 1:-1] = np.sort(stack, axis=-1)[..., 4]
    return out


def right_view(S, dmin):
    """Stage 7a: d_r(xr, y) = argmin over d with xr + d + dmin < W of S(xr + d + dmin, y, d); lowest d on ties; -1 if none."""
    H, W, D = S.shape
    cand = np.full((H, W, D), FAR, dtype=np.int64)
    for d in range(D):
        s = d + dmin
        if s < W:
            cand[:, :W - s, d] = S[:, s:, d]
    dr = cand.argmin(-1)
    return np.where(cand.min(-1) == FAR, -1, dr).astype(np.int16)


def check_and_output(raw, dr, dmin, lr_max_diff, fb16=None):
    """Stages 7b and 8."""
    H, W = raw.shape
    v = raw.astype(np.int64)
    valid = v != INVALID
    dl = (v + 8) >> 4
    xr = np.arange(W)[None, :] - dl - dmin
    valid &= xr >= 0
    if lr_max_diff >= 0:
        other = np.take_along_axis(dr.astype(np.int64), np.clip(xr, 0, W - 1), axis=1)
        valid &= np.abs(dl - other) <= lr_max_diff
    disp16 = np.where(valid, v + 16 * dmin, 16 * (dmin - 1)).astype(np.int16)
    depth = None
    if fb16 is not None:
        ok = valid & (disp16 > 0)
        depth = np.zeros((H, W), dtype=np.float32)
        depth[ok] = np.float32(fb16) / disp16[ok].astype(np.float32)
    return disp16, depth


def fb16_of(fx, baseline):
    """16 fx baseline, formed in float64 and passed as one float32."""
    return np.float32(16.0 * float(fx) * float(baseline))


def sgm(left, right, D=64, dmin=0, P1=10, P2=120, u=5, paths=4, lr_max_diff=1, median=True, fb16=None):
    left, right = np.asarray(left, dtype=np.uint8), np.asarray(right, dtype=np.uint8)
    assert left.shape == right.shape and left.ndim == 2
    cl, cr = census(left), census(right)
    C = cost_volume(cl, cr, D, dmin)
    S = np.zeros_like(C)
    for dx, dy in DIRECTIONS[:paths]:
        S += aggregate(C, dx, dy, P1, P2)
    assert S.max() <= paths * 255
    raw5 = winner(S, u)
    raw6 = median3x3(raw5) if median else raw5.copy()
    dr = right_view(S, dmin)
    disp16, depth = check_and_output(raw6, dr, dmin, lr_max_diff, fb16)
    return {"census_left": cl, "census_right": cr, "S": S.astype(np.uint16), "raw_winner": raw5, "raw_median": raw6,
            "disp_right": dr, "disp16": disp16, "depth": depth}


# ---------------------------------------------------------------- inputs shared by the CPU and GPU tests
def shifted_pair(H=40, W=160, d_top=7, d_bottom=19, seed=7):
    """Left: iid uniform bytes.  right[y, x] = left[y, x + d_t], d_t = d_top in the top half and d_bottom below; the uncovered
    right edge is fresh noise.  Returns (left, right, truth) with truth the (H, W) disparity in pixels."""
    rng = np.random.default_rng(seed)
    left = rng.integers(0, 256, (H, W), dtype=np.uint8)
    truth = np.where(np.arange(H)[:, None] < H // 2, d_top, d_bottom) * np.ones((1, W), dtype=np.int64)
    right = np.zeros((H, W), dtype=np.uint8)
    for y in range(H):
        d = int(truth[y, 0])
        right[y, :W - d] = left[y, d:]
        right[y, W - d:] = rng.integers(0, 256, d, dtype=np.uint8)
    return left, right, truth
