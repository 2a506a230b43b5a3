"""Two references for the frame intake (include/segs_frame_intake.h), neither of them the code under test.

 (a) `*_f32`: a NumPy float32 restatement of the header's operation sequence for the map, the sampler and the resize.  The GPU
     kernels must give its bytes.
 (b) `*_f64`: an independent float64 chain: the map in float64 NumPy from the float64 calibration values (R^-1 included), sampling
     by scipy.ndimage.map_coordinates(order=1, mode="constant", cval=0), the resize by torch.nn.functional.interpolate(
     mode="bilinear", align_corners=False) on the CPU in float64.  scipy's "constant" mode returns cval for every coordinate
     outside [0, n-1] instead of blending with the border, so the source is first padded by one pixel of zeros on each side and
     the coordinates shifted by one: that is cv::remap's constant border, which blends the edge pixel with 0 over (-1, 0).

The map's float32 error, measured as max (|mx_a - mx_b| + |my_a - my_b|) over the pixels whose float64 coordinate reaches the source
(tests/test_frame_intake_cpu.py measures it over every camera below), came to 3.38 units of 2^-24 max(in_w, in_h) pixels (worst: the scaled TUM camera at 67x5; 3.31 at the real 640x480); the
tolerance is twice that: TOL_UNITS = 6.76, i.e. tol_px = 6.76 * 2^-24 * max(in_w, in_h) (2.6e-4 px at 640x480).  The margin is for
inputs not listed.  The count explains it: a coordinate of size max(in_w, in_h) carries half a unit for each of its last roundings
(fx xd, + cx) and the roundings of xd's dozen operations scaled by fx, a few units per axis.
"""
import functools
import json
import os
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
TOL_UNITS = 6.76


def tol_px(in_w: int, in_h: int) -> float:
    return TOL_UNITS * 2.0 ** -24 * max(in_w, in_h)


# ---------------------------------------------------------------------------------------------------------------- cameras
@dataclass(frozen=True)
class Cam:
    """Float64 calibration values, as a calibration file gives them."""
    name: str
    in_w: int
    in_h: int
    out_w: int
    out_h: int
    K: Tuple[float, float, float, float]                 # fx, fy, cx, cy
    dist: Tuple[float, float, float, float, float]       # k1, k2, p1, p2, k3
    R: Optional[Tuple[Tuple[float, ...], ...]]           # rectifying rotation or None
    newK: Tuple[float, float, float, float]
    all_borders: bool = False                            # the map must leave the source through all four borders

    def rinv64(self) -> np.ndarray:
        return np.eye(3) if self.R is None else np.linalg.inv(np.asarray(self.R, dtype=np.float64))

    def model_kwargs(self) -> dict:
        """Keyword arguments of segs_slam_amd.frame_intake.CameraModel for the same camera."""
        kw = dict(width=self.in_w, height=self.in_h, fx=self.K[0], fy=self.K[1], cx=self.K[2], cy=self.K[3])
        kw.update(zip(("k1", "k2", "p1", "p2", "k3"), self.dist))
        kw.update(R=None if self.R is None else [list(r) for r in self.R], new_fx=self.newK[0], new_fy=self.newK[1], new_cx=self.newK[2],
                  new_cy=self.newK[3], new_width=self.out_w, new_height=self.out_h)
        return kw


def rotation(axis, degrees: float):
    """Rodrigues' formula in float64."""
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    t = np.deg2rad(degrees)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + np.sin(t) * Kx + (1 - np.cos(t)) * (Kx @ Kx)
    return tuple(tuple(float(v) for v in row) for row in R)


@functools.lru_cache(maxsize=None)
def settings():
    with open(os.path.join(ROOT, "tests", "golden", "orbslam_camera_values.json")) as f:
        return json.load(f)


TUM = "cfg/ORB_SLAM3/RGB-D/TUM/tum_freiburg2_xyz.yaml"
# (in_w, in_h, out_w, out_h): a resized new camera; one row and one column; one full wave row of four workgroup columns; odd sizes
SHAPES = ((37, 29, 41, 23), (64, 1, 64, 1), (1, 64, 1, 64), (256, 4, 256, 4), (67, 5, 67, 5))


def tum_scaled(in_w, in_h, out_w, out_h) -> Cam:
    """TUM freiburg2's coefficients with its intrinsics scaled to the small size (the focal lengths by the longer side, so that the
    distortion acts over the whole of it), a 5 degree rotation about an oblique axis and a new camera that looks 25 % wider: the
    output sees past the source on every side."""
    s = settings()[TUM]
    f = max(in_w, in_h) / 640.0
    K = (s["Camera1.fx"] * f, s["Camera1.fy"] * f, s["Camera1.cx"] * in_w / 640.0, s["Camera1.cy"] * in_h / 480.0)
    dist = tuple(s["Camera1." + k] for k in ("k1", "k2", "p1", "p2", "k3"))
    g = 0.75 * min(out_w / in_w, out_h / in_h)
    newK = (K[0] * g, K[1] * g, (out_w - 1) / 2.0 + 0.3, (out_h - 1) / 2.0 - 0.2)
    return Cam(f"tum-{in_w}x{in_h}-{out_w}x{out_h}", in_w, in_h, out_w, out_h, K, dist, rotation(_axis(in_w, in_h, (1.0, -2.0, 0.5)), 5.0),
               newK, all_borders=min(in_w, in_h) >= 16)


def _axis(in_w, in_h, oblique):
    """The rotation axis: oblique for an image with two real dimensions; for a strip of a few rows (columns) nearly the axis that
    moves the image along the strip, tilted just enough that the short coordinate gets a fraction of a pixel, or the whole strip
    would map outside the source."""
    if in_w >= 8 * in_h:
        return (0.01, 1.0, 0.004)
    if in_h >= 8 * in_w:
        return (1.0, 0.01, 0.004)
    return oblique


def rotated(in_w, in_h, out_w, out_h) -> Cam:
    f = 0.9 * max(in_w, in_h)
    K = (f, f * 1.01, in_w / 2.0 - 0.37, in_h / 2.0 + 0.21)
    newK = (K[0] * out_w / in_w, K[1] * out_h / in_h, K[2] * out_w / in_w, K[3] * out_h / in_h)
    return Cam(f"rot-{in_w}x{in_h}-{out_w}x{out_h}", in_w, in_h, out_w, out_h, K, (0.0,) * 5,
               rotation(_axis(in_w, in_h, (0.3, 1.0, -0.4)), 3.0), newK)


def identity(w, h) -> Cam:
    """Every float32 step of the map is exact: fx = fy = 64, centres multiples of 0.5, no distortion, no rotation, same size."""
    K = (64.0, 64.0, (w - 1) / 2.0, (h - 1) / 2.0)
    return Cam(f"identity-{w}x{h}", w, h, w, h, K, (0.0,) * 5, None, K)


def tum_full() -> Cam:
    s = settings()[TUM]
    K = tuple(s["Camera1." + k] for k in ("fx", "fy", "cx", "cy"))
    dist = tuple(s["Camera1." + k] for k in ("k1", "k2", "p1", "p2", "k3"))
    return Cam("tum-640x480", int(s["Camera.width"]), int(s["Camera.height"]), int(s["Camera.width"]), int(s["Camera.height"]), K, dist, None, K)


@functools.lru_cache(maxsize=None)
def small_cameras():
    cams = []
    for sh in SHAPES:
        cams += [tum_scaled(*sh), rotated(*sh), identity(sh[0], sh[1])]
    return tuple(cams)


@functools.lru_cache(maxsize=None)
def all_cameras():
    return small_cameras() + (tum_full(),)


def camera(name: str) -> Cam:
    return {c.name: c for c in all_cameras()}[name]


# ---------------------------------------------------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def frame_u8(in_w: int, in_h: int, channels: int = 3, seed: int = 0) -> np.ndarray:
    """(in_h, in_w, C) uint8: smooth structure plus noise, every byte value possible."""
    rng = np.random.default_rng(1000 * in_w + in_h + 7 * channels + seed)
    y, x = np.mgrid[0:in_h, 0:in_w]
    base = 127.5 + 90.0 * np.sin(0.31 * x + 0.17 * y)[..., None] * np.cos(0.05 * x[..., None] * np.arange(1, channels + 1))
    img = np.clip(base + rng.normal(0, 40, (in_h, in_w, channels)), 0, 255).astype(np.uint8)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def depth_u16(in_w: int, in_h: int, seed: int = 0) -> np.ndarray:
    """(in_h, in_w) uint16: a slanted plane with noise between 0.4 and 9 m at 5000 units per metre (values past 32767 included), with
    rectangular holes of raw 0 over about a tenth of it and a few single-pixel holes."""
    rng = np.random.default_rng(77 * in_w + in_h + seed)
    y, x = np.mgrid[0:in_h, 0:in_w]
    z = 2000 + 43000 * (x + 2 * y) / max(in_w + 2 * in_h, 1) + rng.integers(0, 300, (in_h, in_w))
    z = z.astype(np.uint16)
    for _ in range(3):
        w, h = max(in_w // 5, 1), max(in_h // 5, 1)
        x0, y0 = int(rng.integers(0, in_w)), int(rng.integers(0, in_h))
        z[y0:y0 + h, x0:x0 + w] = 0
    z[rng.random((in_h, in_w)) < 0.01] = 0
    z.setflags(write=False)
    return z


INV_FACTOR = float(np.float32(1.0 / 5000.0))


# ---------------------------------------------------------------------------------------------------------------- (a) float32
def map_f32(c: Cam):
    """(mx, my), each (out_h, out_w) float32: the header's sequence, every intermediate a float32."""
    fx, fy, cx, cy = (F(v) for v in c.K)
    k1, k2, p1, p2, k3 = (F(v) for v in c.dist)
    nfx, nfy, ncx, ncy = (F(v) for v in c.newK)
    r = c.rinv64().astype(F).reshape(9)
    v, u = np.mgrid[0:c.out_h, 0:c.out_w]
    u, v = u.astype(F), v.astype(F)
    with np.errstate(all="ignore"):
        x = (u - ncx) / nfx
        y = (v - ncy) / nfy
        X = (r[0] * x + r[1] * y) + r[2]
        Y = (r[3] * x + r[4] * y) + r[5]
        Wc = (r[6] * x + r[7] * y) + r[8]
        x1, y1 = X / Wc, Y / Wc
        x2, y2 = x1 * x1, y1 * y1
        r2 = x2 + y2
        xy2 = (F(2) * x1) * y1
        kr = F(1) + r2 * (k1 + r2 * (k2 + r2 * k3))
        xd = (x1 * kr + p1 * xy2) + p2 * (r2 + F(2) * x2)
        yd = (y1 * kr + p1 * (r2 + F(2) * y2)) + p2 * xy2
        mx = fx * xd + cx
        my = fy * yd + cy
    assert mx.dtype == F and my.dtype == F
    return mx, my


@dataclass
class Taps32:
    reach: np.ndarray
    idx: tuple          # four (yy, xx) index pairs, clipped into the source
    inside: tuple       # four boolean maps
    w: tuple            # four float32 weight maps


def taps_f32(mx, my, in_w, in_h) -> Taps32:
    with np.errstate(invalid="ignore"):
        reach = (mx > F(-1)) & (mx < F(in_w)) & (my > F(-1)) & (my < F(in_h))
    sx, sy = np.where(reach, mx, F(0)), np.where(reach, my, F(0))
    fx0, fy0 = np.floor(sx), np.floor(sy)
    ax, ay = sx - fx0, sy - fy0
    bx, by = F(1) - ax, F(1) - ay
    x0, y0 = fx0.astype(np.int64), fy0.astype(np.int64)
    w = (bx * by, ax * by, bx * ay, ax * ay)
    idx, inside = [], []
    for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
        xx, yy = x0 + dx, y0 + dy
        inside.append(reach & (xx >= 0) & (xx < in_w) & (yy >= 0) & (yy < in_h))
        idx.append((np.clip(yy, 0, in_h - 1), np.clip(xx, 0, in_w - 1)))
    assert all(a.dtype == F for a in w)
    return Taps32(reach, tuple(idx), tuple(inside), w)


def _sum_f32(t: Taps32, vals):
    s = ((vals[0] * t.w[0] + vals[1] * t.w[1]) + vals[2] * t.w[2]) + vals[3] * t.w[3]
    assert s.dtype == F
    return np.where(t.reach, s, F(0))


def _gather(t: Taps32, plane: np.ndarray):
    return [np.where(t.inside[k], plane[t.idx[k]].astype(F), F(0)) for k in range(4)]


def to_byte_f32(v: np.ndarray) -> np.ndarray:
    with np.errstate(invalid="ignore"):
        q = np.rint(v * F(255))                       # nearest, ties to even
        q = np.where(np.isnan(q), F(0), q)
    return np.clip(q, 0, 255).astype(np.uint8)


def image_f32(c: Cam, src: np.ndarray):
    """src (in_h, in_w, C) uint8 -> (image (C, out_h, out_w) float32, grey (out_h, out_w) uint8)."""
    t = taps_f32(*map_f32(c), c.in_w, c.in_h)
    out = np.stack([_sum_f32(t, _gather(t, src[..., ch])) / F(255) for ch in range(src.shape[2])])
    assert out.dtype == F
    if src.shape[2] == 3:
        g = (F(0.299) * out[0] + F(0.587) * out[1]) + F(0.114) * out[2]
    else:
        g = out[0]
    return out, to_byte_f32(g)


def mask_f32(c: Cam) -> np.ndarray:
    t = taps_f32(*map_f32(c), c.in_w, c.in_h)
    return _sum_f32(t, [t.inside[k].astype(F) for k in range(4)])


def depth_f32(c: Cam, raw: np.ndarray, inv_factor: float, hole_aware: bool) -> np.ndarray:
    t = taps_f32(*map_f32(c), c.in_w, c.in_h)
    r = _gather(t, raw)
    s = _sum_f32(t, [v * F(inv_factor) for v in r])
    if hole_aware:
        hole = np.zeros(s.shape, dtype=bool)
        for k in range(4):
            hole |= (t.w[k] != 0) & ~(r[k] > 0)
        s = np.where(hole, F(0), s)
    return s


def resize_f32(img: np.ndarray, w: int, h: int) -> np.ndarray:
    """img (C, H, W) float32 -> (C, h, w) float32."""
    assert img.dtype == F
    _, H, W = img.shape

    def axis(n_out, n_in):
        s = (np.arange(n_out, dtype=F) + F(0.5)) * (F(n_in) / F(n_out)) - F(0.5)
        f0 = np.floor(s)
        a = s - f0
        i0 = f0.astype(np.int64)
        return np.clip(i0, 0, n_in - 1), np.clip(i0 + 1, 0, n_in - 1), a, F(1) - a

    xa, xb, ax, bx = axis(w, W)
    ya, yb, ay, by = axis(h, H)
    ax, bx, ay, by = ax[None, :], bx[None, :], ay[:, None], by[:, None]
    w00, w01, w10, w11 = bx * by, ax * by, bx * ay, ax * ay
    out = []
    for p in img:
        t00, t01, t10, t11 = p[np.ix_(ya, xa)], p[np.ix_(ya, xb)], p[np.ix_(yb, xa)], p[np.ix_(yb, xb)]
        out.append(((t00 * w00 + t01 * w01) + t10 * w10) + t11 * w11)
    out = np.stack(out)
    assert out.dtype == F
    return out


# ---------------------------------------------------------------------------------------------------------------- (b) float64
def map_f64(c: Cam):
    fx, fy, cx, cy = c.K
    k1, k2, p1, p2, k3 = c.dist
    nfx, nfy, ncx, ncy = c.newK
    v, u = np.mgrid[0:c.out_h, 0:c.out_w].astype(np.float64)
    ray = np.einsum("ij,jhw->ihw", c.rinv64(), np.stack([(u - ncx) / nfx, (v - ncy) / nfy, np.ones_like(u)]))
    with np.errstate(all="ignore"):
        x, y = ray[0] / ray[2], ray[1] / ray[2]
        r2 = x * x + y * y
        radial = 1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3
        xd = x * radial + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
        yd = y * radial + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    return fx * xd + cx, fy * yd + cy


def remap_f64(plane: np.ndarray, mx: np.ndarray, my: np.ndarray) -> np.ndarray:
    from scipy.ndimage import map_coordinates
    padded = np.pad(plane.astype(np.float64), 1)
    ok = np.isfinite(mx) & np.isfinite(my)
    coords = np.stack([np.where(ok, my, -10.0) + 1.0, np.where(ok, mx, -10.0) + 1.0])
    return map_coordinates(padded, coords, order=1, mode="constant", cval=0.0)


def image_f64(c: Cam, src: np.ndarray) -> np.ndarray:
    mx, my = map_f64(c)
    return np.stack([remap_f64(src[..., ch], mx, my) for ch in range(src.shape[2])]) / 255.0


def mask_f64(c: Cam) -> np.ndarray:
    return remap_f64(np.ones((c.in_h, c.in_w)), *map_f64(c))


def depth_f64(c: Cam, raw: np.ndarray, inv_factor: float, hole_aware: bool) -> np.ndarray:
    mx, my = map_f64(c)
    z = remap_f64(raw.astype(np.float64) * inv_factor, mx, my)
    if hole_aware:
        # the remap of the hole indicator (1 at a hole, 1 outside the source) is positive exactly where a tap of non-zero weight is a hole
        holes = np.pad((~(raw > 0)).astype(np.float64), 1, constant_values=1.0)
        from scipy.ndimage import map_coordinates
        ok = np.isfinite(mx) & np.isfinite(my)
        coords = np.stack([np.where(ok, my, -10.0) + 1.0, np.where(ok, mx, -10.0) + 1.0])
        touched = map_coordinates(holes, coords, order=1, mode="constant", cval=1.0)
        z = np.where(touched > 0, 0.0, z)
    return z


def resize_f64(img: np.ndarray, w: int, h: int) -> np.ndarray:
    import torch
    t = torch.from_numpy(np.ascontiguousarray(img, dtype=np.float64))[None]
    return torch.nn.functional.interpolate(t, size=(h, w), mode="bilinear", align_corners=False)[0].numpy()


# ---------------------------------------------------------------------------------------------------------------- bounds
def reaches(c: Cam, mx64, my64, margin: float = 0.0):
    with np.errstate(invalid="ignore"):
        return (mx64 > -1 - margin) & (mx64 < c.in_w + margin) & (my64 > -1 - margin) & (my64 < c.in_h + margin)


def map_error_px(c: Cam) -> float:
    """max (|dmx| + |dmy|) between (a) and (b) over the pixels whose float64 coordinate lies within a pixel of reaching the source
    (further out every tap is outside for both and the coordinate has no effect)."""
    (ax, ay), (bx, by) = map_f32(c), map_f64(c)
    sel = reaches(c, bx, by, 1.0)
    if not sel.any():
        return 0.0
    return float((np.abs(ax.astype(np.float64) - bx) + np.abs(ay.astype(np.float64) - by))[sel].max())


def near_grid_line(c: Cam, tol: float) -> np.ndarray:
    """Pixels whose float64 coordinate lies within `tol` of an integer grid line: where the hole-aware depth, which is
    discontinuous there, may legitimately differ between two maps `tol` apart."""
    mx, my = map_f64(c)
    with np.errstate(invalid="ignore"):
        return (np.abs(mx - np.rint(mx)) <= tol) | (np.abs(my - np.rint(my)) <= tol)


def tap_spread(c: Cam, plane: np.ndarray) -> np.ndarray:
    """(out_h, out_w) float64: largest minus smallest value among the taps of the cell the float64 coordinate lies in, joined with
    those of the float32 coordinate's cell where that is another one (taps outside the source are 0).  Bilinear sampling with a zero
    border is continuous and, inside a cell, changes by at most the cell's spread per pixel of L1 distance."""
    padded = np.pad(plane.astype(np.float64), 2)
    H, W = plane.shape
    lo = np.full((c.out_h, c.out_w), np.inf)
    hi = np.full((c.out_h, c.out_w), -np.inf)
    for mx, my in (map_f64(c), tuple(a.astype(np.float64) for a in map_f32(c))):
        ok = np.isfinite(mx) & np.isfinite(my)
        x0 = np.clip(np.floor(np.where(ok, mx, -5.0)), -2, W).astype(np.int64)
        y0 = np.clip(np.floor(np.where(ok, my, -5.0)), -2, H).astype(np.int64)
        for dy in (0, 1):
            for dx in (0, 1):
                v = padded[y0 + dy + 2, x0 + dx + 2]
                lo, hi = np.minimum(lo, v), np.maximum(hi, v)
    return hi - lo


def resize_spread(img: np.ndarray, w: int, h: int) -> np.ndarray:
    """(C, h, w): spread of the 3x3 source pixels around each output pixel's source cell (covers the neighbouring cell too)."""
    _, H, W = img.shape
    sx = np.clip(np.floor((np.arange(w) + 0.5) * (W / w) - 0.5).astype(np.int64), 0, W - 1)
    sy = np.clip(np.floor((np.arange(h) + 0.5) * (H / h) - 0.5).astype(np.int64), 0, H - 1)
    lo = np.full((img.shape[0], h, w), np.inf)
    hi = -lo
    for dy in (-1, 0, 1, 2):
        for dx in (-1, 0, 1, 2):
            v = img[:, np.clip(sy + dy, 0, H - 1)][:, :, np.clip(sx + dx, 0, W - 1)].astype(np.float64)
            lo, hi = np.minimum(lo, v), np.maximum(hi, v)
    return hi - lo
