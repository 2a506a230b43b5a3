"""NumPy restatement of segs_depth_seed (include/segs_densify.h) and the seeded inputs its tests share.

`seed(..., dtype=np.float32)` does every operation of the header in float32, one rounding per operation and in the stated
order, so the device is compared with it bit for bit; `dtype=np.float64` is the same rule in double precision, which tells
how many voxels of an input sit so close to a voxel boundary that the precision decides them (a condition on the inputs)."""
from dataclasses import dataclass

import numpy as np

KEY_BIAS = 1 << 20
COUNT_NAMES = ("valid lattice pixels", "unobserved", "in front", "out of range", "distinct voxels", "new anchors")


@dataclass
class Params:
    stride: int = 4
    alpha_max: float = 0.5
    use_front: bool = False
    front_abs: float = 0.05
    front_rel: float = 0.0
    voxel_size: float = 0.05


def depth_target(z, min_depth, max_depth):
    """segs_depth_target's map: Z where the sensor depth is finite and strictly inside (min_depth, max_depth), else 0."""
    z = np.asarray(z, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(z) & (z > np.float32(min_depth))
        if max_depth > 0:
            ok &= z < np.float32(max_depth)
    return np.where(ok, z, np.float32(0)).astype(np.float32)


def cam_to_world(view):
    """inv(view) in float64, cast to float32 (the view matrix's own transposed layout: translation in the last row)."""
    return np.linalg.inv(np.asarray(view, dtype=np.float64).reshape(4, 4)).astype(np.float32)


def lattice(H, W, stride):
    vs, us = np.arange(stride // 2, H, stride), np.arange(stride // 2, W, stride)
    v, u = np.meshgrid(vs, us, indexing="ij")
    return u.reshape(-1), v.reshape(-1)


def anchor_voxels(anchor, voxel_size, dtype=np.float32):
    """rint(anchor / voxel_size), clamped like pack_key clamps the existing anchors' voxels."""
    if len(anchor) == 0:
        return np.zeros((0, 3), dtype=np.int64)
    g = np.rint(np.asarray(anchor, dtype=dtype) / dtype(voxel_size))
    return np.clip(g, -KEY_BIAS, KEY_BIAS - 1).astype(np.int64)


def seed(anchor, target, depth, alpha, tanfovx, tanfovy, M, p: Params, dtype=np.float32):
    """-> dict(counts=[6 ints], n_new, new_anchor (n_new, 3) float32 in lexicographic voxel order, voxels (distinct, 3) int64,
    cand_pixels = flat image indices of the candidate lattice pixels before the range test)."""
    f = dtype
    H, W = target.shape
    u, v = lattice(H, W, p.stride)
    Z = target[v, u].astype(f)
    valid = Z > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        if alpha is None:
            unobserved, front = valid.copy(), np.zeros_like(valid)
        else:
            A, D = alpha[v, u].astype(f), depth[v, u].astype(f)
            amax = f(np.float32(p.alpha_max))
            unobserved = valid & (A < amax)
            margin = f(np.float32(p.front_abs)) + f(np.float32(p.front_rel)) * Z
            front = valid & bool(p.use_front) & (A >= amax) & ((D / A - Z) > margin)
    cand = unobserved | front
    uc, vc, Zc = u[cand], v[cand], Z[cand]
    M = np.asarray(M, dtype=np.float32).astype(f)
    xv = ((2 * uc + 1).astype(f) / f(W) - f(1)) * f(np.float32(tanfovx)) * Zc
    yv = ((2 * vc + 1).astype(f) / f(H) - f(1)) * f(np.float32(tanfovy)) * Zc
    g = np.empty((len(Zc), 3), dtype=f)
    with np.errstate(invalid="ignore", over="ignore"):
        for d in range(3):
            world = ((xv * M[0, d] + yv * M[1, d]) + Zc * M[2, d]) + M[3, d]
            g[:, d] = np.rint(world / f(np.float32(p.voxel_size)))
        inside = np.all((g >= -KEY_BIAS) & (g < KEY_BIAS), axis=1)
    vox = np.unique(g[inside].astype(np.int64), axis=0) if inside.any() else np.zeros((0, 3), dtype=np.int64)
    taken = set(map(tuple, anchor_voxels(anchor, p.voxel_size, f).tolist()))
    keep = np.array([tuple(r) not in taken for r in vox.tolist()], dtype=bool) if len(vox) else np.zeros(0, dtype=bool)
    new = vox[keep]
    new_anchor = (new.astype(np.float32) * np.float32(p.voxel_size)).astype(np.float32).reshape(-1, 3)
    counts = [int(valid.sum()), int(unobserved.sum()), int(front.sum()), int((~inside).sum()), len(vox), len(new)]
    return dict(counts=counts, n_new=len(new), new_anchor=new_anchor, voxels=vox, new_voxels=new, cand_pixels=(vc * W + uc))


# ---- the seeded inputs of tests/test_depth_seed_gpu.py (tests/test_depth_seed_cpu.py checks the condition on them)
MIN_DEPTH, MAX_DEPTH = 0.1, 10.0
SIZES = [(17, 33), (48, 64)]              # (H, W): 33x17 and 64x48 images
STRIDES = [1, 2, 3, 4]
# 1x1; 3x2 with stride 4, whose lattice (first pixel at stride // 2 = 2, below the image size) is EMPTY under the stated rule;
# and 3x3 with stride 4, which is the single-lattice-pixel image
SMALL = [((1, 1), 1), ((2, 3), 4), ((3, 3), 4)]
ANCHOR_COUNTS = [0, 1, 257, 5000]
TANFOV = (0.57, 0.43)


def rotated_view(seed=0, translation=(0.3, -0.2, 0.5)):
    """A world-to-camera matrix in the transposed layout: a rotation about a skew axis, then a translation."""
    rng = np.random.default_rng(100 + seed)
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    ang = 0.6
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    R = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K)
    view = np.eye(4)
    view[:3, :3] = R.T
    view[3, :3] = np.asarray(translation, dtype=np.float64)
    return view.astype(np.float32)


def maps(H, W, seed, alpha_max=0.5):
    """(sensor depth with 0 / NaN / inf / beyond-max entries, rendered depth D, rendered opacity A straddling alpha_max with
    entries exactly alpha_max, exactly 0 and exactly 1; D / A lies within +-0.5 of the sensor depth)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    z = (1.5 + 0.02 * xx + 0.03 * yy + 0.2 * rng.random((H, W))).astype(np.float32)
    n = H * W
    special = rng.permutation(n)[:max(4, n // 8)] if n >= 4 else np.arange(0)
    for i, val in zip(np.array_split(special, 4), (0.0, np.nan, np.inf, 12.0)):
        z.reshape(-1)[i] = val
    alpha = rng.random((H, W)).astype(np.float32)
    pick = rng.permutation(n)
    for i, val in zip(np.array_split(pick[:max(3, n // 6)], 3), (alpha_max, 0.0, 1.0)):
        alpha.reshape(-1)[i] = val
    zz = np.where(np.isfinite(z), z, 2.0).astype(np.float32)
    depth = (alpha * (zz + (rng.random((H, W)).astype(np.float32) - np.float32(0.5)))).astype(np.float32)
    return z, depth, alpha


def anchors_for(A, target, view, p: Params, seed):
    """A anchors: up to half of them inside candidate voxels of the no-render call, at most a third of those voxels (so that
    some candidates are blocked and most are not), the rest scattered over the same region."""
    rng = np.random.default_rng(1000 + seed)
    if A == 0:
        return np.zeros((0, 3), dtype=np.float32)
    r = seed_all(target, view, p)
    vox = r["voxels"]
    if len(vox) == 0:
        return rng.normal(size=(A, 3)).astype(np.float32)
    k = min((A + 1) // 2, max(1, len(vox) // 3))
    inside = vox[rng.permutation(len(vox))[:k]].astype(np.float32) * np.float32(p.voxel_size)
    inside = inside + (rng.random((k, 3)).astype(np.float32) - np.float32(0.5)) * np.float32(0.6 * p.voxel_size)
    lo, hi = vox.min(0) * p.voxel_size, vox.max(0) * p.voxel_size
    rest = (lo + (hi - lo) * rng.random((A - k, 3))).astype(np.float32)
    return np.concatenate([inside, rest]).astype(np.float32)


def seed_all(target, view, p: Params, dtype=np.float32):
    """The no-render call on an empty map."""
    return seed(np.zeros((0, 3), np.float32), target, None, None, TANFOV[0], TANFOV[1], cam_to_world(view), p, dtype)


def synthetic_cases():
    """Every (H, W, stride, A, use_front) of GPU test 1 with its inputs; built once per process."""
    global _CASES
    if _CASES is None:
        _CASES = []
        view = rotated_view()
        shapes = [(hw, s) for hw in SIZES for s in STRIDES] + SMALL
        for k, ((H, W), stride) in enumerate(shapes):
            z, depth, alpha = maps(H, W, seed=k)
            target = depth_target(z, MIN_DEPTH, MAX_DEPTH)
            for A in ANCHOR_COUNTS:
                for use_front in (False, True):
                    p = Params(stride=stride, use_front=use_front, front_abs=0.1, front_rel=0.05)
                    _CASES.append(dict(H=H, W=W, p=p, A=A, sensor=z, target=target, depth=depth, alpha=alpha, view=view,
                                       anchor=anchors_for(A, target, view, p, seed=k)))
    return _CASES


_CASES = None
