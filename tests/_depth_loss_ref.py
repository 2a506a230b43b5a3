"""Float64 restatement of the depth-supervision loss (include/segs_train.h, "Depth supervision from an RGB-D frame").

D = rendered depth, A = rendered opacity, Z = sensor depth, all (H, W).  The thresholds and weights are what the C struct holds:
float32 values, so they are rounded to float32 first and only then taken to float64 (A >= alpha_min is decided on the device
against float32(alpha_min)).

    valid = isfinite(Z) and Z > min_depth and (max_depth <= 0 or Z < max_depth)          N = count(valid), n = max(N, 1)
    used  = valid and A >= alpha_min                                                     d = D  or  D / A  (normalize)
    L_depth = (1/n) sum_used |d - Z|    L_alpha = (1/n) sum_valid (1 - A)    total = lambda_depth L_depth + lambda_alpha L_alpha
"""
from collections import namedtuple

import numpy as np
import torch

Params = namedtuple("Params", "lambda_depth lambda_alpha alpha_min normalize min_depth max_depth", defaults=(0.0, 0.0, False, 0.0, 0.0))


def f32(x: float) -> float:
    return float(np.float32(x))


def masks(A: torch.Tensor, Z: torch.Tensor, p: Params):
    Z, A = Z.double(), A.double()
    valid = torch.isfinite(Z) & (Z > f32(p.min_depth))
    if f32(p.max_depth) > 0:
        valid = valid & (Z < f32(p.max_depth))
    return valid, valid & (A >= f32(p.alpha_min))


def target_map(Z: torch.Tensor, p: Params) -> torch.Tensor:
    """What segs_depth_target writes: Z where valid, 0 elsewhere (in Z's own dtype)."""
    valid, _ = masks(torch.ones_like(Z), Z, p)
    return torch.where(valid, Z, torch.zeros_like(Z))


def value(D: torch.Tensor, A: torch.Tensor, Z: torch.Tensor, p: Params):
    """(total, L_depth, L_alpha, n_used, N) as float64 tensors / ints; differentiable in D and A."""
    valid, used = masks(A, Z, p)
    D, A, Z = D.double(), A.double(), Z.double()
    N = int(valid.sum())
    n = float(max(N, 1))
    one = torch.ones_like(A)
    d = D / torch.where(used, A, one) if p.normalize else D
    zero = torch.zeros_like(D)
    l_depth = torch.where(used, (d - torch.where(valid, Z, zero)).abs(), zero).sum() / n
    l_alpha = torch.where(valid, 1.0 - A, zero).sum() / n
    return f32(p.lambda_depth) * l_depth + f32(p.lambda_alpha) * l_alpha, l_depth, l_alpha, int(used.sum()), N


def gradients(D: torch.Tensor, A: torch.Tensor, Z: torch.Tensor, p: Params):
    """Closed form: (dL/dD, dL/dA, s) with s = sgn(d - Z) on used pixels and 0 elsewhere, all float64."""
    valid, used = masks(A, Z, p)
    D, A, Z = D.double(), A.double(), Z.double()
    n = float(max(int(valid.sum()), 1))
    ld, la = f32(p.lambda_depth), f32(p.lambda_alpha)
    zero, one = torch.zeros_like(D), torch.ones_like(D)
    As = torch.where(used, A, one)
    d = D / As if p.normalize else D
    s = torch.where(used, torch.sign(d - torch.where(valid, Z, zero)), zero)
    if p.normalize:
        gD = ld * s / (n * As)
        gA = -ld * s * D / (n * As * As)
    else:
        gD = ld * s / n
        gA = zero.clone()
    gA = gA - torch.where(valid, one, zero) * (la / n)
    return gD, gA, s
