"""The float32 restatement of LibTorch's C++ Adam step that pins csrc/optim.hip bit for bit (tests/test_trainer_gpu.py,
tests/test_adam_gpu.py), and the same update in float64 that shows the pin itself is sound."""
import numpy as np


def adam_reference(p, g, m, v, lr, b1, b2, eps, step, gscale):
    """float32 restatement of LibTorch's C++ Adam step, one rounding per operation; hyper-parameters
    are doubles and every scalar is formed in double before it is rounded into the float32 tensor arithmetic."""
    f = np.float32
    bc1 = 1.0 - b1 ** step
    bc2 = 1.0 - b2 ** step
    step_size = f(lr / bc1)
    sqrt_bc2 = f(np.sqrt(bc2))
    gr = g * f(gscale)
    m = m * f(b1) + gr * f(1.0 - b1)
    v = v * f(b2) + gr * gr * f(1.0 - b2)
    denom = np.sqrt(v) / sqrt_bc2 + f(eps)
    p = p - step_size * (m / denom)
    return p.astype(f), m.astype(f), v.astype(f)


def adam_float64(p, g, m, v, lr, b1, b2, eps, step, gscale):
    """The same update with every operand and operation in float64; returns (p, m, v, update) with p = p_in - update."""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    bc1 = 1.0 - b1 ** step
    bc2 = 1.0 - b2 ** step
    gr = g * gscale
    m = m * b1 + gr * (1.0 - b1)
    v = v * b2 + gr * gr * (1.0 - b2)
    upd = (lr / bc1) * (m / (np.sqrt(v) / np.sqrt(bc2) + eps))
    return p - upd, m, v, upd
