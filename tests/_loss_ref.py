"""Shared by tests/test_loss_gpu.py: the float64 reference of the fused L1 + SSIM loss, the float32 yardstick, and the inputs.

Reference: segs_slam_amd.loss_utils.l1_loss / ssim (the mirror of include/loss_utils.h, pinned by tests/golden/loss_reference.npz)
on CPU tensors cast to float64 -- the window is the reference's float32 window cast up -- with autograd for dL/dimage;
loss = (1 - l) * l1 + l * (1 - ssim).  The SAME chain in float32 on the CPU is the yardstick e_ref: how far the reference's own
op chain is from float64 on that input (E[x^2] - mu^2 cancels on smooth images, so this is input-dependent)."""
import functools

import numpy as np
import torch

CLASSES = ("noise", "smooth", "const", "equal", "black", "zero_rows", "out_of_range", "impulse")
WINDOW, HALO, TILE_W = 11, 5, 32


def tile_rows_rule(H, W):
    """The rule of csrc/loss.hip restated: 32-row tiles once 3 * ceil(W / 32) * ceil(H / 32) workgroups reach 1536, else 16."""
    return 32 if 3 * ((W + 31) // 32) * ((H + 31) // 32) >= 1536 else 16


def zero_row_range(H):
    return H // 3, H // 2


def impulse_pixels(H, W):
    """(y, x) of the 1.0 pixels of the `impulse` class: the four corners and the tile seams that fit."""
    pts = {(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)}
    pts |= {(y, x) for y in (15, 16, 31, 32) for x in (31, 32) if y < H and x < W}
    return sorted(pts)


def _noise(H, W, gen):
    gt = torch.rand(3, H, W, generator=gen)
    img = (gt + 0.2 * torch.randn(3, H, W, generator=gen)).clamp(0, 1).contiguous()
    img[:, : H // 4] = gt[:, : H // 4]      # exact-equality region: sign(0) = 0 in the L1 gradient
    return img, gt


def make_pair(cls, H, W, seed=0):
    """(image, target), float32 CPU tensors of shape (3, H, W)."""
    gen = torch.Generator().manual_seed(1000003 * seed + 1009 * H + W)
    if cls == "noise":
        img, gt = _noise(H, W, gen)
    elif cls == "smooth":
        y, x = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
        gt = (0.5 + 0.4 * torch.sin(x / 7.0) * torch.cos(y / 5.0)).float().expand(3, H, W).contiguous()
        img = (gt + 0.01 * torch.randn(3, H, W, generator=gen)).clamp(0, 1)
    elif cls == "const":
        img, gt = torch.full((3, H, W), 0.5), torch.full((3, H, W), 0.25)
    elif cls == "equal":
        gt = _noise(H, W, gen)[1]
        img = gt.clone()
    elif cls == "black":
        img, gt = torch.zeros(3, H, W), torch.zeros(3, H, W)
    elif cls == "zero_rows":
        img, gt = _noise(H, W, gen)
        lo, hi = zero_row_range(H)
        img[:, lo:hi] = 0.0
        gt[:, lo:hi] = 0.0
    elif cls == "out_of_range":
        img, gt = _noise(H, W, gen)
        img = img * 8.0 - 2.0
    elif cls == "impulse":
        img, gt = torch.zeros(3, H, W), torch.zeros(3, H, W)
        for y, x in impulse_pixels(H, W):
            img[:, y, x] = 1.0
    else:
        raise ValueError(cls)
    return img.contiguous(), gt.contiguous()


def loss_chain(img, gt, lam, dtype):
    """The reference op chain in `dtype` on the CPU: ([loss, l1, ssim], dL/dimage) as float64 numpy arrays."""
    from segs_slam_amd import loss_utils
    x = img.detach().to("cpu", dtype).clone().requires_grad_(True)
    t = gt.detach().to("cpu", dtype)
    l1 = loss_utils.l1_loss(x, t)
    ss = loss_utils.ssim(x, t)
    loss = (1.0 - lam) * l1 + lam * (1.0 - ss)
    (g,) = torch.autograd.grad(loss, x)
    return np.array([loss.item(), l1.item(), ss.item()], dtype=np.float64), g.numpy().astype(np.float64)


class Reference:
    """out64 / g64: the float64 reference; e_out (3,) / e_dL: the yardstick, |float32 chain - float64 chain|."""

    def __init__(self, img, gt, lam):
        self.out64, self.g64 = loss_chain(img, gt, lam, torch.float64)
        out32, g32 = loss_chain(img, gt, lam, torch.float32)
        self.e_out = np.abs(out32 - self.out64)
        self.e_dL = float(np.abs(g32 - self.g64).max())
        self.gmax = float(np.abs(self.g64).max())
        self.g64.setflags(write=False)

    def dL_bar(self):
        return 4.0 * self.e_dL + 4.0 * 2.0 ** -23 * self.gmax

    def scalar_bars(self):
        return 4.0 * self.e_out + 2e-6


def _case(cls, H, W, lam, seed):
    img, gt = make_pair(cls, H, W, seed)
    return img, gt, Reference(img, gt, lam)


_cached_case = functools.lru_cache(maxsize=None)(_case)


def case(cls, H, W, lam=0.2, seed=0):
    """(image, target, Reference) of one case; the small ones are computed once per session and shared (the camera-sized
    ones are each used by one test and not kept)."""
    return (_cached_case if H * W <= 64 * 1024 else _case)(cls, H, W, lam, seed)
