"""Depth supervision from an RGB-D frame (include/segs_train.h, csrc/depth_loss.hip): the loss between the
rasterizer's depth / opacity maps and the sensor's depth, and its two gradient maps for RasterEngine.backward.

    used = valid and A >= alpha_min;   d = D  or  D / A (normalize);   n = max(number of valid pixels, 1)
    total = lambda_depth * (1/n) sum_used |d - Z|  +  lambda_alpha * (1/n) sum_valid (1 - A)

A pixel is valid when the sensor depth is finite and strictly inside (min_depth, max_depth) -- the test of the reference's
back-projection (src/gaussian_mapper.cpp:1673-1676), its only use of the sensor depth.  There is no CPU path.
"""
from __future__ import annotations

import ctypes as C
from collections import OrderedDict
from dataclasses import dataclass
from typing import Optional, Union

import torch

from . import _capi


@dataclass(frozen=True)
class DepthLossParams:
    lambda_depth: float
    lambda_alpha: float = 0.0
    alpha_min: float = 0.0           # silhouette threshold: pixels the map covers less than this take no part in the depth term
    normalize: bool = False          # compare D / A (the expected depth of what was hit) instead of D
    min_depth: float = 0.0           # RGBD.min_depth / RGBD.max_depth of the configuration; max_depth <= 0: no upper bound
    max_depth: float = 0.0

    def __post_init__(self):
        if self.normalize and not self.alpha_min > 0.0:
            raise ValueError("normalize divides by the rendered opacity: it needs alpha_min > 0")
        if self.min_depth < 0.0:
            raise ValueError("min_depth must not be negative")


class DepthTarget:
    """A prepared sensor depth: `block` holds the (H, W) map (0 where invalid) followed by the valid-pixel count (uint32) --
    4 H W + 16 bytes on the device.  Made by FusedDepthLoss.prepare, once per keyframe image."""

    def __init__(self, block: torch.Tensor, H: int, W: int):
        self.block, self.H, self.W = block, int(H), int(W)

    @property
    def shape(self):
        return (self.H, self.W)

    @property
    def map(self) -> torch.Tensor:
        return self.block[:self.H * self.W].view(self.H, self.W)

    def n_valid(self) -> int:
        """The number of valid pixels (synchronises)."""
        return int(self.block[self.H * self.W:self.H * self.W + 1].view(torch.int32).item())


def depth_shape(depth) -> tuple:
    """(H, W) of a sensor depth given as a tensor ((H, W) or (1, H, W)) or a DepthTarget."""
    if isinstance(depth, DepthTarget):
        return depth.shape
    if depth.dim() == 3 and depth.shape[0] == 1:
        return tuple(depth.shape[1:])
    if depth.dim() != 2:
        raise ValueError(f"a sensor depth is (H, W) or (1, H, W), not {tuple(depth.shape)}")
    return tuple(depth.shape)


class FusedDepthLoss:
    """One object per image size.  `__call__(depth, alpha, target, loss_inout)` returns (value, dL_ddepth, dL_dalpha): a view of
    result word 0 and the two pre-allocated (H, W) gradient maps, overwritten by every call.  `out` = {total, L_depth, L_alpha,
    used pixels}."""

    MAX_CACHED_TARGETS = 8           # raw tensors handed in as targets: 4 H W bytes each

    def __init__(self, H: int, W: int, device, params: DepthLossParams):
        self._lib = _capi.lib()
        self.H, self.W, self.dev, self.params = int(H), int(W), torch.device(device), params
        if self.dev.type != "cuda":
            raise RuntimeError("FusedDepthLoss needs a GPU device: there is no CPU path")
        self._cparams = _capi.DepthLossParamsC(float(params.lambda_depth), float(params.lambda_alpha), float(params.alpha_min),
                                               int(bool(params.normalize)))
        self._target_floats = int(self._lib.segs_depth_target_floats(self.H, self.W))
        f32 = dict(dtype=torch.float32, device=self.dev)
        self.temp = torch.empty(self._lib.segs_depth_loss_temp_bytes(self.H, self.W), dtype=torch.uint8, device=self.dev)
        self.out = torch.zeros(4, **f32)
        self.dL_ddepth = torch.empty((self.H, self.W), **f32)
        self.dL_dalpha = torch.empty((self.H, self.W), **f32)
        self._targets: "OrderedDict[tuple, tuple]" = OrderedDict()

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)

    def _check_map(self, t: torch.Tensor, what: str):
        if not t.is_cuda:
            raise RuntimeError(f"{what} is not on the GPU: there is no CPU path")
        if tuple(t.shape) != (self.H, self.W) or t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError(f"{what} must be a contiguous float32 ({self.H}, {self.W}) map, not {t.dtype} {tuple(t.shape)}")

    def prepare(self, sensor_depth: torch.Tensor) -> DepthTarget:
        if depth_shape(sensor_depth) != (self.H, self.W):
            raise ValueError(f"sensor depth is {depth_shape(sensor_depth)}, the loss was made for {(self.H, self.W)}")
        z = sensor_depth.view(self.H, self.W) if sensor_depth.is_contiguous() else sensor_depth.reshape(self.H, self.W).contiguous()
        self._check_map(z, "sensor depth")
        block = torch.empty(self._target_floats, dtype=torch.float32, device=self.dev)
        st = self._lib.segs_depth_target(C.c_void_p(z.data_ptr()), self.H, self.W, float(self.params.min_depth),
                                         float(self.params.max_depth), C.c_void_p(block.data_ptr()), self._stream())
        _capi.check(st, "segs_depth_target")
        return DepthTarget(block, self.H, self.W)

    def target_of(self, target: Union[torch.Tensor, DepthTarget]) -> DepthTarget:
        """`target` itself when prepared; a raw tensor goes through a cache of MAX_CACHED_TARGETS entries keyed by its address
        and version (the tensor is kept alive with its entry: the key is its address)."""
        if isinstance(target, DepthTarget):
            if target.shape != (self.H, self.W):
                raise ValueError(f"depth target is {target.shape}, the loss was made for {(self.H, self.W)}")
            return target
        key = (target.data_ptr(), target._version)
        hit = self._targets.get(key)
        if hit is not None:
            self._targets.move_to_end(key)
            return hit[0]
        prepared = self.prepare(target)
        self._targets[key] = (prepared, target)
        while len(self._targets) > self.MAX_CACHED_TARGETS:
            self._targets.popitem(last=False)
        return prepared

    def __call__(self, depth: torch.Tensor, alpha: torch.Tensor, target: Union[torch.Tensor, DepthTarget],
                 loss_inout: Optional[torch.Tensor] = None):
        self._check_map(depth, "depth")
        self._check_map(alpha, "alpha")
        tgt = self.target_of(target)
        p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        st = self._lib.segs_depth_loss(p(depth), p(alpha), p(tgt.block), self.H, self.W, C.byref(self._cparams), p(self.dL_ddepth),
                                       p(self.dL_dalpha), p(self.out), None if loss_inout is None else p(loss_inout), p(self.temp),
                                       self._stream())
        _capi.check(st, "segs_depth_loss")
        return self.out[0], self.dL_ddepth, self.dL_dalpha
