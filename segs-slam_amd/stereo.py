"""Stereo frames as depth frames: semi-global matching of a rectified pair (include/segs_points.h, csrc/stereo_sgm.hip;
specification in DESIGN.md 3i).  The reference's stereo branch (src/gaussian_mapper.cpp:1591-1610) asks cv::cuda::StereoSGM for
the same thing; this is written from the published algorithm, not from OpenCV, and claims no parity with its bytes.

    sgm = StereoSGM.from_config(cfg, H, W, "cuda:0")          # Stereo.min_disparity / Stereo.num_disparity of the configuration
    depth = sgm.compute_depth(left_rgb, right_rgb, fx, baseline)   # (H, W) float32, 0 = no measurement

`depth` is what FusedDepthLoss.prepare, ScaffoldTrainerStep.training_once(..., gt_depths), pose_gradient and seed_keyframe take
as a sensor depth.  The returned tensors are the object's own buffers, overwritten by the next call.  There is no CPU path.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _capi

INVALID_RAW = 0xFFFF


def _require_gpu(t: torch.Tensor, name: str):
    if not t.is_cuda:
        raise RuntimeError(f"{name} must live on the GPU: the stereo matcher has no CPU path")


def _stream(device) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def rgb_to_gray_u8(rgb: torch.Tensor, out: torch.Tensor = None) -> torch.Tensor:
    """cvtColor(RGB2GRAY) + convertTo(CV_8UC1, 255) of the reference's stereo branch: (3, H, W) float32 -> (H, W) uint8."""
    _require_gpu(rgb, "rgb")
    if rgb.dim() != 3 or rgb.shape[0] != 3 or rgb.dtype != torch.float32:
        raise ValueError(f"rgb must be a float32 (3, H, W) image, not {rgb.dtype} {tuple(rgb.shape)}")
    rgb = rgb.contiguous()
    H, W = int(rgb.shape[1]), int(rgb.shape[2])
    if out is None:
        out = torch.empty((H, W), dtype=torch.uint8, device=rgb.device)
    with torch.cuda.device(rgb.device):
        _capi.check(_capi.lib().segs_rgb_to_gray_u8(W, H, C.c_void_p(rgb.data_ptr()), C.c_void_p(out.data_ptr()), _stream(rgb.device)),
                    "segs_rgb_to_gray_u8")
    return out


class StereoSGM:
    """One object per image size and parameter set; every buffer is made here and nothing is allocated per call."""

    def __init__(self, H: int, W: int, device, num_disparities: int = 128, min_disparity: int = 0, P1: int = 10, P2: int = 120,
                 uniqueness_ratio: int = 5, paths: int = 4, lr_max_diff: int = 1, median: bool = True):
        self._lib = _capi.lib()
        self.H, self.W, self.dev = int(H), int(W), torch.device(device)
        if self.dev.type != "cuda":
            raise RuntimeError("StereoSGM needs a GPU device: there is no CPU path")
        self.params = _capi.StereoParamsC(int(num_disparities), int(min_disparity), int(P1), int(P2), int(uniqueness_ratio), int(paths),
                                          int(lr_max_diff), int(bool(median)))
        self.D = int(num_disparities)
        nbytes = int(self._lib.segs_stereo_sgm_temp_bytes(self.W, self.H, self.D, int(paths)))
        if nbytes == 0:
            raise ValueError(f"StereoSGM: unsupported size or parameters (1 <= W, H <= 4096, num_disparities in (64, 128, 256), "
                             f"paths 4 or 8), got {self.H}x{self.W}, {num_disparities}, {paths}")
        mk = lambda shape, dtype: torch.zeros(shape, dtype=dtype, device=self.dev)     # noqa: E731
        self.temp = torch.empty(nbytes, dtype=torch.uint8, device=self.dev)
        self.disp16 = mk((self.H, self.W), torch.int16)
        self.depth = mk((self.H, self.W), torch.float32)
        self._gray = [mk((self.H, self.W), torch.uint8), mk((self.H, self.W), torch.uint8)]

    @classmethod
    def from_config(cls, cfg, H: int, W: int, device, **overrides) -> "StereoSGM":
        """Stereo.min_disparity / Stereo.num_disparity of a MapperConfig (src/gaussian_mapper.cpp:93-95 reads the same two keys
        and leaves everything else at StereoSGM's defaults); an absent key reads as 0, like cv::FileNode."""
        kw = dict(num_disparities=int(cfg.raw.get("Stereo.num_disparity", 0)), min_disparity=int(cfg.raw.get("Stereo.min_disparity", 0)))
        kw.update(overrides)
        return cls(H, W, device, **kw)

    # ------------------------------------------------------------------ inputs
    def _grey(self, img: torch.Tensor, slot: int, name: str) -> torch.Tensor:
        _require_gpu(img, name)
        if img.dtype == torch.uint8 and tuple(img.shape) == (self.H, self.W):
            return img.contiguous()
        if img.dtype == torch.float32 and tuple(img.shape) == (3, self.H, self.W):
            return rgb_to_gray_u8(img, self._gray[slot])
        raise ValueError(f"{name} must be a uint8 ({self.H}, {self.W}) grey image or a float32 (3, {self.H}, {self.W}) RGB image, "
                         f"not {img.dtype} {tuple(img.shape)}")

    def _u8(self, img: torch.Tensor, name: str) -> torch.Tensor:
        _require_gpu(img, name)
        if img.dtype != torch.uint8 or tuple(img.shape) != (self.H, self.W):
            raise ValueError(f"{name} must be a uint8 ({self.H}, {self.W}) image, not {img.dtype} {tuple(img.shape)}")
        return img.contiguous()

    def _run(self, left, right, depth, fb16: float, stages=None):
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())     # noqa: E731
        with torch.cuda.device(self.dev):
            if stages is None:
                st = self._lib.segs_stereo_sgm(C.byref(self.params), self.W, self.H, p(left), p(right), p(self.disp16), p(depth),
                                               float(fb16), p(self.temp), _stream(self.dev))
                _capi.check(st, "segs_stereo_sgm")
            else:
                st = self._lib.segs_debug_stereo_sgm_stages(C.byref(self.params), self.W, self.H, p(left), p(right), p(self.disp16),
                                                            p(depth), float(fb16), p(self.temp), *[p(t) for t in stages],
                                                            _stream(self.dev))
                _capi.check(st, "segs_debug_stereo_sgm_stages")

    # ------------------------------------------------------------------ calls
    def compute(self, left_u8: torch.Tensor, right_u8: torch.Tensor) -> torch.Tensor:
        """(H, W) int16: 16 x disparity where valid, 16 (min_disparity - 1) where not."""
        self._run(self._u8(left_u8, "left"), self._u8(right_u8, "right"), None, 0.0)
        return self.disp16

    @staticmethod
    def fb16(fx: float, baseline: float) -> float:
        """16 fx baseline: formed in float64, handed over as one float32."""
        return float(torch.tensor(16.0 * float(fx) * float(baseline), dtype=torch.float64).to(torch.float32).item())

    def compute_depth(self, left: torch.Tensor, right: torch.Tensor, fx: float, baseline: float) -> torch.Tensor:
        """(H, W) float32 depth = fx baseline / disparity where the match is valid and the disparity positive, else 0.  Inputs:
        uint8 grey (H, W) or float32 RGB (3, H, W) in [0, 1], which goes through rgb_to_gray_u8."""
        self._run(self._grey(left, 0, "left"), self._grey(right, 1, "right"), self.depth, self.fb16(fx, baseline))
        return self.depth

    def stages(self, left: torch.Tensor, right: torch.Tensor, fx: float = 1.0, baseline: float = 1.0) -> dict:
        """The same run with every stage copied out (new tensors: a debugging call): census_left / census_right (int32 holding
        the 31 bits), S (H, W, D) and raw_winner / raw_median (int16 holding the uint16 bits), disp_right, disp16, depth."""
        n = (self.H, self.W)
        mk = lambda shape, dtype: torch.zeros(shape, dtype=dtype, device=self.dev)     # noqa: E731
        out = {"census_left": mk(n, torch.int32), "census_right": mk(n, torch.int32), "S": mk(n + (self.D,), torch.int16),
               "raw_winner": mk(n, torch.int16), "raw_median": mk(n, torch.int16), "disp_right": mk(n, torch.int16)}
        self._run(self._grey(left, 0, "left"), self._grey(right, 1, "right"), self.depth, self.fb16(fx, baseline), list(out.values()))
        out["disp16"], out["depth"] = self.disp16.clone(), self.depth.clone()
        return out
