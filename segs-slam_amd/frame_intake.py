"""Frame intake on the device: a camera frame as the sensor delivers it -> what the step, the stereo matcher, the depth loss and
the depth seeding take (include/segs_frame_intake.h, csrc/frame_intake.hip; specification and bytes in DESIGN.md 3j).

The reference does this with OpenCV on the host: Camera::initUndistortRectifyMapAndMask / undistortImage (include/camera.h:71-115)
and the cv::cuda::resize pyramid loops (src/gaussian_mapper.cpp:623-631, 1286-1297).  Here the undistortion / rectification map is
computed per pixel in registers, never stored, and one more launch writes every pyramid level.

    cam = CameraModel.from_settings(read_opencv_yaml("TUM1.yaml"))        # pinhole + (k1, k2, p1, p2, k3); fisheye is not supported
    intake = FrameIntake(cam, "cuda:0", num_sub_levels=2)                  # mask and mask_levels are computed here, once
    f = intake.rgb(frame_u8_hwc, want_gray=True)                           # f.image (3, H, W), f.levels (coarsest first), f.gray
    z = intake.depth(raw_u16_hw)                                           # (H, W) float32 metres, 0 = no measurement

Stereo: two FrameIntake objects, left and right, each with its rectifying rotation `R` and the shared new camera as the calibration
gives them (computing them from the extrinsics -- cv::stereoRectify -- is host calibration mathematics and stays outside); their
`gray` outputs go straight into StereoSGM.compute_depth.

Returned tensors are the object's own buffers, overwritten by the next call (StereoSGM's convention).  There is no CPU path.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, Mapping, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _capi

MAX_SIZE = 8192      # SEGS_INTAKE_MAX_SIZE
MAX_LEVELS = 8       # SEGS_INTAKE_MAX_LEVELS


def pyramid_sizes(width: int, height: int, num_sub_levels: int) -> List[Tuple[int, int]]:
    """(width, height) of the sub-levels, coarsest first: level l has the factor 0.5^(num_sub_levels - l) and its size is
    truncated (src/gaussian_mapper.cpp:147-150, 329-331: `camera.width_ * kf_gaus_pyramid_factors_[l]` stored into a size_t)."""
    width, height, n = int(width), int(height), int(num_sub_levels)
    if width < 1 or height < 1 or n < 0:
        raise ValueError(f"pyramid_sizes: width, height >= 1 and num_sub_levels >= 0, got {width}, {height}, {n}")
    out = []
    for l in range(n):                                                     # noqa: E741
        factor = np.float32(0.5) ** np.float32(n - l)                       # a power of two: exact in float32
        out.append((int(np.float32(width) * factor), int(np.float32(height) * factor)))
    return out


@dataclass
class CameraModel:
    """A pinhole camera with OpenCV's five distortion coefficients, the optional rectifying rotation R and the optional new
    camera.  The default is the reference's (src/gaussian_mapper.cpp:138-162): same size, same intrinsics, R = I."""
    width: int
    height: int
    fx: float
    fy: float
    cx: float
    cy: float
    k1: float = 0.0
    k2: float = 0.0
    p1: float = 0.0
    p2: float = 0.0
    k3: float = 0.0
    R: Optional[Sequence[Sequence[float]]] = None           # 3x3 rectifying rotation (as cv::stereoRectify's R1 / R2); None = identity
    new_fx: Optional[float] = None
    new_fy: Optional[float] = None
    new_cx: Optional[float] = None
    new_cy: Optional[float] = None
    new_width: Optional[int] = None
    new_height: Optional[int] = None
    depth_map_factor: float = 1.0                            # RGBD.DepthMapFactor: raw depth units per metre
    baseline: float = 0.0                                    # Stereo.b

    def __post_init__(self):
        self.width, self.height = int(self.width), int(self.height)
        if self.new_width is not None:
            self.new_width = int(self.new_width)
        if self.new_height is not None:
            self.new_height = int(self.new_height)
        for name, v in (("width", self.width), ("height", self.height), ("new_width", self.out_width), ("new_height", self.out_height)):
            if not 1 <= v <= MAX_SIZE:
                raise ValueError(f"CameraModel: 1 <= {name} <= {MAX_SIZE}, got {v}")
        floats = [self.fx, self.fy, self.cx, self.cy, self.k1, self.k2, self.p1, self.p2, self.k3, *self.new_intrinsics,
                  self.depth_map_factor, self.baseline]
        if not all(np.isfinite(float(v)) for v in floats):
            raise ValueError("CameraModel: every parameter must be finite")
        if float(self.new_intrinsics[0]) == 0.0 or float(self.new_intrinsics[1]) == 0.0:
            raise ValueError("CameraModel: the new camera's focal lengths must be non-zero")
        if self.R is not None:
            R = np.asarray(self.R, dtype=np.float64)
            if R.shape != (3, 3) or not np.isfinite(R).all():
                raise ValueError("CameraModel: R must be a finite 3x3 matrix")
            if abs(np.linalg.det(R)) < 1e-12:
                raise ValueError("CameraModel: R is singular")
            self.R = R

    # ------------------------------------------------------------------ derived values
    @property
    def out_width(self) -> int:
        return self.width if self.new_width is None else self.new_width

    @property
    def out_height(self) -> int:
        return self.height if self.new_height is None else self.new_height

    @property
    def new_intrinsics(self) -> Tuple[float, float, float, float]:
        pick = lambda new, old: old if new is None else new      # noqa: E731
        return (pick(self.new_fx, self.fx), pick(self.new_fy, self.fy), pick(self.new_cx, self.cx), pick(self.new_cy, self.cy))

    @property
    def rinv(self) -> np.ndarray:
        """R^-1, formed in float64 and rounded once to float32 (row-major, 9 values)."""
        if self.R is None:
            return np.eye(3, dtype=np.float32).reshape(9)
        return np.linalg.inv(np.asarray(self.R, dtype=np.float64)).astype(np.float32).reshape(9)

    @property
    def inv_depth_factor(self) -> float:
        """1 / RGBD.DepthMapFactor as one float32; a factor of 0 (an absent key) means 1, as ORB-SLAM3 reads it."""
        f = float(self.depth_map_factor)
        return 1.0 if abs(f) < 1e-5 else float(np.float32(1.0 / f))

    def c_struct(self) -> "_capi.IntakeCameraC":
        f32 = lambda v: float(np.float32(v))                        # noqa: E731
        nfx, nfy, ncx, ncy = self.new_intrinsics
        return _capi.IntakeCameraC(self.width, self.height, self.out_width, self.out_height, f32(self.fx), f32(self.fy), f32(self.cx),
                                   f32(self.cy), f32(self.k1), f32(self.k2), f32(self.p1), f32(self.p2), f32(self.k3),
                                   (C.c_float * 9)(*[float(v) for v in self.rinv]), f32(nfx), f32(nfy), f32(ncx), f32(ncy))

    @classmethod
    def from_settings(cls, raw: Mapping[str, object], **overrides) -> "CameraModel":
        """From the flat scalar mapping of an ORB-SLAM3 settings file (mapper_config.read_opencv_yaml reads those files as they
        stand): Camera1.fx/fy/cx/cy, Camera1.k1/k2/p1/p2/k3, Camera.width/height, RGBD.DepthMapFactor, Stereo.b.  An absent key
        reads as 0, as everywhere in mapper_config.py.  Only `Camera.type: "PinHole"` (or no type) is accepted."""
        kind = raw.get("Camera.type", "PinHole")
        if kind != "PinHole":
            raise ValueError(f"CameraModel: Camera.type {kind!r} is not supported (the pinhole model only, like the reference's mapper)")

        def num(key):
            v = raw.get(key, 0)
            if isinstance(v, str):
                raise ValueError(f"CameraModel: {key} is not numeric: {v!r}")
            return v

        kw = dict(width=int(num("Camera.width")), height=int(num("Camera.height")),
                  fx=float(num("Camera1.fx")), fy=float(num("Camera1.fy")), cx=float(num("Camera1.cx")), cy=float(num("Camera1.cy")),
                  k1=float(num("Camera1.k1")), k2=float(num("Camera1.k2")), p1=float(num("Camera1.p1")), p2=float(num("Camera1.p2")),
                  k3=float(num("Camera1.k3")), depth_map_factor=float(num("RGBD.DepthMapFactor")), baseline=float(num("Stereo.b")))
        kw.update(overrides)
        return cls(**kw)


class IntakeFrame(NamedTuple):
    image: torch.Tensor                  # (3, H, W) float32 in [0, 1]: the target image of the step
    levels: List[torch.Tensor]           # (3, h_l, w_l), coarsest first like the reference's gaus_pyramid_original_image_
    gray: Optional[torch.Tensor]         # (H, W) uint8, the bytes rgb_to_gray_u8(image) gives; None unless asked for


def _require_gpu(t: torch.Tensor, name: str):
    if not t.is_cuda:
        raise RuntimeError(f"{name} must live on the GPU: the frame intake has no CPU path")


class FrameIntake:
    """One object per camera: every buffer is made here and nothing is allocated per call.  `mask` (H, W) and `mask_levels` are
    Camera::undistort_mask and gaus_pyramid_undistort_mask_, computed once at construction."""

    def __init__(self, camera: CameraModel, device, num_sub_levels: int = 0):
        self.camera, self.dev = camera, torch.device(device)
        if self.dev.type != "cuda":
            raise RuntimeError("FrameIntake needs a GPU device: there is no CPU path")
        n = int(num_sub_levels)
        if not 0 <= n <= MAX_LEVELS:
            raise ValueError(f"FrameIntake: 0 <= num_sub_levels <= {MAX_LEVELS}, got {n}")
        self.W, self.H = camera.out_width, camera.out_height
        self.sizes = pyramid_sizes(self.W, self.H, n)
        if any(w < 1 or h < 1 for w, h in self.sizes):
            raise ValueError(f"FrameIntake: {n} sub-levels of a {self.W}x{self.H} image include an empty level: {self.sizes}")
        self._lib = _capi.lib()
        self._cam = camera.c_struct()
        mk = lambda shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=self.dev)     # noqa: E731
        self.image = mk((3, self.H, self.W))
        self.levels = [mk((3, h, w)) for w, h in self.sizes]
        self.gray_u8 = mk((self.H, self.W), torch.uint8)
        self.gray_image = mk((1, self.H, self.W))
        self.depth_map = mk((self.H, self.W))
        self.mask = mk((self.H, self.W))
        self.mask_levels = [mk((h, w)) for w, h in self.sizes]
        self._widths = (C.c_int * max(n, 1))(*[w for w, _ in self.sizes])
        self._heights = (C.c_int * max(n, 1))(*[h for _, h in self.sizes])
        with torch.cuda.device(self.dev):
            _capi.check(self._lib.segs_undistort_mask(C.byref(self._cam), self._p(self.mask), self._stream()), "segs_undistort_mask")
        self._resize(self.mask, self.mask_levels, 1)

    @classmethod
    def from_config(cls, cfg, settings_raw: Mapping[str, object], device, **camera_overrides) -> "FrameIntake":
        """GausPyramid.do / GausPyramid.num_sub_levels of a MapperConfig (src/gaussian_mapper.cpp:321-324) and the camera of the
        ORB-SLAM3 settings mapping; an absent key reads as 0."""
        do = int(cfg.raw.get("GausPyramid.do", 0)) != 0
        n = int(cfg.raw.get("GausPyramid.num_sub_levels", 0)) if do else 0
        return cls(CameraModel.from_settings(settings_raw, **camera_overrides), device, num_sub_levels=n)

    # ------------------------------------------------------------------ plumbing
    @staticmethod
    def _p(t: Optional[torch.Tensor]):
        return None if t is None else C.c_void_p(t.data_ptr())

    def _stream(self) -> C.c_void_p:
        return C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)

    def _resize(self, src: torch.Tensor, outs: List[torch.Tensor], channels: int):
        if not outs:
            return
        ptrs = (C.c_void_p * len(outs))(*[t.data_ptr() for t in outs])
        with torch.cuda.device(self.dev):
            _capi.check(self._lib.segs_resize_levels(channels, self.W, self.H, self._p(src), len(outs), self._widths, self._heights, ptrs,
                                                     self._stream()), "segs_resize_levels")

    def _source(self, t: torch.Tensor, shape, dtypes, name: str) -> torch.Tensor:
        _require_gpu(t, name)
        if t.dtype not in dtypes or tuple(t.shape) != tuple(shape):
            raise ValueError(f"{name} must be a {' or '.join(str(d) for d in dtypes)} {tuple(shape)} tensor, not {t.dtype} {tuple(t.shape)}")
        return t.contiguous()

    # ------------------------------------------------------------------ calls
    def rgb(self, frame_u8: torch.Tensor, want_gray: bool = False) -> IntakeFrame:
        """frame_u8: (in_h, in_w, 3) uint8 as the camera delivers it.  Two launches: the undistortion (image and, if asked for,
        the grey bytes) and every pyramid level."""
        src = self._source(frame_u8, (self.camera.height, self.camera.width, 3), (torch.uint8,), "frame")
        with torch.cuda.device(self.dev):
            _capi.check(self._lib.segs_undistort_u8(C.byref(self._cam), 3, self._p(src), self._p(self.image),
                                                    self._p(self.gray_u8 if want_gray else None), self._stream()), "segs_undistort_u8")
        self._resize(self.image, self.levels, 3)
        return IntakeFrame(self.image, self.levels, self.gray_u8 if want_gray else None)

    def gray(self, frame_u8_hw: torch.Tensor) -> torch.Tensor:
        """A single-channel source (in_h, in_w) uint8 -> (H, W) uint8 for the stereo matcher; the float image it was rounded from
        stays in `gray_image` (1, H, W)."""
        src = self._source(frame_u8_hw, (self.camera.height, self.camera.width), (torch.uint8,), "frame")
        with torch.cuda.device(self.dev):
            _capi.check(self._lib.segs_undistort_u8(C.byref(self._cam), 1, self._p(src), self._p(self.gray_image), self._p(self.gray_u8),
                                                    self._stream()), "segs_undistort_u8")
        return self.gray_u8

    def depth(self, raw: torch.Tensor, hole_aware: bool = True) -> torch.Tensor:
        """raw: (in_h, in_w) uint16 (int16 storage is read as uint16 bits) or float32 -> (H, W) float32 = raw / DepthMapFactor,
        undistorted.  hole_aware: 0 wherever a contributing tap is a hole (raw <= 0) or outside the frame, so that no hole is
        averaged into a depth; False is the reference's plain bilinear remap."""
        dtypes = (torch.float32, torch.int16) + ((torch.uint16,) if hasattr(torch, "uint16") else ())
        src = self._source(raw, (self.camera.height, self.camera.width), dtypes, "raw depth")
        with torch.cuda.device(self.dev):
            _capi.check(self._lib.segs_undistort_depth(C.byref(self._cam), int(src.dtype == torch.float32), self._p(src),
                                                       self.camera.inv_depth_factor, int(bool(hole_aware)), self._p(self.depth_map),
                                                       self._stream()), "segs_undistort_depth")
        return self.depth_map

    def debug_map(self) -> torch.Tensor:
        """(H, W, 2) float32: the source coordinates (mx, my) of every output pixel (a new tensor: a debugging call)."""
        out = torch.zeros((self.H, self.W, 2), dtype=torch.float32, device=self.dev)
        with torch.cuda.device(self.dev):
            _capi.check(self._lib.segs_debug_undistort_map(C.byref(self._cam), self._p(out), self._stream()), "segs_debug_undistort_map")
        return out
