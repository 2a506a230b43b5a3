"""CPU-side check of the rasterizer's argument marshalling: every builder of the host layer (rasterize_points._forward_args /
_backward_args, RasterEngine._forward_args / _backward_args) names the entry point it is meant to reach and returns as many
arguments as that entry point's ctypes prototype takes, each convertible under its bound type -- what a miscounted or misplaced
argument would otherwise turn into a ctypes.ArgumentError on the first GPU run.  4 Gaussians on a 16x16 image, CPU tensors; no
call into the library is made with the tuples.

Covered: the five reference-shaped wrappers' symbols and the engine's synchronising forward (both forms) and backward (all three).
Not covered: the engine's resident and projected forms -- their buffers hang off a pinned host allocation (pin_memory needs a
device), so they cannot be built here without faking the engine's state; tests/test_raster_gpu.py, test_depth_render_gpu.py and
test_camera_grad_gpu.py call every one of them.
"""
import ctypes as C

import pytest
import torch

from segs_slam_amd import _capi, rasterize_points as rp
from segs_slam_amd.raster_engine import RasterEngine

P, H, W = 4, 16, 16
E = torch.empty(0)


@pytest.fixture(scope="module", autouse=True)
def _library():
    _capi.build()       # RasterEngine loads the library (and asks it for the camera scratch size) in its constructor


def _check(name, args, want, structs=()):
    """`args` leaves out the stream; num_rendered, the only argument behind it, is the last one of a synchronising forward.
    `structs`: the types the trailing struct pointers (in front of the stream) must point to, None for a NULL pointer."""
    assert name == want
    tail = args[:-1] if name in ("segs_rasterize_forward", "segs_rasterize_forward_depth") else args
    for arg, struct in zip(tail[len(tail) - len(structs):], structs):
        assert (arg is None) if struct is None else isinstance(arg._obj, struct), (name, arg, struct)
    argtypes = list(_capi.SYMBOLS[name][1])
    assert len(args) + 1 == len(argtypes)
    del argtypes[-2 if name in ("segs_rasterize_forward", "segs_rasterize_forward_depth") else -1]      # the stream
    for i, (argtype, arg) in enumerate(zip(argtypes, args)):
        try:
            argtype.from_param(arg)
        except (TypeError, C.ArgumentError) as e:
            pytest.fail(f"{name}: argument {i} ({arg!r}) does not convert to {argtype.__name__}: {e}")


def _callbacks():
    return [_capi.ALLOC_FN(lambda _ctx, _nbytes: 0) for _ in range(3)]


def _inputs():
    """background, means3D, sh (absent), colors, opacity, scales, rotations, cov3D_precomp (absent), viewmatrix, projmatrix, campos"""
    return [torch.zeros(3), torch.zeros(P, 3), E, torch.zeros(P, 3), torch.zeros(P, 1), torch.ones(P, 3), torch.ones(P, 4), E,
            torch.eye(4), torch.eye(4), torch.zeros(3)]


@pytest.mark.parametrize("with_maps", [False, True])
def test_wrapper_forward(with_maps):
    maps = (torch.zeros(H, W), torch.zeros(H, W)) if with_maps else ()
    name, args = rp._forward_args(_inputs(), *_callbacks(), 0, 1.0, 1.0, 1.0, False, torch.zeros(3, H, W),
                                  torch.zeros(P, dtype=torch.int32), maps, C.c_int(0))
    _check(name, args, "segs_rasterize_forward_depth" if with_maps else "segs_rasterize_forward",
           (_capi.DepthOutputs,) if with_maps else ())
    assert isinstance(args[-1]._obj, C.c_int) and args[6:9] == (P, 0, 0) and args[10:12] == (W, H)


@pytest.mark.parametrize("form", ["plain", "depth", "depth_null", "camera"])
def test_wrapper_backward(form):
    tensors = _inputs()
    del tensors[4]                          # the backward takes no opacity ...
    tensors.append(torch.zeros(3, H, W))    # ... and ends with dL_dout_color
    grads = [torch.zeros(P, n) for n in (3, 3, 1, 3, 6)] + [torch.zeros(P, 0, 3), torch.zeros(P, 3), torch.zeros(P, 4)]
    extra = {"plain": {}, "depth": dict(map_grads=(torch.zeros(H, W), None)), "depth_null": dict(map_grads=(None, None)),
             "camera": dict(map_grads=(None, torch.zeros(H, W)), camera=(torch.zeros(4, 4), torch.zeros(4, 4), torch.zeros(64)))}[form]
    name, args = rp._backward_args(tensors, torch.zeros(P, dtype=torch.int32), (torch.zeros(8), torch.zeros(8), torch.zeros(8)), 7, 0,
                                   1.0, 1.0, 1.0, grads, **extra)
    _check(name, args, {"plain": "segs_rasterize_backward", "depth": "segs_rasterize_backward_depth",
                        "depth_null": "segs_rasterize_backward_depth", "camera": "segs_rasterize_backward_camera"}[form],
           {"plain": (), "camera": (_capi.DepthGrads, _capi.CameraGrads)}.get(form, (_capi.DepthGrads,)))
    assert args[:4] == (P, 0, 0, 7) and args[5:7] == (W, H)


def _engine(**kw):
    eng = RasterEngine(P, W, H, "cpu", **kw)
    bg, m3, _sh, col, opa, sca, rot, _cov, view, proj, cam = _inputs()
    return eng, (bg, m3, col, opa, sca, rot, view, proj, cam, 1.0, 1.0, 1.0)


@pytest.mark.parametrize("render_depth", [False, True])
def test_engine_synchronising_forward(render_depth):
    eng, last = _engine(render_depth=render_depth)
    name, args = eng._forward_args(*_callbacks(), C.c_int(0), *last)
    _check(name, args, "segs_rasterize_forward_depth" if render_depth else "segs_rasterize_forward",
           (_capi.DepthOutputs,) if render_depth else ())


@pytest.mark.parametrize("form", ["plain", "depth", "camera", "camera_with_maps"])
def test_engine_synchronising_backward(form):
    eng, last = _engine(render_depth=form != "plain", camera_grad=form.startswith("camera"))
    eng._last = last
    assert eng._last_resident is False
    maps = _capi.DepthGrads(torch.zeros(H, W).data_ptr(), None) if form in ("depth", "camera_with_maps") else None
    name, args = eng._backward_args(torch.zeros(3, H, W), maps, eng._camera_out)
    # without a map gradient the camera form gets a NULL depth struct
    _check(name, args, "segs_rasterize_backward" + {"plain": "", "depth": "_depth"}.get(form, "_camera"),
           {"plain": (), "depth": (_capi.DepthGrads,), "camera": (None, _capi.CameraGrads),
            "camera_with_maps": (_capi.DepthGrads, _capi.CameraGrads)}[form])
