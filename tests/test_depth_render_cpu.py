"""CPU-side checks of the depth / alpha maps (segs_rasterize_*_depth, include/segs_raster.h): the library exports the five
twins, the ctypes table binds each with the header's argument count (the entry point it extends plus one struct pointer in
front of `stream`), and the Python paths refuse CPU tensors the way the plain ones do -- there is no CPU fallback."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXTENDED = ("segs_rasterize_forward", "segs_rasterize_backward", "segs_rasterize_forward_resident",
            "segs_rasterize_forward_resident_projected", "segs_rasterize_backward_resident")


def _header_params():
    text = open(os.path.join(ROOT, "include", "segs_raster.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for m in re.finditer(r"\b(segs_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", text):
        out[m.group(1)] = [" ".join(p.split()) for p in m.group(2).split(",")]
    return out


def test_depth_twins_are_exported_and_bound_with_the_header_argument_counts():
    from segs_slam_amd import _capi
    _capi.build()
    lib = _capi.lib()
    params = _header_params()
    for base in EXTENDED:
        twin = base + "_depth"
        assert hasattr(lib, twin), twin
        p_base, p_twin = params[base], params[twin]
        assert len(p_twin) == len(p_base) + 1, twin
        at = p_base.index("void* stream")
        struct = "segs_depth_grads" if "backward" in base else "segs_depth_outputs"
        assert p_twin[at].startswith(f"const {struct}*"), (twin, p_twin[at])
        assert [p.split()[-1] for p in p_twin[:at] + p_twin[at + 1:]] == [p.split()[-1] for p in p_base], twin
        res, args = _capi.SYMBOLS[twin]
        assert len(args) == len(p_twin), twin
        assert args[:at] + args[at + 1:] == _capi.SYMBOLS[base][1], twin
        assert res == _capi.SYMBOLS[base][0]


def test_depth_struct_layouts():
    from segs_slam_amd import _capi
    assert [f for f, _ in _capi.DepthOutputs._fields_] == ["depth", "alpha"]
    assert [f for f, _ in _capi.DepthGrads._fields_] == ["dL_ddepth", "dL_dalpha"]
    assert _capi.DepthOutputs().depth is None and _capi.DepthGrads().dL_dalpha is None   # zero-initialised = NULL fields


def test_depth_paths_refuse_cpu_tensors():
    from segs_slam_amd.gaussian_rasterizer import GaussianRasterizationSettings, rasterizeGaussiansWithDepth
    from segs_slam_amd import rasterize_points as rp
    from segs_slam_amd.raster_engine import RasterEngine
    e = torch.empty(0)
    rs = GaussianRasterizationSettings(16, 16, 1.0, 1.0, torch.zeros(3), 1.0, torch.eye(4), torch.eye(4), 0, torch.zeros(3), False)
    with pytest.raises(RuntimeError, match="GPU"):
        rasterizeGaussiansWithDepth(torch.zeros(4, 3), torch.zeros(4, 3), e, torch.zeros(4, 3), torch.zeros(4, 1), torch.zeros(4, 3),
                                    torch.zeros(4, 4), e, rs)
    with pytest.raises(RuntimeError, match="GPU"):
        rp.RasterizeGaussiansDepthCUDA(torch.zeros(3), torch.zeros(4, 3), torch.zeros(4, 3), torch.zeros(4, 1), torch.zeros(4, 3),
                                       torch.zeros(4, 4), 1.0, e, torch.eye(4), torch.eye(4), 1.0, 1.0, 16, 16, e, 0, torch.zeros(3),
                                       False)
    with pytest.raises(RuntimeError):
        rp.RasterizeGaussiansDepthCUDA(e, torch.zeros(4, 2), e, e, e, e, 1.0, e, e, e, 1.0, 1.0, 8, 8, e, 0, e, False)
    eng = RasterEngine(4, 16, 16, "cpu", render_depth=True)
    assert eng.out_depth.shape == (16, 16) and eng.out_alpha.shape == (16, 16)
    with pytest.raises(AssertionError):
        eng.forward(torch.zeros(3), torch.zeros(4, 3), torch.zeros(4, 3), torch.zeros(4, 1), torch.zeros(4, 3), torch.zeros(4, 4),
                    torch.eye(4), torch.eye(4), torch.zeros(3), 1.0, 1.0)
    plain = RasterEngine(4, 16, 16, "cpu")
    assert plain.out_depth is None and plain.out_alpha is None and not plain.render_depth
