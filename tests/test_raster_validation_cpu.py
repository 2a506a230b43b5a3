"""Argument validation of every rasterizer entry point of csrc/capi.hip, without a GPU: the library loads on any machine and each
check returns before the first HIP call, so the exact status and the exact segs_last_error() text of one call per check can be
pinned here -- and, where two checks could both fire, which one wins.  Device pointers are stood in for by one host buffer that
nothing dereferences.  No case may get past validation (there is no device memory behind the pointers): every call either fails
a check, or returns SEGS_OK through one of the early exits that precede all HIP calls.

segs_resident_projection_targets is host-only; its outputs are pinned as recorded numbers (offsets from the three buffers), which
catches a drift in the shared carve-up of the resident buffers or in the side of the depth sort that K1 writes its keys to."""
import ctypes as C

import pytest

from segs_slam_amd import _capi

OK, INVALID, ALLOC = 0, -1, -3
_HOST = (C.c_char * 4096)()
PTR = (C.addressof(_HOST) + 255) // 256 * 256          # a 256-byte aligned stand-in for every device pointer
_NUM_RENDERED = C.c_int(0)
TOO_WIDE = 16 * 0x10000                                   # 65 536 tile columns: one more than 16-bit tile coordinates hold

_alloc_calls = []


@_capi.ALLOC_FN
def _alloc_null(ctx, nbytes):
    _alloc_calls.append(nbytes)
    return 0


_NO_ALLOC = _capi.ALLOC_FN()       # a null function pointer


def _camera_grads(**over):
    f = dict(dL_dviewmatrix=PTR, dL_dprojmatrix=PTR, temp=PTR)
    f.update(over)
    return _capi.CameraGrads(f["dL_dviewmatrix"], f["dL_dprojmatrix"], f["temp"])


_GAUSS_FWD = dict(means3D=PTR, shs=None, colors_precomp=PTR, opacities=PTR, scales=PTR, scale_modifier=1.0, rotations=PTR,
                  cov3D_precomp=None)
_CAMERA = dict(viewmatrix=PTR, projmatrix=PTR, cam_pos=PTR, tan_fovx=0.5, tan_fovy=0.5)
_GRADS = dict(dL_dpix=PTR, dL_dmean2D=PTR, dL_dconic=PTR, dL_dopacity=PTR, dL_dcolor=PTR, dL_dmean3D=PTR, dL_dcov3D=PTR, dL_dsh=PTR,
              dL_dscale=PTR, dL_drot=PTR)
_RESIDENT = dict(geom_buffer=PTR, binning_buffer=PTR, image_buffer=PTR, capacity=8, geom_rows=4)

# name -> (parameter names in ABI order, arguments that pass every check: P = 4, a 16 x 16 image)
ENTRY = {}


def _entry(name, order, **defaults):
    order = order.split()
    assert sorted(order) == sorted(defaults), (name, set(order) ^ set(defaults))
    ENTRY[name] = (order, defaults)


_FWD = ("geometry_alloc geometry_ctx binning_alloc binning_ctx image_alloc image_ctx P D M background width height means3D shs "
        "colors_precomp opacities scales scale_modifier rotations cov3D_precomp viewmatrix projmatrix cam_pos tan_fovx tan_fovy "
        "prefiltered out_color radii %s stream num_rendered")
_FWD_ARGS = dict(geometry_alloc=_alloc_null, geometry_ctx=None, binning_alloc=_alloc_null, binning_ctx=None, image_alloc=_alloc_null,
                 image_ctx=None, P=4, D=0, M=0, background=PTR, width=16, height=16, prefiltered=0, out_color=PTR, radii=PTR, stream=None,
                 num_rendered=C.byref(_NUM_RENDERED), **_GAUSS_FWD, **_CAMERA)
_entry("segs_rasterize_forward", _FWD % "", **_FWD_ARGS)
_entry("segs_rasterize_forward_depth", _FWD % "depth_out", depth_out=None, **_FWD_ARGS)

_BWD = ("P D M R background width height means3D shs colors_precomp scales scale_modifier rotations cov3D_precomp viewmatrix "
        "projmatrix campos tan_fovx tan_fovy radii geom_buffer binning_buffer image_buffer dL_dpix dL_dmean2D dL_dconic dL_dopacity "
        "dL_dcolor dL_dmean3D dL_dcov3D dL_dsh dL_dscale dL_drot %s stream")
_BWD_ARGS = dict(P=4, D=0, M=0, R=8, background=PTR, width=16, height=16, means3D=PTR, shs=None, colors_precomp=PTR, scales=PTR,
                 scale_modifier=1.0, rotations=PTR, cov3D_precomp=None, viewmatrix=PTR, projmatrix=PTR, campos=PTR, tan_fovx=0.5,
                 tan_fovy=0.5, radii=PTR, geom_buffer=PTR, binning_buffer=PTR, image_buffer=PTR, stream=None, **_GRADS)
_entry("segs_rasterize_backward", _BWD % "", **_BWD_ARGS)
_entry("segs_rasterize_backward_depth", _BWD % "depth_grads", depth_grads=None, **_BWD_ARGS)
_entry("segs_rasterize_backward_camera", _BWD % "depth_grads camera_grads", depth_grads=None, camera_grads=None, **_BWD_ARGS)

_RFWD = ("geom_buffer binning_buffer image_buffer capacity geom_rows P D M background width height means3D shs colors_precomp "
         "opacities scales scale_modifier rotations cov3D_precomp viewmatrix projmatrix cam_pos tan_fovx tan_fovy out_color radii "
         "status %s stream")
_RFWD_ARGS = dict(P=4, D=0, M=0, background=PTR, width=16, height=16, out_color=PTR, radii=PTR, status=PTR, stream=None, **_RESIDENT,
                  **_GAUSS_FWD, **_CAMERA)
_entry("segs_rasterize_forward_resident", _RFWD % "", **_RFWD_ARGS)
_entry("segs_rasterize_forward_resident_depth", _RFWD % "depth_out", depth_out=None, **_RFWD_ARGS)

_PFWD = "geom_buffer binning_buffer image_buffer capacity geom_rows P background width height out_color status %s stream"
_PFWD_ARGS = dict(P=4, background=PTR, width=16, height=16, out_color=PTR, status=PTR, stream=None, **_RESIDENT)
_entry("segs_rasterize_forward_resident_projected", _PFWD % "", **_PFWD_ARGS)
_entry("segs_rasterize_forward_resident_projected_depth", _PFWD % "depth_out", depth_out=None, **_PFWD_ARGS)

_TARGETS = _capi.ProjectionTargets()
_entry("segs_resident_projection_targets", "geom_buffer binning_buffer image_buffer capacity geom_rows P width height radii status out",
       P=4, width=16, height=16, radii=None, status=PTR, out=C.addressof(_TARGETS), **_RESIDENT)

_RBWD = ("geom_buffer binning_buffer image_buffer capacity geom_rows P D M background width height means3D shs scales scale_modifier "
         "rotations cov3D_precomp viewmatrix projmatrix campos tan_fovx tan_fovy radii dL_dpix dL_dmean2D dL_dconic dL_dopacity "
         "dL_dcolor dL_dmean3D dL_dcov3D dL_dsh dL_dscale dL_drot %s stream")
_RBWD_ARGS = {k: v for k, v in _BWD_ARGS.items() if k not in ("R", "colors_precomp")}
_RBWD_ARGS.update(capacity=8, geom_rows=4)
_entry("segs_rasterize_backward_resident", _RBWD % "", **_RBWD_ARGS)
_entry("segs_rasterize_backward_resident_depth", _RBWD % "depth_grads", depth_grads=None, **_RBWD_ARGS)
_entry("segs_rasterize_backward_resident_camera", _RBWD % "depth_grads camera_grads", depth_grads=None, camera_grads=None, **_RBWD_ARGS)

_entry("segs_visible_filter", "P M width height means3D scales scale_modifier rotations cov3D_precomp viewmatrix projmatrix tan_fovx "
       "tan_fovy prefiltered radii stream", P=4, M=0, width=16, height=16, means3D=PTR, scales=PTR, scale_modifier=1.0, rotations=PTR,
       cov3D_precomp=None, viewmatrix=PTR, projmatrix=PTR, tan_fovx=0.5, tan_fovy=0.5, prefiltered=0, radii=PTR, stream=None)
_entry("segs_visible_filter_log_scales", "P width height means3D scaling_log stride rotations viewmatrix projmatrix tan_fovx tan_fovy "
       "radii stream", P=4, width=16, height=16, means3D=PTR, scaling_log=PTR, stride=6, rotations=PTR, viewmatrix=PTR, projmatrix=PTR,
       tan_fovx=0.5, tan_fovy=0.5, radii=PTR, stream=None)
_entry("segs_mark_visible", "P means3D viewmatrix projmatrix present stream", P=4, means3D=PTR, viewmatrix=PTR, projmatrix=PTR,
       present=PTR, stream=None)
_entry("segs_project2_image", "P D M width height means3D shs colors_precomp opacities scales scale_modifier rotations cov3D_precomp "
       "viewmatrix projmatrix cam_pos tan_fovx tan_fovy prefiltered out_color points_image radii stream", P=4, D=0, M=0, width=16,
       height=16, prefiltered=0, out_color=PTR, points_image=PTR, radii=PTR, stream=None, **_GAUSS_FWD, **_CAMERA)
_entry("segs_sort_pairs", "keys_in vals_in keys_out vals_out n end_bit temp stream", keys_in=PTR, vals_in=PTR, keys_out=PTR,
       vals_out=PTR, n=4, end_bit=40, temp=PTR, stream=None)
_entry("segs_debug_unpack_geometry", "geom_buffer P radii means2D conic_opacity depths tiles_touched point_offsets rgb stream",
       geom_buffer=PTR, P=4, radii=None, means2D=PTR, conic_opacity=PTR, depths=PTR, tiles_touched=PTR, point_offsets=None, rgb=None,
       stream=None)
_entry("segs_debug_unpack_binning", "binning_buffer geom_buffer P R width height keys_sorted point_list stream", binning_buffer=PTR,
       geom_buffer=PTR, P=4, R=8, width=16, height=16, keys_sorted=PTR, point_list=PTR, stream=None)
_entry("segs_debug_instance_values", "binning_buffer R values stream", binning_buffer=PTR, R=8, values=PTR, stream=None)
_entry("segs_debug_unpack_image", "image_buffer width height ranges final_T n_contrib stream", image_buffer=PTR, width=16, height=16,
       ranges=PTR, final_T=PTR, n_contrib=PTR, stream=None)
_DBWD = ("P width height means3D radii scales scale_modifier rotations cov3D_precomp viewmatrix projmatrix tan_fovx tan_fovy "
         "dL_dmean2D dL_dconic dL_dmean3D dL_dcov3D dL_dscale dL_drot %s stream")
_DBWD_ARGS = dict(P=4, width=16, height=16, means3D=PTR, radii=PTR, scales=PTR, scale_modifier=1.0, rotations=PTR, cov3D_precomp=None,
                  viewmatrix=PTR, projmatrix=PTR, tan_fovx=0.5, tan_fovy=0.5, dL_dmean2D=PTR, dL_dconic=PTR, dL_dmean3D=PTR,
                  dL_dcov3D=PTR, dL_dscale=PTR, dL_drot=PTR, stream=None)
_entry("segs_debug_preprocess_backward", _DBWD % "", **_DBWD_ARGS)
_entry("segs_debug_preprocess_backward_camera", _DBWD % "dL_dz camera_grads", dL_dz=None, camera_grads=None, **_DBWD_ARGS)

BAD_P_IMAGE = "bad P / image size"
BAD_SIZES = "bad sizes"
REQUIRED = "null required pointer"
NULL_PTR = "null pointer"
NEED_COLOURS = "need colors_precomp, or shs + cam_pos with (D+1)^2 <= M, D <= 3"
NEED_SHAPE = "need scales+rotations or cov3D_precomp"
TOO_LARGE = "image too large for 16-bit tile coordinates"
ROWS_RESIDENT = "geom_rows (rows the geometry buffer was sized for) must be >= P"
CAM_NULL = "segs_camera_grads: null field"
CAM_SH = "camera gradients need colors_precomp: the SH colours depend on campos, which they do not cover"
SH_PATH = "SH path needs campos, dL_dsh and M > 0"
NULL_GRAD = "null gradient output"
NEED_SHAPE_BWD = "need scales+rotations (+ their gradient outputs) or cov3D_precomp"

CASES = []   # (entry point, overrides, status, message or None)


def _fails(names, over, message, status=INVALID):
    for name in names.split():
        CASES.append((name, over, status, message))


def _each_null(names, params, message):
    for p in params.split():
        _fails(names, {p: None}, message)


SH_COLOURS = dict(colors_precomp=None, shs=PTR, D=1, M=4)     # a valid SH colour input, to be broken one field at a time

# ---- the synchronising forward, plain and depth
F = "segs_rasterize_forward segs_rasterize_forward_depth"
for callback in ("geometry_alloc", "binning_alloc", "image_alloc"):
    _fails(F, {callback: _NO_ALLOC}, "null allocator callback")
for bad in (dict(P=-1), dict(width=0), dict(height=-3)):
    _fails(F, bad, BAD_P_IMAGE)
_fails(F, dict(P=(1 << 28) + 1), "P exceeds 2^28 Gaussians (sort values carry a 4-bit quadrant mask)")
_each_null(F, "background out_color viewmatrix projmatrix num_rendered", REQUIRED)
_each_null(F, "means3D opacities", "null means3D/opacities")
for bad in (dict(colors_precomp=None), dict(SH_COLOURS, cam_pos=None), dict(SH_COLOURS, M=3), dict(SH_COLOURS, D=-1, M=16),
            dict(SH_COLOURS, D=4, M=32), dict(SH_COLOURS, D=0, M=0)):
    _fails(F, bad, NEED_COLOURS)
_each_null(F, "scales rotations", NEED_SHAPE)
for bad in (dict(width=TOO_WIDE), dict(height=TOO_WIDE)):
    _fails(F, bad, TOO_LARGE)
_fails(F, {}, "allocator callback returned null", ALLOC)      # every check passes; the (null) allocations come next
# the earlier check wins
_fails(F, dict(geometry_alloc=_NO_ALLOC, P=-1), "null allocator callback")
_fails(F, dict(P=-1, background=None), BAD_P_IMAGE)
_fails(F, dict(P=(1 << 28) + 1, background=None), "P exceeds 2^28 Gaussians (sort values carry a 4-bit quadrant mask)")
_fails(F, dict(out_color=None, means3D=None), REQUIRED)
_fails(F, dict(opacities=None, colors_precomp=None), "null means3D/opacities")
_fails(F, dict(colors_precomp=None, scales=None), NEED_COLOURS)
_fails(F, dict(rotations=None, width=TOO_WIDE), NEED_SHAPE)
_fails(F, dict(P=0, means3D=None, opacities=None, colors_precomp=None, scales=None, width=TOO_WIDE), TOO_LARGE)   # P = 0 needs no Gaussians

# ---- the resident forwards: with K1, and after the producer's K1 ("projected"), and the targets of that producer
RF = "segs_rasterize_forward_resident segs_rasterize_forward_resident_depth"
PF = "segs_rasterize_forward_resident_projected segs_rasterize_forward_resident_projected_depth"
T = "segs_resident_projection_targets"
ALL_RESIDENT = " ".join((RF, PF, T))
for bad in (dict(P=0), dict(P=-1), dict(capacity=0), dict(width=0), dict(height=0)):
    _fails(ALL_RESIDENT, bad, BAD_SIZES)
_fails(T, dict(out=None), BAD_SIZES)
_fails(ALL_RESIDENT, dict(geom_rows=3), ROWS_RESIDENT)
_fails(ALL_RESIDENT, dict(geom_rows=(1 << 28) + 1), "P exceeds 2^28 Gaussians")
_each_null(ALL_RESIDENT, "geom_buffer binning_buffer image_buffer status", REQUIRED)
_each_null(RF + " " + PF, "background out_color", REQUIRED)
_each_null(RF, "viewmatrix projmatrix means3D opacities", REQUIRED)
for bad in (dict(colors_precomp=None), dict(SH_COLOURS, cam_pos=None), dict(SH_COLOURS, M=3), dict(SH_COLOURS, D=4, M=32)):
    _fails(RF, bad, NEED_COLOURS)
_each_null(RF, "scales rotations", NEED_SHAPE)
for bad in (dict(width=TOO_WIDE), dict(height=TOO_WIDE)):
    _fails(ALL_RESIDENT, bad, TOO_LARGE)
# bad sizes before geom_rows >= P before the 2^28 limit before null pointers before the inputs of K1 before the tile grid
_fails(ALL_RESIDENT, dict(capacity=0, geom_rows=3, geom_buffer=None), BAD_SIZES)
_fails(ALL_RESIDENT, dict(geom_rows=3, status=None), ROWS_RESIDENT)
_fails(ALL_RESIDENT, dict(P=(1 << 28) + 2, geom_rows=(1 << 28) + 1), ROWS_RESIDENT)
_fails(ALL_RESIDENT, dict(geom_rows=(1 << 28) + 1, image_buffer=None), "P exceeds 2^28 Gaussians")
_fails(ALL_RESIDENT, dict(binning_buffer=None, width=TOO_WIDE), REQUIRED)
_fails(RF, dict(means3D=None, colors_precomp=None), REQUIRED)
_fails(RF, dict(colors_precomp=None, rotations=None), NEED_COLOURS)
_fails(RF, dict(scales=None, height=TOO_WIDE), NEED_SHAPE)

# ---- the backwards: synchronising and resident, plain, depth and camera
SB = "segs_rasterize_backward segs_rasterize_backward_depth segs_rasterize_backward_camera"
RB = "segs_rasterize_backward_resident segs_rasterize_backward_resident_depth segs_rasterize_backward_resident_camera"
CAM_B = "segs_rasterize_backward_camera segs_rasterize_backward_resident_camera"
B = SB + " " + RB
for bad in (dict(P=-1), dict(width=0), dict(height=0)):
    _fails(B, bad, BAD_SIZES)
_fails(SB, dict(R=-1), BAD_SIZES)
_fails(RB, dict(capacity=-1), BAD_SIZES)
_fails(RB, dict(geom_rows=3), "geom_rows must be >= P")
_fails(B, dict(P=0, means3D=None, geom_buffer=None), None, OK)     # no Gaussians: nothing to do, before any pointer is looked at
SH_BWD = dict(shs=PTR, D=1, M=4)
for bad in (dict(SH_BWD, campos=None), dict(SH_BWD, dL_dsh=None), dict(SH_BWD, M=0)):
    _fails(B, bad, SH_PATH)
_each_null(B, "geom_buffer binning_buffer image_buffer dL_dpix background means3D viewmatrix projmatrix", REQUIRED)
_each_null(B, "dL_dmean2D dL_dopacity dL_dcolor dL_dmean3D", NULL_GRAD)
_fails(B, dict(cov3D_precomp=PTR, dL_dcov3D=None), NULL_GRAD)
_each_null(B, "scales rotations dL_dscale dL_drot", NEED_SHAPE_BWD)
_fails(RB, dict(capacity=-1, geom_rows=3), BAD_SIZES)
_fails(RB, dict(geom_rows=3, means3D=None), "geom_rows must be >= P")
_fails(B, dict(SH_BWD, campos=None, dL_dpix=None), SH_PATH)
_fails(B, dict(image_buffer=None, dL_dcolor=None), REQUIRED)
_fails(B, dict(dL_dopacity=None, scales=None), NULL_GRAD)
# the camera struct is checked right after the sizes, ahead of the "no Gaussians" exit (P and R stay positive whenever the struct is
# whole: without Gaussians or instances the backward would zero-fill the two matrices, a HIP call)
for field in ("dL_dviewmatrix", "dL_dprojmatrix", "temp"):
    _fails(CAM_B, dict(camera_grads=(field,)), CAM_NULL)
_fails(CAM_B, dict(camera_grads=("temp",), P=0), CAM_NULL)
_fails(CAM_B, dict(camera_grads=("temp",), width=0), BAD_SIZES)
_fails(CAM_B, dict(SH_BWD, camera_grads=()), CAM_SH)
_fails(CAM_B, dict(SH_BWD, camera_grads=(), campos=None), CAM_SH)
_fails(CAM_B, dict(camera_grads=(), means3D=None), REQUIRED)
_fails(CAM_B, dict(camera_grads=(), dL_drot=None), NEED_SHAPE_BWD)

# ---- visible filters, mark_visible, project2_image, sort_pairs
VF, VL = "segs_visible_filter", "segs_visible_filter_log_scales"
for bad in (dict(P=-1), dict(width=0), dict(height=0)):
    _fails(VF + " " + VL + " segs_project2_image", bad, BAD_SIZES)
_fails(VF + " " + VL + " segs_project2_image", dict(P=0, means3D=None, radii=None), None, OK)
_each_null(VF + " " + VL, "means3D viewmatrix projmatrix radii", REQUIRED)
_each_null(VF, "scales rotations", NEED_SHAPE)
_fails(VF, dict(radii=None, scales=None), REQUIRED)
for bad in (dict(stride=2), dict(scaling_log=None), dict(rotations=None), dict(stride=0, P=-1)):
    _fails(VL, bad, "need log-scales (stride >= 3) and rotations")
_fails("segs_mark_visible", dict(P=-1), "bad P")
_fails("segs_mark_visible", dict(P=0, means3D=None), None, OK)
_each_null("segs_mark_visible", "means3D viewmatrix present", REQUIRED)
for bad in (dict(colors_precomp=None), dict(SH_COLOURS, cam_pos=None), dict(SH_COLOURS, M=0)):
    _fails("segs_project2_image", bad, "need colors_precomp or shs + cam_pos")
_each_null("segs_project2_image", "means3D opacities viewmatrix projmatrix out_color points_image radii", REQUIRED)
_fails("segs_project2_image", dict(colors_precomp=None, means3D=None), "need colors_precomp or shs + cam_pos")
for bad in (dict(n=-1), dict(end_bit=0), dict(end_bit=65), dict(n=-1, keys_in=None)):
    _fails("segs_sort_pairs", bad, "bad n / end_bit")
_fails("segs_sort_pairs", dict(n=0, temp=None), None, OK)
_each_null("segs_sort_pairs", "keys_in vals_in keys_out vals_out temp", NULL_PTR)

# ---- debug entry points
_fails("segs_debug_unpack_geometry", dict(P=0, geom_buffer=None), None, OK)
_each_null("segs_debug_unpack_geometry", "geom_buffer means2D conic_opacity depths tiles_touched", NULL_PTR)
_fails("segs_debug_unpack_binning", dict(R=0, binning_buffer=None), None, OK)
_each_null("segs_debug_unpack_binning", "binning_buffer geom_buffer", NULL_PTR)
_fails("segs_debug_unpack_binning", dict(P=0), NULL_PTR)               # the 64-bit keys are rebuilt from the geometry buffer
_fails("segs_debug_unpack_binning", dict(keys_sorted=None, point_list=None, geom_buffer=None), None, OK)   # nothing asked for
_fails("segs_debug_instance_values", dict(R=0, values=None), None, OK)
_each_null("segs_debug_instance_values", "binning_buffer values", NULL_PTR)
_fails("segs_debug_unpack_image", dict(image_buffer=None), NULL_PTR)
_fails("segs_debug_unpack_image", dict(ranges=None, final_T=None, n_contrib=None), None, OK)               # nothing asked for
DB = "segs_debug_preprocess_backward segs_debug_preprocess_backward_camera"
_fails(DB, dict(P=0, means3D=None), None, OK)
_each_null(DB, "means3D radii viewmatrix projmatrix dL_dmean2D dL_dconic dL_dmean3D dL_dcov3D", NULL_PTR)
for field in ("dL_dviewmatrix", "dL_dprojmatrix", "temp"):
    _fails("segs_debug_preprocess_backward_camera", dict(camera_grads=(field,)), CAM_NULL)
_fails("segs_debug_preprocess_backward_camera", dict(camera_grads=("temp",), P=0), CAM_NULL)
_fails("segs_debug_preprocess_backward_camera", dict(camera_grads=(), dL_dz=PTR, radii=None), NULL_PTR)


def _case_id(case):
    name, over, status, _ = case
    sizes = ("P", "D", "M", "R", "width", "height", "capacity", "geom_rows", "stride", "n", "end_bit")
    what = ",".join(f"{k}={v}" if k in sizes else f"{k}[{'+'.join(v)}]" if isinstance(v, tuple) else k for k, v in over.items())
    return f"{name[5:]}-{what or 'valid'}-{status}"


def test_every_rasterizer_entry_point_of_the_header_is_covered():
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "segs_raster.h")).read()
    declared = set(re.findall(r"^int (segs_[a-z0-9_]+)\(", text, flags=re.M))
    host_only = {"segs_debug_geometry_layout", "segs_profile_begin", "segs_profile_end", "segs_profile_kernel_count", "segs_profile_query"}
    assert declared - host_only == set(ENTRY)
    assert {c[0] for c in CASES} == set(ENTRY)


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_validation_status_and_message(case):
    name, over, status, message = case
    order, defaults = ENTRY[name]
    assert set(over) <= set(order)
    args = dict(defaults)
    args.update(over)
    keep = []
    if isinstance(args.get("camera_grads"), tuple):      # a tuple names the fields of the struct to leave null
        cam = _camera_grads(**{f: None for f in args["camera_grads"]})
        keep.append(cam)
        args["camera_grads"] = C.addressof(cam)
    lib = _capi.lib()
    del _alloc_calls[:]
    got = getattr(lib, name)(*[args[p] for p in order])
    assert got == status
    if status != OK:
        assert lib.segs_last_error() == message.encode()
    # only the case that passes every check of the synchronising forward gets as far as its (null) allocations: geometry and image
    assert len(_alloc_calls) == (2 if status == ALLOC else 0)


# (P, geom_rows, capacity, W, H, raster flags, bytes the three buffers are off 256-byte alignment) -> the six pointers as offsets
# from geom_buffer / binning_buffer / image_buffer / status, num_tiles, flags.  Recorded numbers, not a restatement of gs_layout.h.
KEEP_DEAD = 2           # SEGS_RASTER_KEEP_DEAD_INSTANCES
TARGETS = [
    ((4, 4, 8, 16, 16, 0, 0), (0, 768, 2048, 26368, 0, 8, 1, 0x80000000)),
    ((257, 300, 5000, 33, 17, 0, 0), (0, 25344, 47616, 180992, 0, 8, 6, 0x80000000)),
    ((4, 4, 8, 16, 16, KEEP_DEAD, 0), (0, 768, 2048, 26368, 0, 8, 1, 0)),
    ((257, 300, 5000, 33, 17, 0, 8), (248, 25592, 47864, 181240, 248, 8, 6, 0x80000000)),
]


@pytest.mark.parametrize("sizes,expected", TARGETS, ids=["-".join(map(str, t[0])) for t in TARGETS])
def test_projection_targets_are_pinned(sizes, expected):
    P, rows, capacity, W, H, flags, off = sizes
    lib = _capi.lib()
    geom, binning, image, status = PTR + off, PTR + 1024 + off, PTR + 2048 + off, PTR + 3072
    out = _capi.ProjectionTargets()
    with _capi.raster_flags(flags):
        assert lib.segs_resident_projection_targets(geom, binning, image, capacity, rows, P, W, H, None, status, C.byref(out)) == OK
    got = (out.records - geom, out.radii - geom, out.tiles_touched - geom, out.depth_keys - binning, out.tile_ranges - image,
           out.depth_overflow - status, out.num_tiles, out.flags)
    assert got == expected
    radii = PTR + 512                                      # the caller's own radii are passed through
    assert lib.segs_resident_projection_targets(geom, binning, image, capacity, rows, P, W, H, radii, status, C.byref(out)) == OK
    assert out.radii == radii
