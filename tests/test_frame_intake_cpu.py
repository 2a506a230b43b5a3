"""The frame intake without a GPU: the two references of tests/_frame_intake_ref.py against each other, the pyramid sizes, the
settings reader and the argument validation of the host mirror and of the C entry points (which refuse before any launch).

Tolerance of the float32 map (measured here, fixed in tests/_frame_intake_ref.py and DESIGN.md 3j): the largest
|mx_a - mx_b| + |my_a - my_b| over every listed camera is 3.38 units of 2^-24 max(in_w, in_h) pixels; tol_px is twice that,
6.76 * 2^-24 * max(in_w, in_h), i.e. 2.6e-4 px at 640x480.  Values then differ by at most tol_px x (spread of the taps) plus the
float32 rounding of the four-term sum (1e-6 for values in [0, 1])."""
import ctypes as C

import numpy as np
import pytest

from tests import _frame_intake_ref as ref

CAMERAS = [c.name for c in ref.all_cameras()]
SUM_ROUNDING = 1e-6          # four products and three sums of values in [0, 1]: below 8 x 2^-24 = 4.8e-7


def test_float32_map_error_is_what_the_tolerance_says():
    worst = 0.0
    for c in ref.all_cameras():
        e = ref.map_error_px(c)
        units = e / (2.0 ** -24 * max(c.in_w, c.in_h))
        print(f"{c.name}: max |a - b| = {e:.3e} px = {units:.2f} units of 2^-24 max(in_w, in_h)")
        worst = max(worst, units)
        if c.name.startswith("identity"):
            assert e == 0.0, c.name                  # every float32 step of the identity camera's map is exact
    print(f"worst: {worst:.3f} units; TOL_UNITS = {ref.TOL_UNITS}")
    assert abs(ref.TOL_UNITS - 2.0 * worst) <= 0.02, worst           # the tolerance IS twice the measured error (two decimals)
    assert ref.TOL_UNITS <= 16.0                                     # and a small multiple of 2^-24 max(in_w, in_h): the operation count


def test_the_distorting_cameras_leave_the_source_through_all_four_borders():
    flagged = [c for c in ref.all_cameras() if c.all_borders]
    assert {c.name for c in flagged} == {"tum-37x29-41x23"}
    for c in flagged + [ref.tum_full()]:
        for mx, my in (ref.map_f64(c), ref.map_f32(c)):
            assert (mx < -1).any() and (mx > c.in_w).any() and (my < -1).any() and (my > c.in_h).any(), c.name
    for c in ref.all_cameras():                                      # and no case is vacuous: part of every output sees the source
        m = ref.mask_f64(c)
        assert (m > 0).mean() > 0.1, c.name
        if not c.name.startswith("identity"):
            assert ((m > 0) & (m < 1)).any(), c.name


@pytest.mark.parametrize("name", CAMERAS)
def test_restatement_against_the_float64_chain(name):
    c = ref.camera(name)
    tol = ref.tol_px(c.in_w, c.in_h)
    for channels in (3, 1):
        src = ref.frame_u8(c.in_w, c.in_h, channels)
        a, gray = ref.image_f32(c, src)
        b = ref.image_f64(c, src)
        for ch in range(channels):
            bound = tol * ref.tap_spread(c, src[..., ch]) / 255.0 + SUM_ROUNDING
            err = np.abs(a[ch].astype(np.float64) - b[ch])
            assert (err <= bound).all(), (name, channels, ch, float(err.max()))
        # the grey bytes: within one step of the float64 grey (rounding at a half can go either way)
        g64 = (0.299 * b[0] + 0.587 * b[1] + 0.114 * b[2]) if channels == 3 else b[0]
        assert np.abs(gray.astype(np.float64) - 255.0 * g64).max() <= 0.5 + 255.0 * (tol + 2 * SUM_ROUNDING), name
    ma, mb = ref.mask_f32(c), ref.mask_f64(c)
    bound = tol * ref.tap_spread(c, np.ones((c.in_h, c.in_w))) + SUM_ROUNDING
    assert (np.abs(ma.astype(np.float64) - mb) <= bound).all(), name
    assert ma.min() >= 0.0 and ma.max() <= 1.0 + 1e-6

    raw = ref.depth_u16(c.in_w, c.in_h)
    metres = raw.astype(np.float64) * ref.INV_FACTOR
    scale = max(1.0, float(metres.max()))
    bound = tol * ref.tap_spread(c, metres) + SUM_ROUNDING * scale
    za, zb = ref.depth_f32(c, raw, ref.INV_FACTOR, False), ref.depth_f64(c, raw, ref.INV_FACTOR, False)
    assert (np.abs(za.astype(np.float64) - zb) <= bound).all(), name
    # hole-aware: discontinuous at the grid lines, so pixels within tol_px of one (and whose two maps differ at all) may be left out
    ha, hb = ref.depth_f32(c, raw, ref.INV_FACTOR, True), ref.depth_f64(c, raw, ref.INV_FACTOR, True)
    (ax, ay), (bx, by) = ref.map_f32(c), ref.map_f64(c)
    with np.errstate(invalid="ignore"):
        differ = ~((ax.astype(np.float64) == bx) & (ay.astype(np.float64) == by))
    out = ref.near_grid_line(c, tol) & differ
    assert out.mean() < 0.02, (name, float(out.mean()))
    assert (np.abs(ha.astype(np.float64) - hb) <= bound)[~out].all(), name
    assert ((ha == 0) | (ha == za)).all() and (ha == 0).sum() >= (za == 0).sum()       # holes only ever remove
    if not name.startswith("identity"):
        assert ((ha == 0) & (za != 0)).any(), name                   # the inputs do have holes that the plain remap averages in


LEVEL_SOURCES = [("tum-37x29-41x23", 2), ("tum-37x29-41x23", 3), ("tum-67x5-67x5", 2), ("tum-67x5-67x5", 3), ("tum-640x480", 2)]


@pytest.mark.parametrize("name,n", LEVEL_SOURCES)
def test_resize_restatement_against_interpolate(name, n):
    from segs_slam_amd.frame_intake import pyramid_sizes
    c = ref.camera(name)
    img, _ = ref.image_f32(c, ref.frame_u8(c.in_w, c.in_h, 3))
    mask = ref.mask_f32(c)[None]
    tol = ref.tol_px(c.out_w, c.out_h)
    sizes = [s for s in pyramid_sizes(c.out_w, c.out_h, n) if min(s) > 0]
    assert sizes
    for w, h in sizes:
        for src in (img, mask):
            a, b = ref.resize_f32(src, w, h), ref.resize_f64(src, w, h)
            assert a.shape == (src.shape[0], h, w)
            bound = tol * ref.resize_spread(src, w, h) + SUM_ROUNDING
            assert (np.abs(a.astype(np.float64) - b) <= bound).all(), (name, w, h)


def test_pyramid_sizes_are_the_reference_formula():
    """camera.width_ * pow(0.5f, num_sub_levels - l), truncated into a size_t (src/gaussian_mapper.cpp:147-150, 329-331)."""
    from segs_slam_amd.frame_intake import pyramid_sizes
    want = {(640, 480): [(80, 60), (160, 120), (320, 240)], (1200, 680): [(150, 85), (300, 170), (600, 340)],
            (1241, 376): [(155, 47), (310, 94), (620, 188)]}
    for (w, h), levels in want.items():
        for n in (1, 2, 3):
            assert pyramid_sizes(w, h, n) == levels[3 - n:], (w, h, n)
            # the formula itself, in the reference's types
            assert pyramid_sizes(w, h, n) == [(int(np.float32(w) * np.float32(0.5 ** (n - l))), int(np.float32(h) * np.float32(0.5 ** (n - l))))
                                              for l in range(n)]                                       # noqa: E741
        assert pyramid_sizes(w, h, 0) == []
    assert pyramid_sizes(67, 5, 3) == [(8, 0), (16, 1), (33, 2)]      # the formula can give an empty level; FrameIntake refuses it
    for bad in ((0, 4, 1), (4, 0, 1), (4, 4, -1)):
        with pytest.raises(ValueError):
            pyramid_sizes(*bad)


def test_from_settings_on_the_fixture():
    from segs_slam_amd.frame_intake import CameraModel
    table = ref.settings()
    assert sorted(table) == ["cfg/ORB_SLAM3/RGB-D/RealCamera/realsense_d455_rgbd.yaml", "cfg/ORB_SLAM3/RGB-D/Replica/room0.yaml",
                             "cfg/ORB_SLAM3/RGB-D/TUM/tum_freiburg2_xyz.yaml"]
    tum = CameraModel.from_settings(table[ref.TUM])
    assert (tum.width, tum.height, tum.out_width, tum.out_height) == (640, 480, 640, 480)
    assert (tum.fx, tum.fy, tum.cx, tum.cy) == (520.908620, 521.007327, 325.141442, 249.701764)
    assert (tum.k1, tum.k2, tum.p1, tum.p2, tum.k3) == (0.231222, -0.784899, -0.003257, -0.000105, 0.917205)
    assert tum.depth_map_factor == 5208.0 and tum.baseline == 0.0767 and tum.R is None
    assert tum.inv_depth_factor == float(np.float32(1.0 / 5208.0))
    assert tum.new_intrinsics == (tum.fx, tum.fy, tum.cx, tum.cy)          # the reference's default new camera
    d455 = CameraModel.from_settings(table["cfg/ORB_SLAM3/RGB-D/RealCamera/realsense_d455_rgbd.yaml"])
    assert (d455.width, d455.height, d455.k3, d455.depth_map_factor) == (1280, 720, -0.0191423, 1000.0)
    room = CameraModel.from_settings(table["cfg/ORB_SLAM3/RGB-D/Replica/room0.yaml"])
    assert (room.width, room.height, room.fx, room.cx, room.k3, room.depth_map_factor) == (1200, 680, 600.0, 599.5, 0.0, 6553.5)
    # the struct the kernels get: every value rounded once to float32, R^-1 = I
    cs = tum.c_struct()
    assert (cs.in_w, cs.in_h, cs.out_w, cs.out_h) == (640, 480, 640, 480)
    assert cs.fx == float(np.float32(520.908620)) and cs.k3 == float(np.float32(0.917205)) and cs.nfy == float(np.float32(521.007327))
    assert list(cs.rinv) == [1, 0, 0, 0, 1, 0, 0, 0, 1]
    # an absent key reads as 0; a DepthMapFactor of 0 divides nothing
    few = CameraModel.from_settings({"Camera.width": 8, "Camera.height": 4, "Camera1.fx": 5.0, "Camera1.fy": 5.0})
    assert (few.cx, few.k1, few.baseline, few.depth_map_factor, few.inv_depth_factor) == (0.0, 0.0, 0.0, 0.0, 1.0)
    over = CameraModel.from_settings(table[ref.TUM], new_width=320, new_height=240, new_fx=260.0, new_fy=260.0, new_cx=160.0, new_cy=120.0)
    assert (over.out_width, over.out_height, over.new_intrinsics) == (320, 240, (260.0, 260.0, 160.0, 120.0))
    with pytest.raises(ValueError, match="not supported"):
        CameraModel.from_settings(dict(table[ref.TUM], **{"Camera.type": "KannalaBrandt8"}))
    with pytest.raises(ValueError, match="numeric"):
        CameraModel.from_settings(dict(table[ref.TUM], **{"Camera1.fx": "wide"}))
    with pytest.raises(ValueError):
        CameraModel.from_settings({})                                  # width 0


def test_the_host_struct_is_the_restatements_camera():
    from segs_slam_amd.frame_intake import CameraModel
    for c in ref.all_cameras():
        cs = CameraModel(**c.model_kwargs()).c_struct()
        assert (cs.in_w, cs.in_h, cs.out_w, cs.out_h) == (c.in_w, c.in_h, c.out_w, c.out_h)
        want = [np.float32(v) for v in c.K + c.dist] + list(c.rinv64().astype(np.float32).reshape(9)) + [np.float32(v) for v in c.newK]
        got = [cs.fx, cs.fy, cs.cx, cs.cy, cs.k1, cs.k2, cs.p1, cs.p2, cs.k3] + list(cs.rinv) + [cs.nfx, cs.nfy, cs.ncx, cs.ncy]
        assert [np.float32(v) for v in got] == want, c.name


def test_host_mirror_validation():
    from segs_slam_amd import frame_intake as fi
    ok = dict(width=8, height=4, fx=5.0, fy=5.0, cx=4.0, cy=2.0)
    fi.CameraModel(**ok)
    for bad in (dict(width=0), dict(height=fi.MAX_SIZE + 1), dict(new_width=0), dict(new_height=-3), dict(fx=float("nan")),
                dict(k2=float("inf")), dict(new_fx=0.0), dict(fy=0.0), dict(R=[[1, 0, 0], [0, 1, 0]]), dict(R=np.zeros((3, 3))),
                dict(R=[[1, 0, 0], [0, 1, 0], [0, 0, float("nan")]]), dict(depth_map_factor=float("nan"))):
        with pytest.raises(ValueError):
            fi.CameraModel(**dict(ok, **bad))
    fi.CameraModel(**dict(ok, fy=0.0, new_fy=3.0))                     # only the NEW focal lengths divide
    cam = fi.CameraModel(**ok)
    with pytest.raises(RuntimeError, match="GPU"):
        fi.FrameIntake(cam, "cpu")
    R = np.asarray(ref.rotation((0.3, 1.0, -0.4), 3.0))
    assert np.allclose(fi.CameraModel(**dict(ok, R=R)).rinv.reshape(3, 3), R.T, atol=1e-7)     # a rotation's inverse is its transpose


def test_c_entry_points_refuse_before_any_launch():
    """Every call below fails validation, so nothing is launched and no GPU is needed; the pointers are never dereferenced."""
    from segs_slam_amd import _capi
    from segs_slam_amd.frame_intake import CameraModel
    lib = _capi.lib()
    good = CameraModel(width=8, height=4, fx=5.0, fy=5.0, cx=4.0, cy=2.0).c_struct()
    p = C.c_void_p(4096)                                               # non-null, never used
    INVALID = -1                                                       # SEGS_ERR_INVALID_ARGUMENT

    def broken(**kw):
        c = CameraModel(width=8, height=4, fx=5.0, fy=5.0, cx=4.0, cy=2.0).c_struct()
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    cams = [broken(in_w=0), broken(in_h=8193), broken(out_w=-1), broken(out_h=0), broken(nfx=0.0), broken(nfy=0.0),
            broken(k1=float("nan")), broken(cx=float("inf"))]
    nan_r = broken()
    nan_r.rinv[4] = float("nan")
    cams.append(nan_r)
    for c in cams:
        assert lib.segs_undistort_u8(C.byref(c), 3, p, p, p, None) == INVALID
        assert lib.segs_undistort_depth(C.byref(c), 0, p, 1.0, 1, p, None) == INVALID
        assert lib.segs_undistort_mask(C.byref(c), p, None) == INVALID
        assert lib.segs_debug_undistort_map(C.byref(c), p, None) == INVALID
    assert b"frame intake" in lib.segs_last_error()
    g = C.byref(good)
    assert lib.segs_undistort_u8(None, 3, p, p, p, None) == INVALID
    for channels in (0, 2, 4):
        assert lib.segs_undistort_u8(g, channels, p, p, p, None) == INVALID
    assert lib.segs_undistort_u8(g, 3, None, p, p, None) == INVALID
    assert lib.segs_undistort_u8(g, 3, p, None, None, None) == INVALID
    assert lib.segs_undistort_depth(g, 2, p, 1.0, 0, p, None) == INVALID
    assert lib.segs_undistort_depth(g, 0, p, 1.0, 2, p, None) == INVALID
    assert lib.segs_undistort_depth(g, 0, p, float("nan"), 0, p, None) == INVALID
    assert lib.segs_undistort_depth(g, 0, None, 1.0, 0, p, None) == INVALID
    assert lib.segs_undistort_depth(g, 1, p, 1.0, 0, None, None) == INVALID
    assert lib.segs_undistort_mask(g, None, None) == INVALID
    assert lib.segs_debug_undistort_map(g, None, None) == INVALID
    one = (C.c_int * 1)(4)
    zero = (C.c_int * 1)(0)
    ptrs = (C.c_void_p * 1)(4096)
    null = (C.c_void_p * 1)(None)
    for args in ((2, 8, 4, p, 1, one, one, ptrs), (3, 0, 4, p, 1, one, one, ptrs), (3, 8, 8193, p, 1, one, one, ptrs),
                 (3, 8, 4, None, 1, one, one, ptrs), (3, 8, 4, p, 0, one, one, ptrs), (3, 8, 4, p, 9, one, one, ptrs),
                 (3, 8, 4, p, 1, zero, one, ptrs), (3, 8, 4, p, 1, one, zero, ptrs), (3, 8, 4, p, 1, one, one, null),
                 (3, 8, 4, p, 1, None, one, ptrs), (3, 8, 4, p, 1, one, None, ptrs), (3, 8, 4, p, 1, one, one, None)):
        assert lib.segs_resize_levels(*args, None) == INVALID, args
    assert b"segs_resize_levels" in lib.segs_last_error()
