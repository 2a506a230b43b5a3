"""CPU-side checks of the drop-in boundary: the C-ABI library builds, loads and exports every symbol
that include/segs_raster.h declares (no compute calls without a GPU), and the host mirror fails loudly
instead of falling back to a CPU path."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    names = set()
    for hdr in sorted(os.listdir(os.path.join(ROOT, "include"))):
        text = open(os.path.join(ROOT, "include", hdr)).read()
        text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
        names |= set(re.findall(r"\b(segs_[a-z0-9_]+)\s*\(", text))
    return sorted(names - {"segs_alloc_fn"})


def test_library_exports_every_declared_symbol():
    from segs_slam_amd import _capi
    _capi.build()
    lib = _capi.lib()
    declared = _declared_symbols()
    assert len(declared) >= 14
    for name in declared:
        assert hasattr(lib, name), name
        assert name in _capi.SYMBOLS, f"{name} has no ctypes prototype"
    assert sorted(_capi.SYMBOLS) == declared


def test_frequency_level_limit_matches_the_header():
    """FusedFrequencyLoss refuses scale counts by the library's SEGS_FREQ_MAX_LEVELS (include/segs_train.h), and that limit
    takes every Mapper.scale_num of the shipped configurations with the frequency regulariser on (2 to 5)."""
    import json
    from segs_slam_amd import frequency_loss, mapper_config as mc
    text = open(os.path.join(ROOT, "include", "segs_train.h")).read()
    m = re.search(r"^#define\s+SEGS_FREQ_MAX_LEVELS\s+(\d+)\b", text, flags=re.M)
    assert m, "SEGS_FREQ_MAX_LEVELS not found"
    assert frequency_loss.MAX_LEVELS == int(m.group(1))
    with open(os.path.join(ROOT, "tests", "golden", "mapper_cfg_values.json")) as f:
        shipped = json.load(f)
    counts = {mc.mapper_config_from_values(v, k).scale_num for k, v in shipped.items()
              if mc.mapper_config_from_values(v, k).use_frequency_regularization}
    assert counts == {2, 3, 4, 5} and max(counts) <= frequency_loss.MAX_LEVELS
    # and their smallest levels exist at the shipped image sizes (a zero-sized level is refused)
    for H, W in ((680, 1200), (480, 640), (480, 752)):
        assert all(h > 0 and w > 0 for h, w in frequency_loss.level_sizes(H, W, [1.0 / 2 ** i for i in range(max(counts))]))


def test_scratch_size_queries_are_monotone_and_aligned():
    from segs_slam_amd import _capi
    lib = _capi.lib()
    prev = 0
    for P in (0, 1, 255, 256, 257, 50_000, 3_000_000):
        b = lib.segs_geometry_bytes(P)
        assert b >= prev and b % 256 == 0
        prev = b
    assert lib.segs_image_bytes(1920, 1080) > 2 * 4 * 1920 * 1080
    assert lib.segs_binning_bytes(10_000_000) > 10_000_000 * 24


def test_no_cpu_fallback():
    from segs_slam_amd import rasterize_points as rp
    e = torch.empty(0)
    with pytest.raises(RuntimeError, match="GPU"):
        rp.RasterizeGaussiansCUDA(torch.zeros(3), torch.zeros(4, 3), torch.zeros(4, 3), torch.zeros(4, 1), torch.zeros(4, 3),
                                  torch.zeros(4, 4), 1.0, e, torch.eye(4), torch.eye(4), 1.0, 1.0, 16, 16, e, 0, torch.zeros(3), False)
    with pytest.raises(RuntimeError):
        rp.RasterizeGaussiansCUDA(e, torch.zeros(4, 2), e, e, e, e, 1.0, e, e, e, 1.0, 1.0, 8, 8, e, 0, e, False)


def test_camera_tensors_match_reference_logger_dump():
    """Known-answer data: keyframes printed by GaussianKeyframe::logger (src/gaussian_keyframe.cpp:293-302) that the
    reference ships in check_colmap.md; extracted to tests/golden/check_colmap_keyframes.json by
    tests/golden/extract_check_colmap.py.  Pins the layout/convention of view / proj / full_proj / campos."""
    import json
    import numpy as np
    from segs_slam_amd import scenes
    data = json.load(open(os.path.join(ROOT, "tests", "golden", "check_colmap_keyframes.json")))
    assert len(data) >= 5
    for kf in data:
        wvt = np.array(kf["world_view_transform"], dtype=np.float32)
        proj = scenes.projection_matrix(0.01, 100.0, kf["FoVx"], kf["FoVy"]).T
        assert np.allclose(proj, np.array(kf["projection_matrix"]), atol=6e-5 * max(1.0, np.abs(proj).max()))
        full = wvt @ proj
        assert np.allclose(full, np.array(kf["full_proj_transform"]), atol=2e-3)
        center = np.linalg.inv(wvt)[3, :3]
        assert np.allclose(center, np.array(kf["camera_center"]), atol=2e-3)


def test_camera_tensors_match_the_second_reference_dump():
    """Known-answer data: 30 of the 179 cameras of the reference's `check_colmap copy.md` (FoV, image size, world_view_transform,
    full_proj_transform, camera_center printed with four decimals by the original pipeline's camera loader; extracted by
    tests/golden/extract_check_colmap_cameras.py).  From FoV and the printed world_view_transform alone, scenes.projection_matrix
    (znear 0.01, zfar 100: include/gaussian_keyframe.h) must give the printed full projection and camera centre -- to the print
    precision propagated through the 4x4 product (inputs +-5e-5, entries up to 4: 1e-3)."""
    import json
    import numpy as np
    from segs_slam_amd import scenes
    data = json.load(open(os.path.join(ROOT, "tests", "golden", "check_colmap_cameras.json")))
    assert len(data) == 30 and len({(k["image_width"], k["image_height"]) for k in data}) >= 1
    for kf in data:
        wvt = np.array(kf["world_view_transform"], dtype=np.float64)
        assert np.allclose(wvt[:3, 3], 0.0) and wvt[3, 3] == 1.0          # the transposed layout: translation in the last ROW
        proj = scenes.projection_matrix(0.01, 100.0, kf["FoVx"], kf["FoVy"]).T.astype(np.float64)
        assert np.allclose(wvt @ proj, np.array(kf["full_proj_transform"]), atol=1e-3), kf["uid"]
        assert np.allclose(np.linalg.inv(wvt)[3, :3], np.array(kf["camera_center"]), atol=1e-3), kf["uid"]
        # and the tangents the rasterizer takes are those of the printed fields of view
        cam = scenes.make_camera(kf["image_width"], kf["image_height"], kf["image_width"] / (2 * np.tan(kf["FoVx"] / 2)),
                                 kf["image_height"] / (2 * np.tan(kf["FoVy"] / 2)), np.eye(3, dtype=np.float32), np.zeros(3, dtype=np.float32))
        assert abs(cam.tanfovx - np.tan(kf["FoVx"] / 2)) < 1e-6 and abs(cam.tanfovy - np.tan(kf["FoVy"] / 2)) < 1e-6


def test_neural_param_layout_matches_state_dict_order():
    """segs_neural_param_layout (host-only) lists the MLP tensors in the order and sizes of the reference's Sequential
    stacks (src/gaussian_model.cpp:61-98), as restated in oracle/neural_ref.py."""
    import ctypes as C
    from oracle import neural_ref
    from segs_slam_amd import _capi
    lib = _capi.lib()
    for kw in (dict(), dict(appearance_dim=0, use_feat_bank=False), dict(appearance_dim=16, use_feat_bank=False, add_color_dist=True),
               dict(add_opacity_dist=True, add_cov_dist=True)):
        rd = neural_ref.NeuralDims(**kw)
        cd = _capi.NeuralDims(rd.feat_dim, rd.n_offsets, rd.appearance_dim, int(rd.use_feat_bank), int(rd.add_opacity_dist),
                              int(rd.add_cov_dist), int(rd.add_color_dist))
        offs, cnts = (C.c_int64 * 18)(), (C.c_int64 * 18)()
        nt, total = C.c_int(0), C.c_int64(0)
        assert lib.segs_neural_param_layout(C.byref(cd), offs, cnts, C.byref(nt), C.byref(total)) == 0
        shapes = rd.tensor_shapes()
        assert nt.value == len(shapes)
        pos = 0
        for i, (_name, shape) in enumerate(shapes):
            n = int(np.prod(shape))
            assert (offs[i], cnts[i]) == (pos, n)
            pos += n
        assert total.value == pos
        assert lib.segs_neural_temp_bytes(C.byref(cd), 1000) > 1000 * 512 * 4
    bad = _capi.NeuralDims(64, 10, 0, 0, 0, 0, 0)
    assert lib.segs_neural_param_layout(C.byref(bad), None, None, None, None) != 0
    assert lib.segs_neural_temp_bytes(C.byref(bad), 10) == 0


def test_keyframe_from_pose_matches_the_camera_helpers():
    """Keyframe.from_pose = setPose + computeTransformTensors (src/gaussian_keyframe.cpp:21-42, 151-184) on the CPU."""
    import torch
    from segs_slam_amd import neural_gaussians as ng, scenes
    ang = 0.3
    q = np.array([np.cos(ang / 2), 0.0, np.sin(ang / 2), 0.0]) * 3.0                # un-normalised on purpose
    R = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]], dtype=np.float32)
    t = np.array([0.2, -0.1, 0.5], dtype=np.float32)
    kf = ng.Keyframe.from_pose(q, t, 640, 480, 525.0, 520.0, "cpu")
    cam = scenes.make_camera(640, 480, 525.0, 520.0, R, t)
    assert torch.allclose(kf.view, torch.from_numpy(cam.world_view_transform), atol=1e-6)
    assert torch.allclose(kf.proj, torch.from_numpy(cam.full_proj_transform), atol=1e-5)
    assert torch.allclose(kf.campos, torch.from_numpy(cam.camera_center), atol=1e-6)
    assert abs(kf.tanfovx - cam.tanfovx) < 1e-7 and abs(kf.tanfovy - cam.tanfovy) < 1e-7
    assert torch.allclose(kf.pose7, torch.tensor([0.2, -0.1, 0.5, np.cos(ang / 2), 0.0, np.sin(ang / 2), 0.0], dtype=torch.float32), atol=1e-6)
