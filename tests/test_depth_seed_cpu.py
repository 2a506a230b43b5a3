"""CPU-side checks of the depth seeding (include/segs_densify.h: segs_depth_seed): the library exports what the
header declares, DepthSeedParams validates, and the inputs of tests/test_depth_seed_gpu.py are inputs on which float32 and
float64 agree well enough for a bit-for-bit comparison with the float32 reference to be meaningful."""
import os
import re

import numpy as np
import pytest

from tests import _depth_seed_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_what_the_library_exports():
    import ctypes as C
    from segs_slam_amd import _capi
    text = open(os.path.join(ROOT, "include", "segs_densify.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(segs_[a-z0-9_]+)\s*\(", text))
    assert {"segs_depth_seed", "segs_depth_seed_temp_bytes"} <= declared
    lib = _capi.lib()
    for name in ("segs_depth_seed", "segs_depth_seed_temp_bytes"):
        assert hasattr(lib, name) and name in _capi.SYMBOLS
    # the struct of the header, field for field
    m = re.search(r"typedef struct \{([^}]*)\} segs_depth_seed_params;", text)
    fields = [n.strip() for part in m.group(1).split(";") if part.strip() for n in part.strip().split(" ", 1)[1].split(",")]
    assert fields == [n for n, _ in _capi.DepthSeedParamsC._fields_]
    assert C.sizeof(_capi.DepthSeedParamsC) == 24
    # host-only size query: grows with the lattice and with the map, refuses bad sizes
    small, fine, big = (lib.segs_depth_seed_temp_bytes(a, 680, 1200, s) for a, s in ((1000, 4), (1000, 2), (300_000, 4)))
    assert 0 < small < fine and small < big and small % 256 == 0
    assert lib.segs_depth_seed_temp_bytes(10, 680, 1200, 0) == 0 and lib.segs_depth_seed_temp_bytes(-1, 680, 1200, 4) == 0
    assert lib.segs_depth_seed_temp_bytes(0, 3, 2, 4) > 0


def test_depth_seed_params_validation():
    from segs_slam_amd.densify import DepthSeedParams
    p = DepthSeedParams()
    assert (p.stride, p.alpha_max, p.use_front, p.voxel_size, p.max_new) == (4, 0.5, False, None, None)
    DepthSeedParams(stride=1, alpha_max=1.0, voxel_size=0.01, max_new=0)
    for bad in (dict(stride=0), dict(stride=-2), dict(alpha_max=0.0), dict(alpha_max=1.5), dict(alpha_max=float("nan")),
                dict(voxel_size=0.0), dict(voxel_size=-0.01), dict(max_new=-1)):
        with pytest.raises(ValueError):
            DepthSeedParams(**bad)


def test_step_refuses_seeding_it_was_not_made_for():
    """Raised before anything touches a device."""
    import torch
    from segs_slam_amd import neural_gaussians as ng

    class _Step:
        depth_seed = None
    with pytest.raises(ValueError, match="depth_seed"):
        ng.ScaffoldTrainerStep.seed_keyframe(_Step(), None, torch.zeros(4, 4))


def test_lattice_is_the_stated_one():
    for (H, W), s in [((17, 33), 1), ((17, 33), 4), ((48, 64), 3), ((1, 1), 1), ((2, 3), 4), ((3, 3), 4), ((2, 2), 8)]:
        u, v = ref.lattice(H, W, s)
        want = [(uu, vv) for vv in range(H) for uu in range(W) if uu >= s // 2 and (uu - s // 2) % s == 0 and vv >= s // 2 and (vv - s // 2) % s == 0]
        assert list(zip(u.tolist(), v.tolist())) == want
    assert len(ref.lattice(2, 3, 4)[0]) == 0 and len(ref.lattice(3, 3, 4)[0]) == 1 and len(ref.lattice(1, 1, 1)[0]) == 1


def test_float32_and_float64_references_agree_on_the_gpu_tests_inputs():
    """Same candidate set; fewer than 2 % of the voxels differ.  A condition on the inputs: an input that misses it is changed,
    the device is never given a tolerance."""
    seen = 0
    for c in ref.synthetic_cases():
        M = ref.cam_to_world(c["view"])
        a = ref.seed(c["anchor"], c["target"], c["depth"], c["alpha"], *ref.TANFOV, M, c["p"], np.float32)
        b = ref.seed(c["anchor"], c["target"], c["depth"], c["alpha"], *ref.TANFOV, M, c["p"], np.float64)
        assert a["counts"][:4] == b["counts"][:4] and np.array_equal(a["cand_pixels"], b["cand_pixels"])
        va, vb = set(map(tuple, a["voxels"].tolist())), set(map(tuple, b["voxels"].tolist()))
        assert len(va ^ vb) < 0.02 * max(len(va), 1) or len(va ^ vb) == 0, (c["H"], c["W"], c["p"], len(va ^ vb), len(va))
        na, nb = set(map(tuple, a["new_voxels"].tolist())), set(map(tuple, b["new_voxels"].tolist()))
        assert len(na ^ nb) < 0.02 * max(len(na), 1) or len(na ^ nb) == 0
        seen += 1
        if c["H"] * c["W"] > 9:
            # the inputs do exercise what they are meant to: invalid pixels, both sides of alpha_max, blocking anchors
            u, v = ref.lattice(c["H"], c["W"], c["p"].stride)
            assert a["counts"][0] < len(u) and 0 < a["counts"][1] < a["counts"][0]
            if c["p"].use_front:
                assert a["counts"][2] > 0
            if c["A"] >= 257:
                assert a["counts"][5] < a["counts"][4]
    assert seen == (len(ref.SIZES) * len(ref.STRIDES) + len(ref.SMALL)) * len(ref.ANCHOR_COUNTS) * 2
