"""The stereo matcher's kernels (csrc/stereo_sgm.hip behind segs-slam_amd/stereo.py) against the NumPy restatement of the
specification (tests/_sgm_ref.py, itself held to ground truth by tests/test_stereo_sgm_cpu.py): every stage that `stages()` copies
out and both outputs, bit for bit -- the arithmetic is integer, so there is no tolerance anywhere; depth is compared as float32 bits."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

from tests import _sgm_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
FX, BASELINE = 435.2, 0.11
DEFAULTS = dict(D=64, dmin=0, P1=10, P2=120, u=5, paths=4, lr_max_diff=1, median=True)


@functools.lru_cache(maxsize=None)
def make_pair(kind: str, W: int, H: int, seed: int = 7):
    rng = np.random.default_rng(seed + 1000 * W + H)
    if kind == "shifted" and W > 40:
        left, right, _ = ref.shifted_pair(H, W, 7, 19, seed=seed)
    elif kind in ("shifted", "noise"):
        left, right = (rng.integers(0, 256, (H, W), dtype=np.uint8) for _ in range(2))
    elif kind == "constant":
        left = right = np.full((H, W), 93, dtype=np.uint8)
    elif kind == "ramp":                                   # 3 grey levels per column, wrapping: every row alike, ties along y
        left = np.tile(((3 * np.arange(W)) % 256).astype(np.uint8), (H, 1))
        right = np.tile(((3 * (np.arange(W) + 5)) % 256).astype(np.uint8), (H, 1))
    else:
        raise KeyError(kind)
    left.setflags(write=False)
    right.setflags(write=False)
    return left, right


@functools.lru_cache(maxsize=None)
def reference(kind, W, H, items):
    left, right = make_pair(kind, W, H)
    st = ref.sgm(left, right, fb16=ref.fb16_of(FX, BASELINE), **dict(items))
    for v in st.values():
        v.setflags(write=False)
    return st


def matcher(W, H, p):
    from segs_slam_amd import stereo
    return stereo.StereoSGM(H, W, DEV, num_disparities=p["D"], min_disparity=p["dmin"], P1=p["P1"], P2=p["P2"], uniqueness_ratio=p["u"],
                            paths=p["paths"], lr_max_diff=p["lr_max_diff"], median=p["median"])


def bits(t: torch.Tensor, dtype):
    return t.cpu().numpy().view(dtype)


STAGES = (("census_left", np.uint32), ("census_right", np.uint32), ("S", np.uint16), ("raw_winner", np.uint16),
          ("disp_right", np.int16), ("raw_median", np.uint16), ("disp16", np.int16), ("depth", np.uint32))


def check_case(kind, W, H, **over):
    p = dict(DEFAULTS, **over)
    want = reference(kind, W, H, tuple(sorted(p.items())))
    left, right = (torch.from_numpy(a.copy()).to(DEV) for a in make_pair(kind, W, H))
    sgm = matcher(W, H, p)
    got = sgm.stages(left, right, FX, BASELINE)
    torch.cuda.synchronize()
    for name, dt in STAGES:                                  # in pipeline order: the first mismatch names the stage at fault
        g, w = bits(got[name], dt), want[name].view(dt)
        assert g.shape == w.shape, name
        bad = np.argwhere(g != w)
        assert len(bad) == 0, f"{name}: {len(bad)} of {g.size} differ, first at {bad[0].tolist()}: {g[tuple(bad[0])]} != {w[tuple(bad[0])]}"
    # the two public calls give the same bytes as the debug run
    assert np.array_equal(bits(sgm.compute(left, right), np.int16), want["disp16"])
    assert np.array_equal(bits(sgm.compute_depth(left, right, FX, BASELINE), np.uint32), want["depth"].view(np.uint32))
    return sgm, left, right, want


# W x H, D: smaller than the census window; one census pixel; W < D; odd sizes across a wave and the four-line strips; the two
# wider disparity ranges; all-border medians
SHAPES = [(8, 6, 64), (9, 7, 64), (40, 16, 64), (97, 33, 64), (130, 20, 128), (70, 11, 256), (1, 1, 64), (3, 3, 64), (2, 5, 128)]


@pytest.mark.parametrize("paths", [4, 8])
@pytest.mark.parametrize("W,H,D", SHAPES)
def test_every_stage_matches_the_restatement(W, H, D, paths):
    check_case("shifted", W, H, D=D, paths=paths)


@pytest.mark.parametrize("kind", ["noise", "constant", "ramp"])
@pytest.mark.parametrize("W,H,D,paths", [(97, 33, 64, 8), (130, 20, 128, 4), (70, 11, 256, 8)])
def test_other_inputs(kind, W, H, D, paths):
    check_case(kind, W, H, D=D, paths=paths)


@pytest.mark.parametrize("paths", [4, 8])
@pytest.mark.parametrize("dmin", [0, 5, 96])
def test_min_disparity_at_width_130(dmin, paths):
    """96 is EuRoC.yaml's value: at this width nearly no left pixel has a right pixel."""
    check_case("shifted", 130, 20, D=128, dmin=dmin, paths=paths)


VARIANTS = [dict(P1=0, P2=0), dict(P1=224, P2=224), dict(u=0), dict(u=50), dict(lr_max_diff=-1), dict(lr_max_diff=0), dict(median=False),
            dict(u=0, lr_max_diff=-1, median=False), dict(dmin=5, P1=224, P2=224, u=50, lr_max_diff=0)]


@pytest.mark.parametrize("paths", [4, 8])
@pytest.mark.parametrize("variant", VARIANTS, ids=lambda v: "-".join(f"{k}{x}" for k, x in v.items()))
def test_parameter_variants(variant, paths):
    _, _, _, want = check_case("shifted", 97, 33, paths=paths, **variant)
    if variant.get("P2", 1) == 0:                            # no smoothing: every path's cost is the matching cost
        C = ref.cost_volume(want["census_left"], want["census_right"], 64, 0)
        assert np.array_equal(want["S"].astype(np.int64), paths * C)


def test_variants_on_the_wider_ranges():
    check_case("shifted", 130, 20, D=128, paths=8, P1=0, P2=0, u=50, lr_max_diff=0, median=False)
    check_case("noise", 70, 11, D=256, paths=4, P1=224, P2=224, u=0, lr_max_diff=-1, dmin=5)


def test_two_calls_give_identical_bytes_and_a_side_stream_works():
    sgm, left, right, want = check_case("shifted", 160, 40)
    a = sgm.compute_depth(left, right, FX, BASELINE).clone()
    d16 = sgm.disp16.clone()
    sgm.depth.fill_(-1.0)
    sgm.disp16.fill_(-7)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        b = sgm.compute_depth(left, right, FX, BASELINE)
    side.synchronize()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(d16, sgm.disp16)
    assert np.array_equal(bits(b, np.uint32), want["depth"].view(np.uint32))


def test_grey_conversion():
    from segs_slam_amd import stereo
    rng = np.random.default_rng(3)
    k = np.arange(0, 256, dtype=np.float32)
    halves = (k + np.float32(0.5)) / np.float32(255.0)        # g * 255 lands on or next to k + 0.5
    special = np.array([-1.0, -1e-3, 0.0, 1.0, 1.0 + 1e-3, 2.0, np.nan, np.inf, -np.inf, 0.5], dtype=np.float32)
    grey = np.concatenate([halves, k / np.float32(255.0), special])
    n = grey.size
    rgb = np.empty((3, 3, n), dtype=np.float32)
    rgb[:, 0] = grey                                          # R = G = B
    rgb[:, 1] = rng.random((3, n), dtype=np.float32)
    rgb[:, 2] = rng.random((3, n), dtype=np.float32) * 2 - 0.5
    rgb[0, 2, :4] = np.nan
    got = stereo.rgb_to_gray_u8(torch.from_numpy(rgb).to(DEV))
    assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), ref.rgb_to_gray_u8(rgb))
    assert got[0, 256 + 256 + 6].item() == 0                  # NaN


def test_rgb_inputs_go_through_the_grey_kernel():
    from segs_slam_amd import stereo
    W, H = 97, 33
    rng = np.random.default_rng(11)
    lrgb = rng.random((3, H, W), dtype=np.float32)
    rrgb = np.roll(lrgb, -6, axis=2)
    want = ref.sgm(ref.rgb_to_gray_u8(lrgb), ref.rgb_to_gray_u8(rrgb), fb16=ref.fb16_of(FX, BASELINE), **DEFAULTS)
    sgm = matcher(W, H, DEFAULTS)
    depth = sgm.compute_depth(torch.from_numpy(lrgb).to(DEV), torch.from_numpy(rrgb).to(DEV), FX, BASELINE)
    assert np.array_equal(bits(depth, np.uint32), want["depth"].view(np.uint32))
    assert np.array_equal(bits(sgm.disp16, np.int16), want["disp16"])
    assert (want["depth"] > 0).mean() > 0.5                   # the case is not vacuous
    with pytest.raises(RuntimeError, match="GPU"):
        sgm.compute_depth(torch.zeros((H, W), dtype=torch.uint8), torch.zeros((H, W), dtype=torch.uint8), FX, BASELINE)
    with pytest.raises(RuntimeError, match="GPU"):
        stereo.StereoSGM(H, W, "cpu")
    with pytest.raises(ValueError):
        sgm.compute(torch.zeros((H, W + 1), dtype=torch.uint8, device=DEV), torch.zeros((H, W), dtype=torch.uint8, device=DEV))


BAD = [dict(D=32), dict(D=100), dict(D=512), dict(dmin=-1), dict(D=256, dmin=1792), dict(P1=-1), dict(P1=11, P2=10), dict(P2=225),
       dict(paths=5), dict(paths=2), dict(u=-1), dict(u=100), dict(lr_max_diff=-2), dict(median=2), dict(W=0), dict(H=0), dict(W=4097),
       dict(H=4097)]


def test_invalid_parameters_return_the_error_and_write_nothing():
    from segs_slam_amd import _capi
    lib = _capi.lib()
    W, H = 40, 16
    left = torch.zeros((H, W), dtype=torch.uint8, device=DEV)
    disp = torch.full((H, W), -7, dtype=torch.int16, device=DEV)
    depth = torch.full((H, W), -1.0, dtype=torch.float32, device=DEV)
    temp = torch.full((lib.segs_stereo_sgm_temp_bytes(W, H, 64, 4),), 0x5A, dtype=torch.uint8, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())       # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    for bad in BAD:
        q = {**DEFAULTS, "W": W, "H": H, **bad}
        cp = _capi.StereoParamsC(q["D"], q["dmin"], q["P1"], q["P2"], q["u"], q["paths"], q["lr_max_diff"], int(q["median"]))
        rc = lib.segs_stereo_sgm(C.byref(cp), q["W"], q["H"], p(left), p(left), p(disp), p(depth), 1.0, p(temp), stream)
        assert rc == -1, bad                                    # SEGS_ERR_INVALID_ARGUMENT
        rc = lib.segs_debug_stereo_sgm_stages(C.byref(cp), q["W"], q["H"], p(left), p(left), p(disp), p(depth), 1.0, p(temp),
                                              None, None, None, None, None, None, stream)
        assert rc == -1, bad
    for args in ((0, 16, 64, 4), (40, 4097, 64, 4), (40, 16, 96, 4), (40, 16, 64, 6)):
        assert lib.segs_stereo_sgm_temp_bytes(*args) == 0
    assert lib.segs_stereo_sgm(None, W, H, p(left), p(left), p(disp), p(depth), 1.0, p(temp), stream) == -1
    assert lib.segs_rgb_to_gray_u8(0, 4, p(depth), p(left), stream) == -1
    torch.cuda.synchronize()
    assert (disp == -7).all() and (depth == -1.0).all() and (temp == 0x5A).all()
    # the edge of the valid range is accepted: D + dmin = 2047
    from segs_slam_amd import stereo
    sgm = stereo.StereoSGM(H, W, DEV, num_disparities=256, min_disparity=1791, P1=0, P2=224, uniqueness_ratio=99, paths=8, lr_max_diff=0)
    out = sgm.compute(left, left)
    assert (out == 16 * 1790).all()                             # nothing has a right pixel
    with pytest.raises(ValueError):
        stereo.StereoSGM(H, W, DEV, num_disparities=96)
    with pytest.raises(_capi.SegsError):
        stereo.StereoSGM(H, W, DEV, P1=200, P2=100).compute(left, left)


def test_from_config_reads_the_shipped_stereo_values():
    from segs_slam_amd import mapper_config as mc, stereo
    with open(os.path.join(ROOT, "tests", "golden", "mapper_cfg_values.json")) as f:
        shipped = json.load(f)
    names = sorted(k for k in shipped if "/Stereo/" in k)
    assert len(names) == 4 and any("EuRoC" in k for k in names) and any("KITTI" in k for k in names)
    seen = set()
    for name in names:
        cfg = mc.mapper_config_from_values(shipped[name], name)
        sgm = stereo.StereoSGM.from_config(cfg, 20, 130, DEV)
        assert sgm.params.num_disparities == shipped[name]["Stereo.num_disparity"] == 128
        assert sgm.params.min_disparity == shipped[name]["Stereo.min_disparity"]
        assert (sgm.params.P1, sgm.params.P2, sgm.params.uniqueness_ratio, sgm.params.paths) == (10, 120, 5, 4)
        seen.add(sgm.params.min_disparity)
        over = stereo.StereoSGM.from_config(cfg, 20, 130, DEV, paths=8, min_disparity=3)
        assert (over.params.paths, over.params.min_disparity) == (8, 3)
    assert seen == {8, 96}
    # and the object a configuration makes computes what the restatement computes with those values
    cfg = mc.mapper_config_from_values(shipped[names[0]], names[0])
    sgm = stereo.StereoSGM.from_config(cfg, 20, 130, DEV)
    want = reference("shifted", 130, 20, tuple(sorted(dict(DEFAULTS, D=128, dmin=sgm.params.min_disparity).items())))
    left, right = (torch.from_numpy(a.copy()).to(DEV) for a in make_pair("shifted", 130, 20))
    assert np.array_equal(bits(sgm.compute(left, right), np.int16), want["disp16"])


def test_depth_goes_straight_into_the_depth_loss():
    from segs_slam_amd.depth_loss import DepthLossParams, FusedDepthLoss
    sgm, left, right, want = check_case("shifted", 160, 40)
    depth = sgm.compute_depth(left, right, FX, BASELINE)
    loss = FusedDepthLoss(40, 160, DEV, DepthLossParams(1.0))
    target = loss.prepare(depth)
    nonzero = int((depth != 0).sum().item())
    assert target.n_valid() == nonzero == int((want["depth"] != 0).sum()) and nonzero > 0.8 * depth.numel()
    assert torch.equal(target.map, depth)
    # 7 pixels of disparity in the top half: fx baseline / d, to the half pixel that the sub-pixel offset can move it by
    inner = depth[5:15, 40:150]
    assert ((inner - FX * BASELINE / 7.0).abs() <= FX * BASELINE * (1 / 6.5 - 1 / 7.0)).all()
