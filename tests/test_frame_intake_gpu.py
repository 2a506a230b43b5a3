"""The frame-intake kernels (csrc/frame_intake.hip behind segs-slam_amd/frame_intake.py) against the two references of
tests/_frame_intake_ref.py (held against each other by tests/test_frame_intake_cpu.py):

 * the map, image, grey, mask, both depth modes and every pyramid level: the BYTES of the float32 restatement (a);
 * image and mask within tol_px x (spread of the taps) + 1e-6 of the float64 chain (b), every pixel; the hole-aware depth likewise
   outside the pixels within tol_px of a grid line, which stay under 2 % of the image.
   tol_px = 6.76 * 2^-24 * max(in_w, in_h): twice the float32 map error measured on the CPU (2.6e-4 px at 640x480).

Shapes: 37x29 -> 41x23, one row, one column, one full wave row of four workgroup columns (256x4), 67x5, and TUM freiburg2 at its
real 640x480.  67x5 with 3 sub-levels has an empty coarsest level (5 / 8 truncates to 0): FrameIntake refuses it, and the test runs
its two non-empty levels through the C entry."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import _frame_intake_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CAMERAS = [c.name for c in ref.all_cameras()]
SUM_ROUNDING = 1e-6


def dev(a: np.ndarray) -> torch.Tensor:
    if a.dtype == np.uint16:                                         # the bits travel as int16
        return torch.from_numpy(a.view(np.int16).copy()).to(DEV)
    return torch.from_numpy(np.ascontiguousarray(a).copy()).to(DEV)


def make_intake(c: ref.Cam, n: int = 0):
    from segs_slam_amd.frame_intake import CameraModel, FrameIntake
    return FrameIntake(CameraModel(depth_map_factor=5000.0, **c.model_kwargs()), DEV, num_sub_levels=n)


def same_bits(got: torch.Tensor, want: np.ndarray, what: str):
    g = got.detach().cpu().numpy()
    assert g.shape == want.shape and g.dtype == want.dtype, (what, g.shape, want.shape, g.dtype, want.dtype)
    if g.dtype == np.float32:
        differ = (g.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(g) & np.isnan(want))
    else:
        differ = g != want
    bad = np.argwhere(differ)
    assert len(bad) == 0, f"{what}: {len(bad)} of {g.size} differ, first at {bad[0].tolist()}: {g[tuple(bad[0])]!r} != {want[tuple(bad[0])]!r}"


@functools.lru_cache(maxsize=None)
def want_of(name: str):
    """Everything reference (a) says about a camera, computed once."""
    c = ref.camera(name)
    rgb, mono, raw = ref.frame_u8(c.in_w, c.in_h, 3), ref.frame_u8(c.in_w, c.in_h, 1), ref.depth_u16(c.in_w, c.in_h)
    image, gray = ref.image_f32(c, rgb)
    mono_image, mono_gray = ref.image_f32(c, mono)
    rawf = (raw.astype(np.float32) * np.float32(0.731) - np.float32(900.0)).astype(np.float32)      # negatives are holes too
    w = dict(map=np.stack(ref.map_f32(c), axis=-1), image=image, gray=gray, mono_image=mono_image, mono_gray=mono_gray,
             mask=ref.mask_f32(c), rawf=rawf)
    for hole in (False, True):
        w[f"depth{int(hole)}"] = ref.depth_f32(c, raw, ref.INV_FACTOR, hole)
        w[f"depthf{int(hole)}"] = ref.depth_f32(c, rawf, ref.INV_FACTOR, hole)
    for v in w.values():
        v.setflags(write=False)
    return w


@pytest.mark.parametrize("name", CAMERAS)
def test_every_output_has_the_restatements_bytes(name):
    c, want = ref.camera(name), want_of(name)
    it = make_intake(c)
    same_bits(it.debug_map(), want["map"], "map")
    same_bits(it.mask, want["mask"], "mask")
    f = it.rgb(dev(ref.frame_u8(c.in_w, c.in_h, 3)), want_gray=True)
    assert f.image is it.image and f.levels == [] and f.gray is it.gray_u8
    same_bits(f.image, want["image"], "image")
    same_bits(f.gray, want["gray"], "gray")
    assert it.rgb(dev(ref.frame_u8(c.in_w, c.in_h, 3))).gray is None
    same_bits(it.gray(dev(ref.frame_u8(c.in_w, c.in_h, 1)[..., 0])), want["mono_gray"], "gray of a single channel")
    same_bits(it.gray_image, want["mono_image"], "single-channel image")
    raw = dev(ref.depth_u16(c.in_w, c.in_h))
    rawf = dev(want["rawf"])
    for hole in (False, True):
        same_bits(it.depth(raw, hole_aware=hole), want[f"depth{int(hole)}"], f"depth of uint16, hole_aware={hole}")
        same_bits(it.depth(rawf, hole_aware=hole), want[f"depthf{int(hole)}"], f"depth of float32, hole_aware={hole}")
    if hasattr(torch, "uint16"):
        same_bits(it.depth(raw.view(torch.uint16)), want["depth1"], "depth of a uint16 tensor")


@pytest.mark.parametrize("name", CAMERAS)
def test_outputs_lie_within_the_map_tolerance_of_the_float64_chain(name):
    c = ref.camera(name)
    tol = ref.tol_px(c.in_w, c.in_h)
    it = make_intake(c)
    src = ref.frame_u8(c.in_w, c.in_h, 3)
    image = it.rgb(dev(src)).image.cpu().numpy().astype(np.float64)
    b = ref.image_f64(c, src)
    for ch in range(3):
        err = np.abs(image[ch] - b[ch])
        bound = tol * ref.tap_spread(c, src[..., ch]) / 255.0 + SUM_ROUNDING
        print(f"{name} channel {ch}: max error {err.max():.3e}, largest bound {bound.max():.3e}")
        assert (err <= bound).all(), (name, ch, float(err.max()))
    err = np.abs(it.mask.cpu().numpy().astype(np.float64) - ref.mask_f64(c))
    assert (err <= tol * ref.tap_spread(c, np.ones((c.in_h, c.in_w))) + SUM_ROUNDING).all(), (name, float(err.max()))
    raw = ref.depth_u16(c.in_w, c.in_h)
    metres = raw.astype(np.float64) * ref.INV_FACTOR
    bound = tol * ref.tap_spread(c, metres) + SUM_ROUNDING * max(1.0, float(metres.max()))
    (ax, ay), (bx, by) = ref.map_f32(c), ref.map_f64(c)
    with np.errstate(invalid="ignore"):
        differ = ~((ax.astype(np.float64) == bx) & (ay.astype(np.float64) == by))
    out = ref.near_grid_line(c, tol) & differ
    assert out.mean() < 0.02, (name, float(out.mean()))
    z = it.depth(dev(raw), hole_aware=True).cpu().numpy().astype(np.float64)
    err = np.abs(z - ref.depth_f64(c, raw, ref.INV_FACTOR, True))
    print(f"{name} hole-aware depth: {int(out.sum())} of {out.size} pixels left out, max error elsewhere {err[~out].max():.3e}")
    assert (err <= bound)[~out].all(), (name, float(err[~out].max()))


def test_the_map_leaves_the_source_through_all_four_borders():
    for name in ("tum-37x29-41x23", "tum-640x480"):
        c = ref.camera(name)
        m = make_intake(c).debug_map()
        mx, my = m[..., 0], m[..., 1]
        assert (mx < -1).any() and (mx > c.in_w).any() and (my < -1).any() and (my > c.in_h).any(), name
        assert ref.camera("tum-37x29-41x23").all_borders


# ---------------------------------------------------------------------------------------------------------------- levels
@pytest.mark.parametrize("name,n", [("tum-37x29-41x23", 2), ("tum-37x29-41x23", 3), ("tum-67x5-67x5", 2), ("rot-37x29-41x23", 3)])
def test_pyramid_levels_have_the_restatements_bytes(name, n):
    from segs_slam_amd.frame_intake import pyramid_sizes
    c, want = ref.camera(name), want_of(name)
    it = make_intake(c, n)
    sizes = pyramid_sizes(c.out_w, c.out_h, n)
    assert it.sizes == sizes and all(w * 2 ** (n - l) <= c.out_w for l, (w, _) in enumerate(sizes))       # noqa: E741
    f = it.rgb(dev(ref.frame_u8(c.in_w, c.in_h, 3)))
    same_bits(f.image, want["image"], "image")
    assert len(f.levels) == len(it.mask_levels) == n
    for l, (w, h) in enumerate(sizes):                                                                     # noqa: E741
        assert f.levels[l].shape == (3, h, w) and it.mask_levels[l].shape == (h, w)
        same_bits(f.levels[l], ref.resize_f32(want["image"], w, h), f"level {l} ({w}x{h})")
        same_bits(it.mask_levels[l], ref.resize_f32(want["mask"][None], w, h)[0], f"mask level {l} ({w}x{h})")


def test_three_sub_levels_of_67x5_through_the_c_entry():
    """5 * 0.125 truncates to 0: the reference's formula gives an empty coarsest level, which FrameIntake refuses; the two levels
    that exist (16x1 and 33x2) are written by one launch of the C entry."""
    from segs_slam_amd import _capi
    from segs_slam_amd.frame_intake import pyramid_sizes
    c, want = ref.camera("tum-67x5-67x5"), want_of("tum-67x5-67x5")
    sizes = pyramid_sizes(67, 5, 3)
    assert sizes == [(8, 0), (16, 1), (33, 2)]
    with pytest.raises(ValueError, match="empty level"):
        make_intake(c, 3)
    live = sizes[1:]
    src = dev(want["image"])
    outs = [torch.full((3, h, w), float("nan"), device=DEV) for w, h in live]
    rc = _capi.lib().segs_resize_levels(3, 67, 5, C.c_void_p(src.data_ptr()), 2, (C.c_int * 2)(*[w for w, _ in live]),
                                        (C.c_int * 2)(*[h for _, h in live]), (C.c_void_p * 2)(*[t.data_ptr() for t in outs]),
                                        C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
    assert rc == 0
    for t, (w, h) in zip(outs, live):
        same_bits(t, ref.resize_f32(want["image"], w, h), f"level {w}x{h}")


# ---------------------------------------------------------------------------------------------------------------- identity
@pytest.mark.parametrize("name", [n for n in CAMERAS if n.startswith("identity")])
def test_identity_camera_is_a_conversion(name):
    from segs_slam_amd import stereo
    c = ref.camera(name)
    it = make_intake(c)
    frame = ref.frame_u8(c.in_w, c.in_h, 3)
    f = it.rgb(dev(frame), want_gray=True)
    # frame.float() / 255 as an IEEE division (torch's CUDA division by a scalar multiplies by the reciprocal instead)
    same_bits(f.image, frame.transpose(2, 0, 1).astype(np.float32) / np.float32(255), "image")
    assert (it.mask == 1).all()
    assert torch.equal(f.gray, stereo.rgb_to_gray_u8(f.image))
    raw = ref.depth_u16(c.in_w, c.in_h)
    z = it.depth(dev(raw), hole_aware=True)
    same_bits(z, raw.astype(np.float32) * np.float32(ref.INV_FACTOR), "depth")
    assert torch.equal(z, it.depth(dev(raw), hole_aware=False).clone())


def test_identity_greys_give_the_stereo_matcher_the_same_bytes():
    from segs_slam_amd import stereo
    W, H = 97, 33
    c = ref.identity(W, H)
    left = ref.frame_u8(W + 9, H, 3, seed=5)
    pair = [np.ascontiguousarray(left[:, :W]), np.ascontiguousarray(left[:, 9:])]           # left pixel x is the right view's x - 9
    intakes = [make_intake(c), make_intake(c)]
    greys = [it.rgb(dev(a), want_gray=True).gray for it, a in zip(intakes, pair)]
    direct = [stereo.rgb_to_gray_u8(dev(a.transpose(2, 0, 1).astype(np.float32) / np.float32(255))) for a in pair]
    assert all(torch.equal(g, d) for g, d in zip(greys, direct))
    sgm = stereo.StereoSGM(H, W, DEV, num_disparities=64)
    a = sgm.compute(*greys).clone()
    b = sgm.compute(*direct)
    assert torch.equal(a, b)
    assert ((a[5:-5, 40:90] - 16 * 9).abs() <= 16).float().mean() > 0.8           # and the pair does match: 9 pixels of disparity
    depth = sgm.compute_depth(greys[0], greys[1], 64.0, 0.1)                        # the grey outputs go straight in
    assert depth.shape == (H, W) and (depth > 0).any()


# ---------------------------------------------------------------------------------------------------------------- hand-off
def test_hand_off_to_the_step_and_the_depth_loss():
    from segs_slam_amd import neural_gaussians as ng, scenes
    from segs_slam_amd.depth_loss import DepthLossParams, FusedDepthLoss
    from segs_slam_amd.frame_intake import CameraModel, FrameIntake
    W, H = 64, 48
    it = FrameIntake(CameraModel(width=W, height=H, fx=60.0, fy=60.0, cx=31.5, cy=23.5, k1=0.05, k2=-0.01, depth_map_factor=5000.0), DEV,
                     num_sub_levels=1)
    f = it.rgb(dev(ref.frame_u8(W, H, 3)))
    assert [tuple(t.shape) for t in f.levels] == [(3, 24, 32)] and tuple(f.image.shape) == (3, H, W)
    cam = scenes.make_camera(W, H, 60.0, 60.0, np.eye(3, dtype=np.float32), np.zeros(3, dtype=np.float32))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    kf = ng.Keyframe(t(cam.world_view_transform), t(cam.full_proj_transform), t(cam.camera_center),
                     torch.tensor([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0], device=DEV), cam.tanfovx, cam.tanfovy)
    step = ng.ScaffoldTrainerStep(ng.synthetic_model(500, ng.ModelDims(), cam, torch.device(DEV), seed=9), W, H)
    low = float(step.training_once([kf], [f.levels[0]]))
    assert (step.W, step.H) == (32, 24)
    full = float(step.training_once([kf], [f.image]))
    assert (step.W, step.H) == (W, H)
    torch.cuda.synchronize()
    assert np.isfinite(low) and np.isfinite(full) and low > 0 and full > 0
    assert len(step._levels) == 2 and step.dropped_steps() == 0
    z = it.depth(dev(ref.depth_u16(W, H)))
    target = FusedDepthLoss(H, W, DEV, DepthLossParams(1.0)).prepare(z)
    assert torch.equal(target.map, z) and target.n_valid() == int((z != 0).sum().item()) > 0.5 * W * H


# ---------------------------------------------------------------------------------------------------------------- buffers
def _poison(it):
    for tns in [it.image, it.gray_u8, it.gray_image, it.depth_map] + it.levels:
        if tns.dtype == torch.uint8:
            tns.fill_(0xCD)
        else:
            tns.fill_(float("nan"))


def test_a_second_frame_overwrites_the_buffers_whatever_they_held():
    name = "tum-37x29-41x23"
    c, want = ref.camera(name), want_of(name)
    it = make_intake(c, 2)
    other = ref.frame_u8(c.in_w, c.in_h, 3, seed=1)
    assert (other != ref.frame_u8(c.in_w, c.in_h, 3)).any()
    first = it.rgb(dev(other), want_gray=True)
    other_image, other_gray = ref.image_f32(c, other)
    same_bits(first.image, other_image, "first frame")
    _poison(it)
    f = it.rgb(dev(ref.frame_u8(c.in_w, c.in_h, 3)), want_gray=True)
    assert f.image.data_ptr() == first.image.data_ptr()
    same_bits(f.image, want["image"], "image")
    same_bits(f.gray, want["gray"], "gray")
    for l, (w, h) in enumerate(it.sizes):                                          # noqa: E741
        same_bits(f.levels[l], ref.resize_f32(want["image"], w, h), f"level {l}")
    _poison(it)
    same_bits(it.depth(dev(ref.depth_u16(c.in_w, c.in_h))), want["depth1"], "depth")
    same_bits(it.gray(dev(ref.frame_u8(c.in_w, c.in_h, 1)[..., 0])), want["mono_gray"], "gray")
    same_bits(it.gray_image, want["mono_image"], "single-channel image")
    same_bits(it.mask, want["mask"], "the mask is left alone")


def test_rgb_replays_from_a_graph_to_the_same_bytes():
    name = "tum-67x5-67x5"
    c, want = ref.camera(name), want_of(name)
    it = make_intake(c, 2)
    frame = dev(ref.frame_u8(c.in_w, c.in_h, 3, seed=1))
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        it.rgb(frame, want_gray=True)                                              # warm-up outside the capture
    torch.cuda.current_stream(DEV).wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        it.rgb(frame, want_gray=True)                                              # two launches on one stream: a single chain
    frame.copy_(dev(ref.frame_u8(c.in_w, c.in_h, 3)))
    _poison(it)
    g.replay()
    torch.cuda.synchronize()
    same_bits(it.image, want["image"], "image")
    same_bits(it.gray_u8, want["gray"], "gray")
    for l, (w, h) in enumerate(it.sizes):                                          # noqa: E741
        same_bits(it.levels[l], ref.resize_f32(want["image"], w, h), f"level {l}")
    eager = make_intake(c, 2).rgb(frame, want_gray=True)
    assert torch.equal(eager.image.view(torch.int32), it.image.view(torch.int32)) and torch.equal(eager.gray, it.gray_u8)


def test_wrong_inputs_are_refused():
    from segs_slam_amd import _capi
    c = ref.camera("rot-37x29-41x23")
    it = make_intake(c)
    with pytest.raises(RuntimeError, match="GPU"):
        it.rgb(torch.zeros((c.in_h, c.in_w, 3), dtype=torch.uint8))
    with pytest.raises(ValueError):
        it.rgb(torch.zeros((c.out_h, c.out_w, 3), dtype=torch.uint8, device=DEV))  # the OUTPUT size is not the source's
    with pytest.raises(ValueError):
        it.rgb(torch.zeros((c.in_h, c.in_w, 3), dtype=torch.float32, device=DEV))
    with pytest.raises(ValueError):
        it.gray(torch.zeros((c.in_h, c.in_w, 1), dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError):
        it.depth(torch.zeros((c.in_h, c.in_w), dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError):
        make_intake(c, 9)
    with pytest.raises(_capi.SegsError, match="frame intake"):
        it._cam.nfx = 0.0
        it.debug_map()
