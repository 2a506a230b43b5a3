"""Keyframe evaluation on the device (include/segs_eval.h, csrc/eval_metrics.hip, segs_slam_amd/evaluation.py)
against the float64 chain of tests/_eval_metrics_ref.py, whose bars tests/test_eval_metrics_cpu.py checks on the float32 torch chain
first (largest |float32 chain - float64 chain| / bar there: 0.216; largest |kernel - float64 chain| / bar measured over the cases of
this file on the MI355X: 0.613).  Every case prints its ratio before it asserts."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from segs_slam_amd import evaluation as ev  # noqa: E402
from tests import _eval_metrics_ref as ref  # noqa: E402

DEV = "cuda:0"
IMAGE_SHAPES = ref.SMALL_SHAPES + [(5, 8), (3, 2052), (2, 1031)]      # + dword stores (W % 4 == 0), a second round of either form
SENTINEL = -12345.5


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _nan_pair(H, W):
    """A noise pair with NaNs in image and target, one of them alone in an otherwise zero target row (NaN != 0: the row stays on)."""
    img, gt = (t.clone() for t in ref.make_pair("noise", H, W, seed=3))
    img.view(-1)[::7] = float("nan")
    gt.view(-1)[3::11] = float("nan")
    gt[1, H // 2] = 0.0
    gt[1, H // 2, W // 2] = float("nan")
    gt[2, H - 1] = 0.0
    img[0, 0, 0] = float("inf")
    return img.contiguous(), gt.contiguous()


def _report_row(what, r, row):
    print(f"{what}: |row - float64| / bar = {r.ratio(row):.3f}  row {np.asarray(row).tolist()}")


@pytest.mark.parametrize("H,W", ref.SMALL_SHAPES)
def test_metrics_of_every_class_with_and_without_the_row_mask(H, W):
    """One pixel, less than a halo, both seams of the 32 x 16 tile: the sixteen (class, row_mask) pairs go to sixteen slots of one
    table and come back in ONE readback.  ssim within 4 e + 2e-6; mse, mse_c, l1 within 4 e_rel + 32 * 2^-24 relative (segs_eval.h:
    the longest chain of additions is 28); the PSNRs within 4.35 * that + 4 * 2^-24 * |value| dB; `equal` and `black` (and `impulse`
    under the mask, whose target is all zero) give exactly +inf and ssim == 1 within its bar."""
    from segs_slam_amd import _capi
    assert _capi.lib().segs_l1_ssim_tile_rows(H, W) == 16
    cases = [(c, m) for c in ref.CLASSES for m in (True, False)]
    fm = ev.FusedImageMetrics(H, W, DEV, len(cases))
    for slot, (cls, m) in enumerate(cases):
        img, gt, _ = ref.case(cls, H, W, m)
        fm.measure(img.to(DEV), gt.to(DEV), slot, row_mask=m)
    table = fm.results()
    assert table.shape == (len(cases), 8) and table.dtype == np.float64
    for slot, (cls, m) in enumerate(cases):
        _, _, r = ref.case(cls, H, W, m)
        _report_row(f"{cls} mask={m}", r, table[slot])
        assert r.misses(table[slot]) == [], (cls, m)
        if cls in ("equal", "black") or (cls == "impulse" and m):
            assert table[slot, 1] == table[slot, 2] == float("inf") and table[slot, 3] == 0.0 and table[slot, 7] == 0.0
            assert abs(table[slot, 0] - 1.0) <= r.bars()[0]


def test_metrics_at_the_smallest_size_with_32_row_tiles():
    from segs_slam_amd import _capi
    H, W = ref.TY32_SHAPE
    lib = _capi.lib()
    assert lib.segs_l1_ssim_tile_rows(H, W) == 32 and lib.segs_l1_ssim_tile_rows(H - 1, W) == 16
    img, gt, r = ref.case("masked", H, W, True)
    fm = ev.FusedImageMetrics(H, W, DEV, 2)
    x, t = img.to(DEV), gt.to(DEV)
    fm.measure(x, t, 1, row_mask=True)
    ims = fm.images_u8(x, t, row_mask=True)
    row = fm.results()[1]
    _report_row("masked 481x1024", r, row)
    assert r.misses(row) == []
    want = ref.images(img, gt, True)
    for name in ev.IMAGES:
        assert np.array_equal(ims[name].cpu().numpy(), want[name]), name


@pytest.mark.parametrize("H,W", IMAGE_SHAPES)
def test_recorded_images_are_the_restated_bytes(H, W):
    """Device bytes == the NumPy float32 restatement, every element, for every class, `out_of_range` and an input with NaNs
    included; with the flags computed by the kernel itself and with the flags a measure() of the same target left behind."""
    fm = ev.FusedImageMetrics(H, W, DEV, 1)
    pairs = [(c, ref.make_pair(c, H, W)) for c in ref.CLASSES] + [("nan", _nan_pair(H, W))]
    for cls, (img, gt) in pairs:
        x, t = img.to(DEV), gt.to(DEV)
        for m in (True, False):
            want = ref.images(img, gt, m)
            fm._flags_of = None
            own = fm.images_u8(x, t, row_mask=m)                     # flags computed in the images kernel
            fm.measure(x, t, 0, row_mask=m)
            shared = fm.images_u8(x, t, row_mask=m)                  # flags read from temp
            for name in ev.IMAGES:
                assert own[name].shape == (H, W, 3) and own[name].dtype == torch.uint8
                assert np.array_equal(own[name].cpu().numpy(), want[name]), (cls, m, name)
                assert np.array_equal(shared[name].cpu().numpy(), want[name]), (cls, m, name, "flags from temp")
        only = fm.images_u8(x, t, row_mask=True, which=("loss",))
        assert list(only) == ["loss"] and np.array_equal(only["loss"].cpu().numpy(), ref.images(img, gt, True)["loss"])
    with pytest.raises(ValueError):
        fm.images_u8(x, t, which=("depth",))


def _frame(lib, x, t, H, W, m, table, n_slots, slot, temp):
    from segs_slam_amd import _capi
    _capi.check(lib.segs_eval_frame(_ptr(x), _ptr(t), H, W, int(m), _ptr(table), n_slots, slot, _ptr(temp), _stream()), "segs_eval_frame")


def test_slots_order_scratch_and_repeatability():
    """Three pairs into slots 2, 0, 1 of a four-slot table pre-filled with a sentinel: slot 3 keeps it, the rows depend neither on
    the order of the calls nor on what `temp` held, and two runs are bit-identical."""
    from segs_slam_amd import _capi
    lib = _capi.lib()
    H, W = 37, 53
    pairs = [tuple(t.to(DEV) for t in ref.make_pair(c, H, W)) for c in ("noise", "masked", "smooth")]
    nbytes = lib.segs_eval_temp_bytes(H, W)

    def run(order, fill):
        table = torch.full((4, 8), SENTINEL, device=DEV)
        temp = torch.full((nbytes,), fill, dtype=torch.uint8, device=DEV)
        for i in order:
            _frame(lib, *pairs[i], H, W, True, table, 4, (2, 0, 1)[i], temp)
        torch.cuda.synchronize()
        return table.cpu().numpy()

    a = run((0, 1, 2), 0x00)
    assert (a[3] == SENTINEL).all() and np.isfinite(a[:3]).all() and not (a[:3] == SENTINEL).any()
    for order, fill in (((2, 1, 0), 0x00), ((1, 0, 2), 0xFF), ((0, 1, 2), 0xFF), ((0, 1, 2), 0x00)):
        assert np.array_equal(run(order, fill).view(np.int32), a.view(np.int32)), (order, fill)
    for i, cls in enumerate(("noise", "masked", "smooth")):
        assert ref.case(cls, H, W, True)[2].misses(a[(2, 0, 1)[i]]) == [], cls


@pytest.mark.parametrize("H,W", [(17, 33), (37, 53)])
def test_no_access_next_to_the_buffers(H, W):
    """Inputs, table row, temp and the three byte images in the middle of larger allocations: NaN around the inputs changes
    nothing, the bytes around every output keep their fill, and every output element is written (two fills: an element that
    is skipped cannot equal the expected byte under both)."""
    from segs_slam_amd import _capi
    lib = _capi.lib()
    n, pad = 3 * H * W, 1031
    img, gt = ref.make_pair("masked", H, W)
    fm = ev.FusedImageMetrics(H, W, DEV, 1)
    fm.measure(img.to(DEV), gt.to(DEV), 0, row_mask=True)
    want_row = fm.table.cpu().numpy()[0]
    want_im = ref.images(img, gt, True)
    bufs = []
    for src in (img, gt):
        big = torch.full((n + 2 * pad,), float("nan"), device=DEV)
        big[pad:pad + n] = src.reshape(-1).to(DEV)
        bufs.append(big)
    x, t = bufs[0][pad:pad + n], bufs[1][pad:pad + n]
    nbytes = lib.segs_eval_temp_bytes(H, W)
    temp = torch.full((nbytes + 2 * 4096,), 0xA5, dtype=torch.uint8, device=DEV)
    table = torch.full((3, 8), SENTINEL, device=DEV)
    _frame(lib, x, t, H, W, True, table, 3, 1, temp[4096:])
    torch.cuda.synchronize()
    assert (temp[:4096] == 0xA5).all() and (temp[-4096:] == 0xA5).all()
    got = table.cpu().numpy()
    assert (got[0] == SENTINEL).all() and (got[2] == SENTINEL).all()
    assert np.array_equal(got[1].view(np.int32), want_row.view(np.int32))
    ipad = 1028                                   # keeps the images dword-aligned: both store forms run (W odd here: bytes)
    for fill in (0x5A, 0xA5):
        for flags in (None, temp[4096:]):
            outs = [torch.full((n + 2 * ipad,), fill, dtype=torch.uint8, device=DEV) for _ in range(3)]
            st = lib.segs_eval_images_u8(_ptr(x), _ptr(t), H, W, 1, *(_ptr(o[ipad:]) for o in outs), _ptr(flags), _stream())
            _capi.check(st, "segs_eval_images_u8")
            torch.cuda.synchronize()
            for o, name in zip(outs, ev.IMAGES):
                assert (o[:ipad] == fill).all() and (o[ipad + n:] == fill).all(), name
                assert np.array_equal(o[ipad:ipad + n].cpu().numpy().reshape(H, W, 3), want_im[name]), (name, fill)
    assert (temp[:4096] == 0xA5).all() and (temp[-4096:] == 0xA5).all()


def test_bad_arguments_are_refused_and_touch_nothing():
    from segs_slam_amd import _capi
    lib = _capi.lib()
    H, W = 17, 33
    x, t = (v.to(DEV) for v in ref.make_pair("noise", H, W))
    table = torch.full((4, 8), SENTINEL, device=DEV)
    temp = torch.full((lib.segs_eval_temp_bytes(H, W),), 0xA5, dtype=torch.uint8, device=DEV)
    outs = [torch.full((H, W, 3), 0x5A, dtype=torch.uint8, device=DEV) for _ in range(3)]
    ok = (_ptr(x), _ptr(t), H, W, 1, _ptr(table), 4, 1, _ptr(temp), _stream())
    for at, v in ((0, None), (1, None), (5, None), (8, None), (2, 0), (3, 0), (2, -1), (3, 4097), (7, 4), (7, -1), (6, 0)):
        args = ok[:at] + (v,) + ok[at + 1:]
        assert lib.segs_eval_frame(*args) == -1, (at, v)                      # SEGS_ERR_INVALID_ARGUMENT
        assert b"invalid argument" in lib.segs_last_error()
    ok_im = (_ptr(x), _ptr(t), H, W, 1, *(_ptr(o) for o in outs), _ptr(temp), _stream())
    for at, v in ((0, None), (1, None), (2, 0), (3, 0), (2, 4097)):
        assert lib.segs_eval_images_u8(*(ok_im[:at] + (v,) + ok_im[at + 1:])) == -1, (at, v)
    torch.cuda.synchronize()
    assert (table == SENTINEL).all() and (temp == 0xA5).all() and all((o == 0x5A).all() for o in outs)
    with pytest.raises(ValueError):
        ev.FusedImageMetrics(0, W, DEV, 1)
    with pytest.raises(ValueError):
        ev.FusedImageMetrics(H, W, DEV, 1).measure(x[:, :-1].contiguous(), t, 0)
    with pytest.raises(_capi.SegsError):
        ev.FusedImageMetrics(H, W, DEV, 2).measure(x, t, 2)


# ---- end to end: KeyframeEvaluator on a ScaffoldTrainerStep -------------------------------------------------------------------
XIS = [[0.02, -0.03, 0.015, 0.01, -0.02, 0.03], [-0.04, 0.02, 0.03, -0.02, 0.015, -0.01], [0.05, 0.04, -0.02, 0.02, 0.02, 0.015]]
SHAPES = [(2, 37, (64, 72), False), (0, 4001, (333, 187), True)]


def _step(case, A, W, H, white):
    """A mapper-like step (densification statistics on from the first iteration) and three keyframes at different poses; built
    through tests.test_neural_gpu._setup like tests/test_depth_supervision_gpu._step."""
    from segs_slam_amd import neural_gaussians as ng, scenes
    from segs_slam_amd.densify import AnchorDensifier, DensifyParams
    from segs_slam_amd.pose_refine import KeyframePose
    from tests.test_neural_gpu import CASES, _setup
    dev = torch.device(DEV)
    _, model, _ = _setup(CASES[case], A, 40 + case, dev)
    cam = scenes.make_camera(W, H, 0.9 * W, 0.9 * W, np.eye(3, dtype=np.float32), np.zeros(3, dtype=np.float32))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    kf0 = ng.Keyframe(t(cam.world_view_transform), t(cam.full_proj_transform), t(cam.camera_center),
                      torch.tensor([0.0, 0.1, 0.2, 1.0, 0.0, 0.0, 0.0], device=dev), cam.tanfovx, cam.tanfovy)
    kfs = []
    for xi in XIS:
        pose = KeyframePose(kf0, 1e-3)
        with torch.no_grad():
            pose.xi.copy_(torch.tensor(xi, dtype=torch.float64))
        kfs.append(pose.keyframe())
    step = ng.ScaffoldTrainerStep(model, W, H, scaling_reg_weight=0.01)
    step.set_background(white)
    step.enable_densification(AnchorDensifier(model, DensifyParams(start_stat=0, update_from=1000)), seed=1)
    return step, kfs


def _target(W, H, seed):
    return torch.rand(3, H, W, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))


def _state(step):
    m, d = step.model, step.densifier
    return dict(params=m.params.clone(), grads=m.grads.clone(), exp_avg=m.exp_avg.clone(), exp_avg_sq=m.exp_avg_sq.clone(),
                count=step._mlp_count.words.clone(), stats=d._stats_flat.clone(), delta=d._delta_flat.clone(),
                host=(step._mlp_count.calls, step._anchor_count, step.iteration, step._last_iteration, step.redone_steps,
                      step.W, step.H, m.A, step.use_graph))


def _same_state(a, b):
    for k in a:
        if k == "host":
            assert a[k] == b[k], (a[k], b[k])
        else:
            assert torch.equal(a[k], b[k]), k


def _image_of(step, kf, W, H):
    level = (step.W, step.H)
    step.use_level(W, H)
    im = step.render(kf)
    torch.cuda.synchronize()
    assert step.engine.check()
    im = im.clone()
    step.use_level(*level)
    return im


@pytest.mark.parametrize("case,A,size,white", SHAPES)
def test_evaluate_all_matches_the_chain_and_leaves_training_alone(case, A, size, white):
    """Every row of evaluate_all == the float64 chain on step.render(kf)'s image and the target, within the bars, with
    step.row_mask on and off; one target has a zeroed band, one is a pyramid level below the one in flight (which is restored);
    parameters, gradients, Adam moments and step counts, densification statistics and the step's bookkeeping are bit-equal
    before and after; training goes on afterwards."""
    W, H = size
    step, kfs = _step(case, A, W, H, white)
    assert bool((step.bg == (1.0 if white else 0.0)).all())
    gts = [_target(W, H, 1), _target(W, H, 2), _target(W // 2, H // 2, 3)]
    gts[1][:, H // 4: H // 3] = 0.0
    train_gt = _target(W, H, 4)
    for i in range(3):                      # (the first forwards calibrate; statistics and moments are live afterwards)
        step.training_once(kfs, [train_gt] * 3)
    step.finish()
    torch.cuda.synchronize()
    assert step.iteration == 3 and float(step.densifier._stats_flat.abs().sum()) > 0 and float(step.model.exp_avg.abs().sum()) > 0
    before = _state(step)
    items = [(10 + i, kfs[i], gts[i]) for i in range(3)]
    rows = {}
    for rm in (True, False):
        step.row_mask = rm
        rep = ev.KeyframeEvaluator(step).evaluate_all(items)
        _same_state(before, _state(step))
        assert step.engine.check() and (step.W, step.H) == (W, H)
        assert rep.ids == [10, 11, 12] and rep.table.shape == (3, 8) and rep.images is None
        assert (rep.render_ms > 0).all() and np.isfinite(rep.render_ms).all()
        for i, (_, kf, gt) in enumerate(items):
            img = _image_of(step, kf, gt.shape[-1], gt.shape[-2])
            r = ref.Reference(img.cpu(), gt.cpu(), rm)
            _report_row(f"case {case} kf {i} mask={rm}", r, rep.table[i])
            assert r.misses(rep.table[i]) == [], (i, rm)
        assert abs(rep.psnr_mean - rep.table[:, 1].mean()) < 1e-12 and abs(rep.ssim_mean - rep.table[:, 0].mean()) < 1e-12
        rows[rm] = rep.table
        _same_state(before, _state(step))
    assert rows[True][1, 3] < rows[False][1, 3]          # the zeroed band's error is masked out only with row_mask on
    assert np.array_equal(rows[True][0], rows[False][0])     # a target without an all-zero row: the mask is all ones
    loss = step.training_once(kfs, [train_gt] * 3)
    step.finish()
    assert np.isfinite(float(loss)) and step.iteration == 4 and step.lost_steps() == 0
    assert not torch.equal(step.model.params, before["params"])


def test_record_round_trip(tmp_path):
    """write() with the three record_* switches on: the four text files and the three JPEG files of one keyframe; the text
    parses back to the report's numbers at the printed precision, the recorded bytes are the restatement's."""
    from PIL import Image
    case, A, (W, H), white = SHAPES[0]
    step, kfs = _step(case, A, W, H, white)
    step.row_mask = True
    for _ in range(2):                      # calibrated: the evaluation and the comparison render take the same forward
        step.render(kfs[0])
        torch.cuda.synchronize()
        assert step.engine.check()
    gt = _target(W, H, 5)
    gt[:, H // 4: H // 3] = 0.0
    evaluator = ev.KeyframeEvaluator(step, ev.RecordParams(True, True, True, 3000, 0, 0))
    rep = evaluator.evaluate_all([(42, kfs[0], gt)])
    want = ref.images(_image_of(step, kfs[0], W, H).cpu(), gt.cpu(), True)
    for name in ev.IMAGES:
        assert np.array_equal(rep.images[0][name], want[name]), name
    paths = evaluator.write(rep, str(tmp_path), 3000, "_shutdown")
    d = tmp_path / "3000_shutdown"
    assert sorted(os.path.relpath(p, d) for p in paths) == sorted([
        "render_time.txt", "dssim.txt", "psnr.txt", "psnr_gaussian_splatting.txt", os.path.join("image", "3000_42.jpg"),
        os.path.join("image_gt", "3000_42.jpg"), os.path.join("image_loss", "3000_42_loss.jpg")])
    assert all(os.path.isfile(p) for p in paths)
    for name, col, tol in (("render_time.txt", None, 0.5e-8), ("dssim.txt", "ssim", 0.5e-10), ("psnr.txt", "psnr", 0.5e-10),
                           ("psnr_gaussian_splatting.txt", "psnr_gs", 0.5e-10)):
        lines = (d / name).read_text().splitlines()
        assert lines[0].startswith("##[Gaussian Mapper]") and len(lines) == 2
        kfid, value = lines[1].split(" ")
        have = rep.render_ms[0] if col is None else rep.column(col)[0]
        assert kfid == "42" and abs(float(value) - have) <= tol * 1.0001 and len(value.split(".")[1]) == (8 if col is None else 10)
    for sub, fname in (("image", "3000_42.jpg"), ("image_gt", "3000_42.jpg"), ("image_loss", "3000_42_loss.jpg")):
        with Image.open(d / sub / fname) as im:
            assert im.size == (W, H) and im.mode == "RGB"
