"""GPU parity of the anchor statistics / densification (include/segs_densify.h, segs-slam_amd/densify.py) against the
torch restatement of src/gaussian_model.cpp:1459-1762 (oracle/densify_ref.py).

Integer / index work (which voxels receive an anchor, their order, the per-voxel feature maximum, row compaction) is
compared exactly; the accumulated gradient norms to 1e-6 relative (sqrt rounding)."""
import json
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import densify_ref, neural_ref  # noqa: E402

DIMS = dict(feat_dim=32, n_offsets=10, appearance_dim=0, use_feat_bank=False)
NO = DIMS["n_offsets"]

# ---- the densification settings of every shipped Scaffold configuration (the files that set Model.voxel_size)
SHIPPED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mapper_cfg_values.json")
TUPLE_FIELDS = ("voxel_size", "update_depth", "update_init_factor", "update_hierachy_factor", "densify_grad_threshold",
                "success_threshold", "min_opacity", "update_interval")


def densify_tuple(params):
    """The DensifyParams fields adjust_anchor depends on, in TUPLE_FIELDS order."""
    return tuple(getattr(params, k) for k in TUPLE_FIELDS)


def shipped_densify_tuples():
    """{tuple: [configuration files]} over the committed extract of the shipped configurations, read through mapper_config."""
    from segs_slam_amd import mapper_config as mc
    with open(SHIPPED) as f:
        shipped = json.load(f)
    out = {}
    for rel, values in sorted(shipped.items()):
        if "Model.voxel_size" in values:
            out.setdefault(densify_tuple(mc.mapper_config_from_values(values, rel).densify), []).append(rel)
    return out


def _adjust_cases():
    """Every shipped tuple at 40 anchors and at 2 500 anchors with the capacity one row above A (the storage grows inside
    the call); then a map-sized case per tuple: 300 000 anchors for hierarchy factor 1 (thresholds 0 at levels 1-2, more than
    2^20 candidates at one level), 60 001 and 300 000 (capacity A + 1) in turn for the others."""
    cases, big = [], [(60_001, None), (300_000, 300_001)]
    k = 0
    for t in sorted(shipped_densify_tuples()):
        cases += [(t, 40, None), (t, 2_500, 2_501)]
        if t[3] == 1:
            cases.append((t, 300_000, None))
        else:
            cases.append((t, *big[k % 2]))
            k += 1
    return cases


ADJUST_CASES = _adjust_cases()


def _model(A, seed, dev, capacity=None):
    from segs_slam_amd import neural_gaussians as ng
    rd = neural_ref.NeuralDims(**DIMS)
    g = torch.Generator().manual_seed(seed)
    anchor = torch.rand(A, 3, generator=g) - 0.5
    offset = torch.randn(A, 10, 3, generator=g)
    offset[::7] = 0.0                                        # candidates that fall into their parent's voxel
    feat = torch.randn(A, 32, generator=g)
    scaling_log = torch.log(0.02 + 0.08 * torch.rand(A, 6, generator=g))
    _, _, _, _, mlp = neural_ref.random_model(rd, 1, seed)
    model = ng.ScaffoldModel(A, ng.ModelDims(**DIMS), dev, capacity=capacity)
    model.load(anchor, offset, feat, scaling_log, mlp)
    return model, (anchor, offset, feat, scaling_log), g


def test_training_statis_matches_restatement():
    _check_training_statis(900, 3)


def test_training_statis_at_map_scale():
    """300 000 anchors (3 M candidate slots, 12 000 workgroups of 25 anchors), about 60 % of them visible."""
    _check_training_statis(300_000, 13)


def _check_training_statis(A, seed):
    from segs_slam_amd import densify, neural_gaussians as ng
    dev = torch.device("cuda:0")
    no = 10
    model, _, g = _model(A, seed, dev)
    dens = densify.AnchorDensifier(model)
    gen = ng.NeuralGaussians(model)
    visible = torch.rand(A, generator=g) < 0.6
    nop = torch.tanh(torch.randn(A * no, generator=g))
    nop[~visible.repeat_interleave(no)] = 0.0
    radii = (torch.rand(A * no, generator=g) < 0.5).to(torch.int32) * 4
    g2d = torch.randn(A * no, 3, generator=g)
    gen.neural_opacity.copy_(nop.view(-1, 1))
    vis_radii = visible.to(torch.int32) * 2
    init = {k: torch.rand_like(v.cpu()) for k, v in dens._stats.items()}
    for k, v in init.items():
        dens._stats[k].copy_(v)
    dens.training_statis(gen, vis_radii.to(dev), radii.to(dev), g2d.to(dev))
    torch.cuda.synchronize()

    st = densify_ref.DensifyState(params={}, exp_avg={}, exp_avg_sq={}, opacity_accum=init["opacity_accum"].view(-1, 1).clone(),
                                  anchor_demon=init["anchor_demon"].view(-1, 1).clone(),
                                  offset_gradient_accum=init["offset_gradient_accum"].view(-1, 1).clone(),
                                  offset_denom=init["offset_denom"].view(-1, 1).clone())
    vis_rows = visible.repeat_interleave(no)
    mask = nop[vis_rows] > 0                                   # offset_selection_mask over the visible anchors' slots
    full_mask = torch.zeros(A * no, dtype=torch.bool)
    full_mask[vis_rows] = mask
    densify_ref.training_statis(st, g2d[full_mask], nop[vis_rows].view(-1, 1), radii[full_mask] > 0, mask, visible)
    np.testing.assert_array_equal(dens.stat("anchor_demon").cpu().numpy(), st.anchor_demon.numpy())
    np.testing.assert_array_equal(dens.stat("offset_denom").cpu().numpy(), st.offset_denom.numpy())
    np.testing.assert_allclose(dens.stat("opacity_accum").cpu().numpy(), st.opacity_accum.numpy(), rtol=1e-6)
    np.testing.assert_allclose(dens.stat("offset_gradient_accum").cpu().numpy(), st.offset_gradient_accum.numpy(), rtol=1e-6)


@pytest.mark.parametrize("A,seed,capacity", [(600, 1, None), (2500, 2, 9000), (40, 5, None)])
def test_adjust_anchor_matches_restatement(A, seed, capacity):
    from segs_slam_amd import densify
    dev = torch.device("cuda:0")
    no = 10
    model, (anchor, offset, feat, scaling_log), g = _model(A, seed, dev, capacity)
    P = densify.DensifyParams(voxel_size=0.01, update_depth=3, update_init_factor=16, update_hierachy_factor=4)
    dens = densify.AnchorDensifier(model, P)
    # statistics: about half of the offsets eligible, a third of the anchors old enough to be judged
    denom = torch.floor(torch.rand(A * no, generator=g) * 100)
    accum = torch.rand(A * no, generator=g) * denom * 0.0005
    demon = torch.floor(torch.rand(A, generator=g) * 160)
    opac = torch.rand(A, generator=g) * demon * 0.01
    for k, v in (("offset_denom", denom), ("offset_gradient_accum", accum), ("anchor_demon", demon), ("opacity_accum", opac)):
        dens._stats[k][:v.numel()] = v.to(dev)
    m_rand = {n: torch.randn(A, w, generator=g) for n, w in model.widths.items()}
    v_rand = {n: torch.rand(A, w, generator=g) for n, w in model.widths.items()}
    for n in model.widths:
        model._view(model.exp_avg, n).copy_(m_rand[n].view(model._view(model.exp_avg, n).shape))
        model._view(model.exp_avg_sq, n).copy_(v_rand[n].view(model._view(model.exp_avg_sq, n).shape))
    rands = [torch.rand(A * no, generator=g) for _ in range(3)]

    rot = torch.zeros(A, 4); rot[:, 0] = 1.0
    ref = densify_ref.DensifyState(
        params={"anchor": anchor.clone(), "offset": offset.clone(), "anchor_feat": feat.clone(), "opacity": torch.zeros(A, 1),
                "scaling": scaling_log.clone(), "rotation": rot},
        exp_avg={"anchor": m_rand["anchor"].clone(), "offset": m_rand["offset"].view(A, no, 3).clone(),
                 "anchor_feat": m_rand["anchor_feat"].clone(), "scaling": m_rand["scaling"].clone()},
        exp_avg_sq={"anchor": v_rand["anchor"].clone(), "offset": v_rand["offset"].view(A, no, 3).clone(),
                    "anchor_feat": v_rand["anchor_feat"].clone(), "scaling": v_rand["scaling"].clone()},
        opacity_accum=opac.view(-1, 1).clone(), anchor_demon=demon.view(-1, 1).clone(),
        offset_gradient_accum=accum.view(-1, 1).clone(), offset_denom=denom.view(-1, 1).clone(),
        voxel_size=0.01, update_depth=3, update_init_factor=16, update_hierachy_factor=4)
    ref_prune = densify_ref.adjust_anchor(ref, 100, 0.8, 0.0002, 0.005, rands)

    prune = dens.adjust_anchor(100, 0.8, 0.0002, 0.005, rands=[r.to(dev) for r in rands])
    torch.cuda.synchronize()
    grown = ref_prune.shape[0] - A
    assert grown > 0 and int(ref_prune.sum()) > 0, "the case must exercise both growing and pruning"
    _assert_same_map(model, dens, prune, ref, ref_prune)


def _assert_same_map(model, dens, prune, ref, ref_prune):
    """Every output of adjust_anchor equal to the restatement's: integer and row outputs exactly, scaling to 1e-6."""
    A1 = ref.params["anchor"].shape[0]
    assert model.A == A1
    np.testing.assert_array_equal(prune.cpu().numpy(), ref_prune.numpy())
    eq = lambda a, b, msg: np.testing.assert_array_equal(a.cpu().numpy(), b.numpy(), err_msg=msg)  # noqa: E731
    eq(model.param("anchor"), ref.params["anchor"], "anchor")
    eq(model.param("offset"), ref.params["offset"], "offset")
    eq(model.param("anchor_feat"), ref.params["anchor_feat"], "anchor_feat")
    np.testing.assert_allclose(model.param("scaling").cpu().numpy(), ref.params["scaling"].numpy(), rtol=0, atol=1e-6)
    eq(model.rotation[:A1], ref.params["rotation"], "rotation")
    np.testing.assert_allclose(model.opacity[:A1].cpu().numpy(), ref.params["opacity"].numpy(), atol=1e-6)
    for n in ("anchor", "offset", "anchor_feat", "scaling"):
        eq(model._view(model.exp_avg, n), ref.exp_avg[n], "exp_avg " + n)
        eq(model._view(model.exp_avg_sq, n), ref.exp_avg_sq[n], "exp_avg_sq " + n)
    for k in ("opacity_accum", "anchor_demon", "offset_gradient_accum", "offset_denom"):
        eq(dens.stat(k), getattr(ref, k), k)


def _densifier_with_state(model, t, denom, accum, demon, opac, g):
    """An AnchorDensifier of `model` at the settings of tuple `t`, its statistics set to the given values and the Adam
    moments of every anchor row random; returns it with the restatement's DensifyState of the same map."""
    from segs_slam_amd import densify
    dev = model.device
    A = model.A
    anchor, offset, feat, scaling_log = (model.param(n).cpu() for n in ("anchor", "offset", "anchor_feat", "scaling"))
    kw = dict(zip(TUPLE_FIELDS, t))
    dens = densify.AnchorDensifier(model, densify.DensifyParams(**kw))
    for k, v in (("offset_denom", denom), ("offset_gradient_accum", accum), ("anchor_demon", demon), ("opacity_accum", opac)):
        dens._stats[k][:v.numel()] = v.to(dev)
    m_rand = {n: torch.randn(A, w, generator=g) for n, w in model.widths.items()}
    v_rand = {n: torch.rand(A, w, generator=g) for n, w in model.widths.items()}
    for n in model.widths:
        model._view(model.exp_avg, n).copy_(m_rand[n].view(model._view(model.exp_avg, n).shape))
        model._view(model.exp_avg_sq, n).copy_(v_rand[n].view(model._view(model.exp_avg_sq, n).shape))
    rot = torch.zeros(A, 4)
    rot[:, 0] = 1.0
    moments = lambda d: {"anchor": d["anchor"], "offset": d["offset"].view(A, NO, 3), "anchor_feat": d["anchor_feat"],  # noqa: E731
                         "scaling": d["scaling"]}
    ref = densify_ref.DensifyState(
        params={"anchor": anchor, "offset": offset, "anchor_feat": feat, "opacity": torch.zeros(A, 1), "scaling": scaling_log,
                "rotation": rot},
        exp_avg=moments(m_rand), exp_avg_sq=moments(v_rand), opacity_accum=opac.view(-1, 1).clone(),
        anchor_demon=demon.view(-1, 1).clone(), offset_gradient_accum=accum.view(-1, 1).clone(),
        offset_denom=denom.view(-1, 1).clone(), voxel_size=kw["voxel_size"], update_depth=kw["update_depth"],
        update_init_factor=kw["update_init_factor"], update_hierachy_factor=kw["update_hierachy_factor"])
    return dens, ref


def _level_sizes(t):
    """cur_size of every growing level, as anchor_growing forms it (a float32 value)."""
    vs, depth, init, hier = t[:4]
    return [float(torch.tensor(vs * math.floor(init / hier ** i), dtype=torch.float32)) for i in range(depth)]


# ---- tie policy of the map-scale cases.  The device forms xyz = anchor + offset * expf(scaling) and rintf(xyz / cur_size),
# the restatement the same float32 operations with CPU torch.exp; the two exp implementations may differ by 1 ulp.
#  * Directly that moves xyz by |offset * exp(s)| * 2^-23 at most: <= 0.12 m * 1.19e-7 = 1.4e-8 m for the N(0,1) offsets and
#    exp(s) <= 0.03 used here (6e-9 m for the 5-cm cluster slots), i.e. <= 1.4e-5 voxel at 1 mm -- TIE_MARGIN = 1e-4 voxel
#    is 7x that for the largest offsets and 16x for the cluster slots.  A slot whose float64 xyz / cur_size lies within
#    TIE_MARGIN of a half-integer at any level is redrawn.
#  * But when the float32 sum anchor + offset * exp(s) then rounds to the neighbouring float, xyz moves by 1 ulp of xyz:
#    2.4e-7 m for |xyz| < 4 m, 2.4e-4 voxel at 1 mm, more than the margin.  So a slot is also redrawn when its voxel changes
#    at some level with exp(s) moved 1 ulp either way in the float32 formula.  Any two exp implementations that are each
#    within 1 ulp of the true value return one of the two floats around it, so this covers every such pair exactly.
TIE_MARGIN = 1e-4


def _redraw_ties(anchor, offset, scaling_log, sizes, g):
    """Redraws (in place) the offsets of the slots the tie policy above excludes; returns (slots flagged at the first pass,
    redraws in all)."""
    a32 = anchor.unsqueeze(1)
    e = torch.exp(scaling_log)[:, :3].unsqueeze(1)                     # the restatement's float32 exp, same call
    e_ulp = (torch.nextafter(e, torch.zeros_like(e)), torch.nextafter(e, torch.full_like(e, math.inf)))
    e64 = torch.exp(scaling_log.double())[:, :3].unsqueeze(1)
    first, total = None, 0
    while True:
        q64 = anchor.double().unsqueeze(1) + offset.double() * e64
        bad = torch.zeros(offset.shape[:2], dtype=torch.bool)
        for cs in sorted(set(sizes)):
            q = q64 / cs
            bad |= ((q - torch.floor(q) - 0.5).abs() < TIE_MARGIN).any(-1)
            v = torch.round((a32 + offset * e) / cs)
            for e2 in e_ulp:
                bad |= (torch.round((a32 + offset * e2) / cs) != v).any(-1)
        n = int(bad.sum())
        first = n if first is None else first
        if n == 0:
            return first, total
        total += n
        offset[bad] = torch.randn(n, 3, generator=g)


BOX_LO, BOX_EXT = torch.tensor([-3.0, -2.0, -1.5]), torch.tensor([6.0, 4.0, 3.0])      # a Replica-sized room around the origin


def _map_scene(A, t, seed):
    """Anchors in a 6 x 4 x 3 m room, log-scales near the 1-mm grid, N(0,1) offsets; every 7th anchor's offsets tiny
    (candidates in the parent's own voxel); the last ~10 % of the anchors in clusters of 12 parents within 2 mm whose slot k
    all point at one spot 5 cm away (long runs of candidates of many parents in one voxel: the per-voxel feature maximum);
    statistics scaled to the tuple so that every level grows and pruning happens, 5 % of the gradients exactly 0."""
    g = torch.Generator().manual_seed(seed)
    anchor = torch.rand(A, 3, generator=g) * BOX_EXT + BOX_LO
    scaling_log = torch.log(0.002 + 0.028 * torch.rand(A, 6, generator=g))
    offset = torch.randn(A, NO, 3, generator=g)
    offset[::7] *= 1e-3
    n_cl = max(1, A // 120)
    first = A - 12 * n_cl
    centre = anchor[first::12][:n_cl]
    member = centre.repeat_interleave(12, 0) + (torch.rand(12 * n_cl, 3, generator=g) - 0.5) * 0.004
    anchor[first:] = member
    target = centre.unsqueeze(1) + 0.05 * torch.nn.functional.normalize(torch.randn(n_cl, NO, 3, generator=g), dim=-1)
    offset[first:] = (target.repeat_interleave(12, 0) - member.unsqueeze(1)) / torch.exp(scaling_log[first:, :3]).unsqueeze(1)
    first_pass, redraws = _redraw_ties(anchor, offset, scaling_log, _level_sizes(t), g)
    feat = torch.randn(A, 32, generator=g)
    interval, thr, min_op = t[7], t[4], t[6]
    denom = torch.floor(torch.rand(A * NO, generator=g) * interval)     # offset_mask (> 0.4 interval): ~60 % of the slots
    accum = torch.rand(A * NO, generator=g) * denom * (8 * thr)          # gradient ~ U(0, 8 thr): every level's threshold cuts
    accum[torch.rand(A * NO, generator=g) < 0.05] = 0.0
    demon = torch.floor(torch.rand(A, generator=g) * 2 * interval)      # judged (> 0.8 interval): ~60 % of the anchors
    opac = torch.rand(A, generator=g) * demon * 2 * min_op              # half of the judged ones pruned
    rands = [torch.rand(A * NO, generator=g) for _ in range(t[1])]
    return (anchor, offset, feat, scaling_log), (denom, accum, demon, opac), rands, (first_pass, redraws), g


@pytest.mark.parametrize("t,A,capacity", ADJUST_CASES, ids=[f"hier{t[3]}-thr{t[4]}-every{t[7]}-A{A}" for t, A, _ in ADJUST_CASES])
def test_adjust_anchor_at_shipped_settings(t, A, capacity):
    """adjust_anchor at every shipped densification tuple, up to map size: growth at 1/4/16-mm voxels in a room-sized map,
    pruning, storage growth, and -- at 300 000 anchors with hierarchy factor 1 -- more than 2^20 candidates at one level
    (scan_sums_kernel past its first round, 63-bit keys sorted in the millions).  Exact parity under the tie policy above."""
    from segs_slam_amd import neural_gaussians as ng
    dev = torch.device("cuda:0")
    seed = 1000 + A % 977 + 10 * t[3] + int(1e5 * t[4]) + t[7]
    (anchor, offset, feat, scaling_log), (denom, accum, demon, opac), rands, (first_pass, redraws), g = _map_scene(A, t, seed)
    assert first_pass < 0.005 * A * NO, f"the tie policy redrew {first_pass} of {A * NO} slots"
    _, _, _, _, mlp = neural_ref.random_model(neural_ref.NeuralDims(**DIMS), 1, seed)
    model = ng.ScaffoldModel(A, ng.ModelDims(**DIMS), dev, capacity=capacity)
    model.load(anchor, offset, feat, scaling_log, mlp)
    dens, ref = _densifier_with_state(model, t, denom, accum, demon, opac, g)
    interval, success, thr, min_op = t[7], t[5], t[4], t[6]
    trace = []
    ref_prune = densify_ref.adjust_anchor(ref, interval, success, thr, min_op, rands, trace=trace)
    prune = dens.adjust_anchor(interval, success, thr, min_op, rands=[r.to(dev) for r in rands])
    torch.cuda.synchronize()
    info = f"tie-redrawn slots {first_pass} (redraws {redraws}) of {A * NO}; levels {trace}"
    assert len(trace) == t[1] and all(lv["new"] > 0 for lv in trace) and int(ref_prune.sum()) > 0, info
    if capacity is not None:
        assert model.capacity > capacity, info                     # the storage grew inside the call
    if A >= 2_500:
        assert sum(lv["in_grown"] for lv in trace) > 0, info       # candidates in voxels an earlier level of this call filled
    if t[3] == 1:
        grads = (accum / denom).nan_to_num(0.0)
        zero_in = (grads == 0) & (denom > interval * success * 0.5) & (rands[1] > 0.25)
        assert int(zero_in.sum()) > 0, info                         # threshold 0 at level 1 admits gradient-0 slots (>=)
        if A == 300_000:
            assert max(lv["candidates"] for lv in trace) > 1 << 20, info
    _assert_same_map(model, dens, prune, ref, ref_prune)


def test_adjust_anchor_rounds_exact_half_voxels_to_even():
    """Candidates exactly on half-integer voxel coordinates, on both sides of zero: voxel_size = 2^-10 makes every cur_size a
    power of two and scaling_log = 0 makes exp exactly 1, so xyz / cur_size is exact on both sides.  The device's rintf and
    the restatement's torch.round both round half to even; round-half-away (roundf) places other voxels."""
    from segs_slam_amd import neural_gaussians as ng
    dev = torch.device("cuda:0")
    t = (2.0 ** -10, 3, 16, 4, 1e-3, 0.8, 0.005, 100)
    A = 32
    g = torch.Generator().manual_seed(77)
    anchor = torch.zeros(A, 3)
    anchor[:, 0] = 1.0 + torch.arange(A) / 16.0                   # parents on the grid, far from the candidates
    anchor[:, 1:] = 1.0
    level = torch.arange(A * NO) % 2                               # half of the slots tie at level 0 (2^-6), half at level 2
    cs = torch.where(level == 0, 2.0 ** -6, 2.0 ** -10).unsqueeze(1)
    k = torch.randint(-6, 6, (A * NO, 3), generator=g).float()
    target = (k + 0.5) * cs                                        # exact half-integers of that level's voxel
    offset = (target - anchor.repeat_interleave(NO, 0)).view(A, NO, 3)
    assert torch.equal(anchor.repeat_interleave(NO, 0) + offset.view(-1, 3), target)
    scaling_log = torch.zeros(A, 6)
    feat = torch.randn(A, 32, generator=g)
    _, _, _, _, mlp = neural_ref.random_model(neural_ref.NeuralDims(**DIMS), 1, 77)
    model = ng.ScaffoldModel(A, ng.ModelDims(**DIMS), dev)
    model.load(anchor, offset, feat, scaling_log, mlp)
    denom = torch.full((A * NO,), 100.0)
    accum = torch.full((A * NO,), 100.0)                            # gradient 1 >= 4 thr: a candidate at every level
    dens, ref = _densifier_with_state(model, t, denom, accum, torch.zeros(A), torch.zeros(A), g)
    rands = [torch.full((A * NO,), 0.99) for _ in range(3)]
    trace = []
    ref_prune = densify_ref.adjust_anchor(ref, 100, 0.8, 1e-3, 0.005, rands, trace=trace)
    prune = dens.adjust_anchor(100, 0.8, 1e-3, 0.005, rands=[r.to(dev) for r in rands])
    torch.cuda.synchronize()
    # the restatement's first level is round-half-to-even, and round-half-away would differ from it
    q = (target / 2.0 ** -6).numpy()
    even = np.unique(np.rint(q) + 0.0, axis=0)
    away = np.unique(np.trunc(q + np.copysign(0.5, q)) + 0.0, axis=0)
    n0 = trace[0]["new"]
    assert n0 == even.shape[0] and not np.array_equal(even, away)
    np.testing.assert_array_equal(ref.params["anchor"][A:A + n0].numpy(), (even * 2.0 ** -6).astype(np.float32))
    _assert_same_map(model, dens, prune, ref, ref_prune)


def test_trainer_keeps_running_through_densification():
    from segs_slam_amd import densify, neural_gaussians as ng, scenes
    dev = torch.device("cuda:0")
    cam = scenes.make_camera(320, 240, 300.0, 300.0, np.eye(3, dtype=np.float32), np.zeros(3, dtype=np.float32))
    model = ng.synthetic_model(3000, ng.ModelDims(), cam, dev, seed=4)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    kf = ng.Keyframe(t(cam.world_view_transform), t(cam.full_proj_transform), t(cam.camera_center),
                     torch.tensor([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0], device=dev), cam.tanfovx, cam.tanfovy)
    step = ng.ScaffoldTrainerStep(model, cam.width, cam.height)
    dens = densify.AnchorDensifier(model, densify.DensifyParams(voxel_size=0.01, start_stat=2, update_from=5, update_interval=10,
                                                                update_until=1000, densify_grad_threshold=1e-7))
    step.enable_densification(dens, seed=0)
    gt = torch.full((3, cam.height, cam.width), 0.4, device=dev)
    sizes = []
    for it in range(1, 32):
        loss = step.training_once([kf], [gt])
        sizes.append(model.A)
        assert np.isfinite(float(loss))
    assert sizes[-1] != 3000, sizes[::5]      # the map changed size and the step kept running
    # anchor tensors are skipped by Adam at the 3 densify iterations; a pass right after the map grew may outgrow the resident
    # scratch and is then dropped ON THE DEVICE (both counts stay put), so the counts say how many steps were really taken
    mlp, anchor = step._mlp_count.value(), step._anchor_count.value()
    assert mlp - anchor == 3 and 28 <= mlp <= 31, (mlp, anchor)


def test_trainer_survives_a_map_pruned_to_nothing():
    """All anchors pruned: the reference's rasterizer short-circuits P == 0 to a zero image (src/rasterize_points.cu:81);
    the step must keep running (loss against the zero image, no gradient) rather than fault."""
    from segs_slam_amd import densify, neural_gaussians as ng, scenes
    dev = torch.device("cuda:0")
    cam = scenes.make_camera(96, 64, 90.0, 90.0, np.eye(3, dtype=np.float32), np.zeros(3, dtype=np.float32))
    model = ng.synthetic_model(200, ng.ModelDims(), cam, dev, seed=5)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    kf = ng.Keyframe(t(cam.world_view_transform), t(cam.full_proj_transform), t(cam.camera_center),
                     torch.tensor([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0], device=dev), cam.tanfovx, cam.tanfovy)
    step = ng.ScaffoldTrainerStep(model, cam.width, cam.height)
    dens = densify.AnchorDensifier(model, densify.DensifyParams(voxel_size=0.01, start_stat=2, update_from=5, update_interval=10,
                                                                update_until=1000))
    step.enable_densification(dens, seed=0)
    gt = torch.full((3, cam.height, cam.width), 0.4, device=dev)
    step.training_once([kf], [gt])
    dens.prune_anchor(torch.ones(model.A, dtype=torch.bool, device=dev))
    assert model.A == 0
    for _ in range(12):                      # crosses a densify iteration with A == 0
        loss = step.training_once([kf], [gt])
    torch.cuda.synchronize()
    assert abs(float(loss) - (0.8 * 0.4 + 0.2 * 1.0)) < 0.05      # L1 = 0.4 against zeros, SSIM ~ 0


def test_create_from_pcd_and_increase_pcd_match_restatement():
    """GaussianModel::createFromPcd / increasePcd (src/gaussian_model.cpp:327-381, 443-520) restated on the CPU: voxel centres
    by torch.unique over round(points / voxel_size), scales from the oracle's simple-knn (tests/test_points.py pins the GPU
    kernel to it bit for bit)."""
    from oracle import gs_oracle
    from segs_slam_amd import densify, neural_gaussians as ng, scenes
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(11)
    vs = 0.05
    pts = torch.rand(6000, 3, generator=g) * torch.tensor([2.0, 1.5, 1.0]) + torch.tensor([-1.0, -0.75, 2.0])
    pts = torch.cat([pts, pts[:1500] + 0.004])                 # near-duplicates: many land in an occupied voxel

    def restate(p):
        u = (torch.unique(torch.round(p / vs), dim=0, sorted=True) * vs).to(torch.float32)
        d2 = torch.from_numpy(gs_oracle.knn_mean_dist2(u.numpy())).clamp_min(0.0000001)
        return u, torch.log(torch.sqrt(d2)).unsqueeze(1).repeat(1, 6)

    model = ng.create_from_pcd(pts, ng.ModelDims(), vs, dev)
    u, sc = restate(pts)
    A = u.shape[0]
    assert model.A == A and A < pts.shape[0]
    assert torch.equal(model.param("anchor").cpu(), u)
    assert torch.allclose(model.param("scaling").cpu(), sc, rtol=1e-6, atol=1e-6)
    assert float(model.param("offset").abs().max()) == 0.0 and float(model.param("anchor_feat").abs().max()) == 0.0
    assert torch.allclose(model.opacity[:A].cpu(), torch.full((A, 1), float(np.log(0.1 / 0.9))), atol=1e-6)
    assert torch.equal(model.rotation[:A].cpu(), torch.tensor([[1.0, 0.0, 0.0, 0.0]]).repeat(A, 1))
    w = model.param("mlp_cov.0.weight")
    assert float(w.abs().max()) <= 1.0 / np.sqrt(w.shape[1]) and float(w.abs().max()) > 0.0      # nn::Linear's default range

    # increasePcd: new voxels appended (unique among themselves only), counters and Adam moments of the new rows zero
    dens = densify.AnchorDensifier(model, densify.DensifyParams(voxel_size=vs))
    model.exp_avg.fill_(0.5)
    new = torch.rand(900, 3, generator=g) * torch.tensor([1.0, 1.0, 0.5]) + torch.tensor([1.2, -0.5, 2.2])
    new = torch.cat([new, pts[:50]])                            # some fall into voxels that already hold an anchor: kept, like the reference
    n_new = dens.increase_pcd(new.to(dev))
    u2, sc2 = restate(new)
    assert n_new == u2.shape[0] and model.A == A + n_new
    assert torch.equal(model.param("anchor")[A:].cpu(), u2) and torch.equal(model.param("anchor")[:A].cpu(), u)
    assert torch.allclose(model.param("scaling")[A:].cpu(), sc2, rtol=1e-6, atol=1e-6)
    for name in model.widths:
        assert float(model._view(model.exp_avg, name)[A:].abs().max()) == 0.0
        assert float(model._view(model.exp_avg, name)[:A].min()) == 0.5
    assert float(dens.stat("offset_denom")[A * 10:].abs().max()) == 0.0 and float(dens.stat("anchor_demon")[A:].abs().max()) == 0.0
    assert dens.increase_pcd(torch.zeros(0, 3, device=dev)) == 0

    # the grown model trains
    cam = scenes.make_camera(160, 120, 150.0, 150.0, np.eye(3, dtype=np.float32), np.zeros(3, dtype=np.float32))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    kf = ng.Keyframe(t(cam.world_view_transform), t(cam.full_proj_transform), t(cam.camera_center),
                     torch.tensor([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0], device=dev), cam.tanfovx, cam.tanfovy)
    model.exp_avg.zero_()
    step = ng.ScaffoldTrainerStep(model, cam.width, cam.height)
    gt = torch.full((3, cam.height, cam.width), 0.5, device=dev)
    losses = [float(step.training_once([kf], [gt])) for _ in range(30)]
    assert np.isfinite(losses).all() and losses[-1] < losses[0]


def test_create_from_pcd_and_increase_pcd_at_millimetre_voxels():
    """createFromPcd / increasePcd at the shipped voxel_size = 0.001 on dense depth surfaces: more than 65 536 anchors, so
    simple-knn runs past its first round of 256 candidate boxes; the same assertions as at 5-cm voxels."""
    from segs_slam_amd import densify, neural_gaussians as ng
    from tests.test_points import depth_surface_points, knn_oracle
    dev = torch.device("cuda:0")
    vs = 0.001

    def restate(p):
        u = (torch.unique(torch.round(p / vs), dim=0, sorted=True) * vs).to(torch.float32)
        d2 = torch.from_numpy(knn_oracle(u.numpy())).clamp_min(0.0000001)
        return u, torch.log(torch.sqrt(d2)).unsqueeze(1).repeat(1, 6)

    def off_ties(p):
        # torch divides a GPU tensor by a scalar as a multiplication by its reciprocal, the CPU divides: the quotients may
        # differ by an ulp (6e-5 voxel at 0.6 m), so points within 1e-3 voxel of a half-integer are left out
        q = p.double() / vs
        return p[((q - torch.floor(q) - 0.5).abs() > 1e-3).all(1)]

    pts = off_ties(torch.from_numpy(depth_surface_points(480, 360, 700.0, 31)))
    model = ng.create_from_pcd(pts, ng.ModelDims(), vs, dev)
    u, sc = restate(pts)
    A = u.shape[0]
    assert model.A == A and 65_536 < A < pts.shape[0]
    assert torch.equal(model.param("anchor").cpu(), u)
    assert torch.allclose(model.param("scaling").cpu(), sc, rtol=1e-6, atol=1e-6)
    dens = densify.AnchorDensifier(model, densify.DensifyParams(voxel_size=vs))
    new = torch.from_numpy(depth_surface_points(320, 240, 500.0, 32)) + torch.tensor([0.05, -0.02, 0.3])
    new = off_ties(torch.cat([new, pts[:5000]]))                # some fall into voxels that already hold an anchor: kept
    n_new = dens.increase_pcd(new.to(dev))
    u2, sc2 = restate(new)
    assert n_new == u2.shape[0] and model.A == A + n_new
    assert torch.equal(model.param("anchor")[A:].cpu(), u2) and torch.equal(model.param("anchor")[:A].cpu(), u)
    assert torch.allclose(model.param("scaling")[A:].cpu(), sc2, rtol=1e-6, atol=1e-6)


def test_coarse_anchor_set_is_created_and_grown_like_the_reference():
    """Model.use_coarse_anchor = 1: createCoarseAnchorFromPcd / increasePcdCoarse (src/gaussian_model.cpp:288-325, 383-441)
    restated with torch.unique and the oracle's simple-knn, quirks included -- the coarse set is rounded at coarse_voxel_size but
    PLACED at unique * voxel_size (:290-291), and grown at the fine voxel size (:385-386); offsets and features take the FINE
    n_offsets / feat_dim.  The set is an inert payload: the step trains exactly as without it and never touches it."""
    from oracle import gs_oracle
    from segs_slam_amd import coarse_anchors as ca, densify, mapper_config as mc, neural_gaussians as ng, scenes
    dev = torch.device("cuda:0")
    cfg = mc.load_committed_config("cfg/colmap/gaussian_splatting.yaml")
    g = torch.Generator().manual_seed(21)
    vs, cvs = 0.05, cfg.coarse.coarse_voxel_size
    pts = torch.rand(8000, 3, generator=g) * torch.tensor([2.0, 1.5, 1.0]) + torch.tensor([-1.0, -0.75, 2.0])

    def restate(p, round_size, place_size):
        u = (torch.unique(torch.round(p / round_size), dim=0, sorted=True) * place_size).to(torch.float32)
        d2 = torch.from_numpy(gs_oracle.knn_mean_dist2(u.numpy())).clamp_min(0.0000001)
        return u, torch.log(torch.sqrt(d2)).unsqueeze(1).repeat(1, 6)

    model = ng.create_from_pcd(pts, cfg.model, vs, dev, coarse=cfg.coarse)
    plain = ng.create_from_pcd(pts, cfg.model, vs, dev)
    c = model.coarse
    u, sc = restate(pts, cvs, vs)
    assert isinstance(c, ca.CoarseAnchors) and c.n == u.shape[0] and 0 < c.n < model.A          # 0.2-m voxels: far fewer than the fine set
    assert torch.equal(c.anchor.cpu(), u) and torch.allclose(c.scaling.cpu(), sc, rtol=1e-6, atol=1e-6)
    assert c.offset.shape == (c.n, cfg.model.n_offsets, 3) and c.anchor_feat.shape == (c.n, cfg.model.feat_dim)
    assert float(c.offset.abs().max()) == 0.0 and float(c.anchor_feat.abs().max()) == 0.0
    assert torch.equal(c.rotation.cpu(), torch.tensor([[1.0, 0.0, 0.0, 0.0]]).repeat(c.n, 1))
    assert torch.allclose(c.opacity.cpu(), torch.full((c.n, 1), float(np.log(0.1 / 0.9))), atol=1e-6)
    for name, shape in ca.coarse_mlp_shapes(cfg.model, cfg.coarse).items():
        assert tuple(c.mlp[name].shape) == shape and float(c.mlp[name].abs().max()) > 0
    names = [n for n, _, _ in c.optimizer_groups(0)]
    assert names == ["anchor_c", "offset_c", "anchor_feat_c", "opacity_c", "scaling_c", "rotation_c", "mlp_opacity_c", "mlp_cov_c",
                     "mlp_color_c", "mlp_apperance_c"]                                           # :730-758 (appearance, no feature bank)
    lr = {n: v for n, _, v in c.optimizer_groups(15000)}
    assert lr["anchor_c"] == 0.0 and lr["offset_c"] == pytest.approx(0.001) and lr["mlp_cov_c"] == pytest.approx(0.004)
    # the fine set is what it is without the coarse one
    assert torch.equal(model.params, plain.params)

    # increasePcd -> increasePcdCoarse: the same new points, rounded and placed at the FINE voxel size, appended
    dens = densify.AnchorDensifier(model, densify.DensifyParams(voxel_size=vs))
    new = torch.rand(700, 3, generator=g) * torch.tensor([1.0, 1.0, 0.5]) + torch.tensor([1.2, -0.5, 2.2])
    n0 = c.n
    n_new = dens.increase_pcd(new.to(dev))
    u2, sc2 = restate(new, vs, vs)
    assert n_new == u2.shape[0] and c.n == n0 + u2.shape[0]
    assert torch.equal(c.anchor[n0:].cpu(), u2) and torch.equal(c.anchor[:n0].cpu(), u)
    assert torch.allclose(c.scaling[n0:].cpu(), sc2, rtol=1e-6, atol=1e-6) and c.max_radii2D.shape == (c.n,)

    # a mapper step of this configuration takes the model; training leaves the coarse set bit for bit alone
    cam = scenes.make_camera(160, 120, 150.0, 150.0, np.eye(3, dtype=np.float32), np.zeros(3, dtype=np.float32))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    kf = ng.Keyframe(t(cam.world_view_transform), t(cam.full_proj_transform), t(cam.camera_center),
                     torch.tensor([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0], device=dev), cam.tanfovx, cam.tanfovy)
    step = mc.make_mapper_step(cfg, model, cam.width, cam.height)
    before = {k: v.clone() for k, v in (("anchor", c.anchor), ("scaling", c.scaling), ("w", c.mlp["mlp_cov_c.0.weight"]))}
    gt = torch.full((3, cam.height, cam.width), 0.5, device=dev)
    losses = [float(step.training_once([kf], [gt])) for _ in range(10)]
    assert np.isfinite(losses).all()
    assert torch.equal(before["anchor"], c.anchor) and torch.equal(before["scaling"], c.scaling) and torch.equal(before["w"], c.mlp["mlp_cov_c.0.weight"])
