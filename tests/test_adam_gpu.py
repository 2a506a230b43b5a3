"""The fused multi-segment Adam (csrc/optim.hip: segs_adam_step, _guarded, _device, _graph, segs_set_doubles) bit for bit against
the float32 restatement of LibTorch's step (tests/_adam_ref.py), at every segment alignment and count around the vector body, with
guard elements around every segment: inside a segment the four arrays equal the restatement, outside they keep their bits --
gradients included, which a launch may only clear inside its segments.  FusedAdam.step(exchange=...) and ScaffoldTrainerStep._adam
hand the kernel shards clipped at arbitrary points and rely on exactly that."""
import ctypes as C

import numpy as np
import pytest
import torch

from ._adam_ref import adam_float64, adam_reference

DEV = "cuda:0"
B1, B2, EPS = 0.9, 0.999, 1e-15
GUARD = 8
COUNTS = (0, 1, 2, 3, 4, 5, 7, 8, 4095, 4096, 4097, 4103, 8197)
ERR = -1     # SEGS_ERR_INVALID_ARGUMENT


# ---- the pin itself (no GPU) ------------------------------------------------------------------------------------------------

def test_restatement_stays_within_a_few_ulp_of_float64_per_step():
    """50 steps of the float32 restatement; at every step the float64 update FROM THE SAME STATE differs by no more than the
    roundings the restatement makes (u = 2^-24 each): exp_avg 4 u (|m b1| + |g (1-b1)|) (two products, a sum, the rounded
    constants), exp_avg_sq 6 u v, the parameter update 12 u |upd| plus what exp_avg's error contributes, and u |p| (half an ulp)
    for the final subtraction."""
    rng = np.random.default_rng(11)
    n, lr, u = 4001, 5e-3, 2.0 ** -24
    p = rng.standard_normal(n).astype(np.float32)
    m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    for step in range(1, 51):
        g = (rng.standard_normal(n) * 1e-3 * rng.choice([1.0, 30.0, 1e-3], n)).astype(np.float32)
        p2, m2, v2 = adam_reference(p, g, m, v, lr, B1, B2, EPS, step, 0.5)
        p64, m64, v64, upd = adam_float64(p, g, m, v, lr, B1, B2, EPS, step, 0.5)
        dm = np.abs(m2 - m64)
        assert (dm <= 4 * u * (np.abs(m * B1) + np.abs(g * 0.5 * (1 - B1)))).all()
        assert (np.abs(v2 - v64) <= 6 * u * v64).all()
        per_m = (lr / (1 - B1 ** step)) / (np.sqrt(v64) / np.sqrt(1 - B2 ** step) + EPS)       # d upd / d exp_avg
        dp = np.abs(p2 - p64)
        assert (dp <= u * np.maximum(np.abs(p64), np.abs(p2)) + 12 * u * np.abs(upd) + per_m * dm).all()
        p, m, v = p2, m2, v2


# ---- helpers ---------------------------------------------------------------------------------------------------------------

def _lay(cells, first=GUARD):
    """Segments (offset, count) for cells (offset mod 4, count), >= GUARD elements before, between and after them; total size."""
    segs, pos = [], first
    for r, cnt in cells:
        pos += GUARD
        pos += (r - pos) % 4
        segs.append((pos, cnt))
        pos += cnt
    return segs, pos + GUARD + 3


def _arrays(n, seed):
    """p, g, m, v with distinct values everywhere (guards included)."""
    rng = np.random.default_rng(seed)
    p = rng.standard_normal(n).astype(np.float32)
    g = (rng.standard_normal(n) * 1e-3).astype(np.float32)
    m = (rng.standard_normal(n) * 1e-4).astype(np.float32)
    v = (rng.random(n) * 1e-6 + 1e-12).astype(np.float32)
    return [p, g, m, v]


def _dev(arrs):
    return [torch.from_numpy(a.copy()).to(DEV) for a in arrs]


def _host(tens):
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in tens]


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _table(segs):
    from segs_slam_amd import _capi
    tab = (_capi.AdamSegment * max(len(segs), 1))()
    for i, (o, n, lr) in enumerate(segs):
        tab[i].offset, tab[i].count, tab[i].lr = o, n, lr
    return tab


def _step(tens, segs, step, gscale=1.0, zero_grad=1, nseg=None):
    """segs_adam_step (host step count); returns the status."""
    from segs_slam_amd import _capi
    return _capi.lib().segs_adam_step(*map(_ptr, tens), _table(segs), len(segs) if nseg is None else nseg, B1, B2, EPS, step,
                                      gscale, zero_grad, _stream())


def _step_device(tens, segs, words, call, gscale=1.0, zero_grad=1, skip=None):
    from segs_slam_amd import _capi
    return _capi.lib().segs_adam_step_device(*map(_ptr, tens), _table(segs), len(segs), B1, B2, EPS, _ptr(words), call, gscale,
                                             zero_grad, _ptr(skip), _stream())


def _step_graph(tens, segs, lr_table, words, gscale=1.0, zero_grad=1, skip=None):
    from segs_slam_amd import _capi
    return _capi.lib().segs_adam_step_graph(*map(_ptr, tens), _table(segs), len(segs), _ptr(lr_table), B1, B2, EPS, _ptr(words),
                                            gscale, zero_grad, _ptr(skip), _stream())


def _expected(arrs, segs, step, gscale=1.0, zero_grad=1):
    """The restatement inside every segment, the input bits everywhere else."""
    p, g, m, v = (a.copy() for a in arrs)
    with np.errstate(all="ignore"):
        for o, n, lr in segs:
            sl = slice(o, o + n)
            p[sl], m[sl], v[sl] = adam_reference(arrs[0][sl], arrs[1][sl], arrs[2][sl], arrs[3][sl], lr, B1, B2, EPS, step, gscale)
            if zero_grad:
                g[sl] = 0.0
    return [p, g, m, v]


def _same_bits(got, want):
    """Bit for bit; a NaN must sit where a NaN is expected (its payload is not compared)."""
    for name, a, b in zip(("param", "grad", "exp_avg", "exp_avg_sq"), got, want):
        nan = np.isnan(b)
        assert np.array_equal(np.isnan(a), nan), name
        bad = np.flatnonzero((a.view(np.int32) != b.view(np.int32)) & ~nan)
        assert bad.size == 0, (name, bad[:8], a[bad[:8]], b[bad[:8]])


def _lrs(n):
    return [1.6e-4 * 1.37 ** i for i in range(n)]


# ---- 1. alignment matrix --------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("residue", [0, 1, 2, 3])
def test_alignment_matrix(residue):
    """offset mod 4 x count: head longer than the count, no vector body, one and two workgroups plus head and tail.  The 13 counts of
    one residue are the segments of one launch (the empty one included), each behind a guard gap."""
    where, n = _lay([(residue, c) for c in COUNTS])
    assert all(o % 4 == residue for o, _ in where)
    segs = [(o, c, lr) for (o, c), lr in zip(where, _lrs(len(where)))]
    arrs = _arrays(n, 100 + residue)
    tens = _dev(arrs)
    assert _step(tens, segs, 7, 0.5) == 0
    _same_bits(_host(tens), _expected(arrs, segs, 7, 0.5))


@pytest.mark.gpu
@pytest.mark.parametrize("residue", [0, 1, 2, 3])
@pytest.mark.parametrize("count", [1, 2, 3, 5, 4097])
def test_alignment_single_segment(residue, count):
    """The same cells alone in a launch (block_start has one entry; the shard of a rank is often one clipped segment)."""
    where, n = _lay([(residue, count)])
    segs = [(where[0][0], count, 2.5e-3)]
    arrs = _arrays(n, 7 * count + residue)
    tens = _dev(arrs)
    assert _step(tens, segs, 7) == 0
    _same_bits(_host(tens), _expected(arrs, segs, 7))


# ---- 2. segment table -----------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_sixteen_segments_with_empty_ones_and_table_limits():
    counts = [0, 37, 4100, 1, 0, 0, 513, 4, 6, 0, 2051, 3, 9, 130, 8, 0]          # empty: first, in the middle (twice in a row), last
    where, n = _lay([((3 * i) % 4, c) for i, c in enumerate(counts)])
    segs = [(o, c, lr) for (o, c), lr in zip(where, _lrs(16))]
    assert len(segs) == 16 and len({s[2] for s in segs}) == 16
    arrs = _arrays(n, 21)
    tens = _dev(arrs)
    assert _step(tens, segs, 3) == 0
    _same_bits(_host(tens), _expected(arrs, segs, 3))
    # refused tables change nothing: 17 segments, none, a negative offset or count
    tens = _dev(arrs)
    assert _step(tens, segs + [(n - GUARD, 2, 1e-3)], 3) == ERR
    assert _step(tens, segs, 3, nseg=0) == ERR
    assert _step(tens, [(GUARD, 5, 1e-3), (-4, 5, 1e-3)], 3) == ERR
    assert _step(tens, [(GUARD, 5, 1e-3), (40, -1, 1e-3)], 3) == ERR
    words = torch.zeros(3, dtype=torch.int64, device=DEV)
    assert _step_device(tens, segs + [(n - GUARD, 2, 1e-3)], words, 0) == ERR
    assert _step_device(tens, [(-4, 5, 1e-3)], words, 0) == ERR
    _same_bits(_host(tens), arrs)
    assert not words.any()


# ---- 3. zero_grad and grad_scale ------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("zero_grad", [0, 1])
@pytest.mark.parametrize("gscale", [1.0, 0.5, 1.0 / 3.0, 0.125])
def test_zero_grad_and_grad_scale(zero_grad, gscale):
    where, n = _lay([(1, 4099), (2, 6), (0, 1030), (3, 2)])
    segs = [(o, c, lr) for (o, c), lr in zip(where, _lrs(4))]
    arrs = _arrays(n, 31)
    tens = _dev(arrs)
    assert _step(tens, segs, 7, gscale, zero_grad) == 0
    got = _host(tens)
    _same_bits(got, _expected(arrs, segs, 7, gscale, zero_grad))
    if not zero_grad:
        assert np.array_equal(got[1].view(np.int32), arrs[1].view(np.int32))


# ---- 4. values ------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_special_values():
    """Zero, -0.0, a gradient whose square underflows next to a denormal second moment (the restatement keeps denormals: a device
    that flushed them would differ), a gradient whose square overflows, and NaN gradients in the middle of a float4 and in the
    scalar tail, which must stay in their own element."""
    cnt = 4 * 300 + 3
    where, n = _lay([(0, cnt)])
    o = where[0][0]
    arrs = _arrays(n, 41)
    p, g, m, v = arrs
    z = slice(o + 16, o + 32)                 # g = 0, zero moments: 0 / eps
    g[z], m[z], v[z] = 0.0, 0.0, 0.0
    nz = slice(o + 32, o + 48)
    g[nz], m[nz], v[nz] = -0.0, 0.0, 0.0
    tiny = slice(o + 48, o + 80)              # g^2 underflows; v is a denormal
    g[tiny], v[tiny] = 1e-30, np.float32(1e-40)
    m[o + 48:o + 64] = 0.0
    huge = slice(o + 80, o + 96)              # g^2 = inf
    g[huge] = 1e20
    g[o + 80 + 5] = -1e20
    nan_vec, nan_tail = o + 4 * 50 + 1, o + cnt - 2
    g[nan_vec] = g[nan_tail] = np.nan
    assert nan_tail >= o + 4 * 300 and 0 < float(v[o + 48]) < 2.0 ** -126
    segs = [(o, cnt, 1e-3)]
    tens = _dev(arrs)
    assert _step(tens, segs, 2) == 0
    got = _host(tens)
    want = _expected(arrs, segs, 2)
    assert 0 < float(want[3][o + 48]) < 2.0 ** -126 and np.isinf(want[3][huge]).all()           # the restatement kept / made them
    _same_bits(got, want)
    assert np.array_equal(got[0][z].view(np.int32), p[z].view(np.int32)) and np.array_equal(got[0][nz].view(np.int32), p[nz].view(np.int32))
    assert np.array_equal(got[0][huge].view(np.int32), p[huge].view(np.int32))                   # m / inf = 0
    for a in (got[0], got[2], got[3]):
        assert sorted(np.flatnonzero(np.isnan(a))) == [nan_vec, nan_tail]
    assert not np.isnan(got[1]).any()


# ---- 5. many steps --------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_fifty_steps_over_the_field_layout():
    from segs_slam_amd.gaussian_trainer import OptimizationParams, expon_lr, field_segments
    P, opt = 777, OptimizationParams()
    rng = np.random.default_rng(51)
    lrs = {"scales": opt.scaling_lr, "rotations": opt.rotation_lr, "opacity": opt.opacity_lr, "colors": opt.feature_lr}
    n = 14 * P
    arrs = _arrays(n + 2 * GUARD, 52)
    arrs[2][GUARD:GUARD + n], arrs[3][GUARD:GUARD + n] = 0.0, 0.0      # fresh moments inside; the guards keep their values
    tens = _dev(arrs)
    for step in range(1, 51):
        lrs["means3D"] = expon_lr(step, opt.position_lr_init, opt.position_lr_final, opt.position_lr_max_steps)
        segs = [(GUARD + o, c, lr) for o, c, lr in field_segments(lrs, P)]
        arrs[1] = (rng.standard_normal(n + 2 * GUARD) * 1e-3).astype(np.float32)
        tens[1].copy_(torch.from_numpy(arrs[1]))
        assert _step(tens, segs, step) == 0
        arrs = _expected(arrs, segs, step)
        _same_bits(_host(tens), arrs)
    assert segs[0][2] < opt.position_lr_init and segs[-1][0] + segs[-1][1] == GUARD + n


# ---- 6. device step count -------------------------------------------------------------------------------------------------

def _device_layout():
    where, n = _lay([(2, 4101), (1, 3), (0, 1029)])
    return [(o, c, lr) for (o, c), lr in zip(where, _lrs(3))], n


@pytest.mark.gpu
def test_device_count_equals_host_count():
    """t = 1 ... 12 from a zeroed word pair, then counts preset into the pair: the bias corrections formed on the device (double
    pow, one lane per workgroup) give the bits of the host-count form and of the restatement."""
    segs, n = _device_layout()
    rng = np.random.default_rng(61)
    arrs = _arrays(n, 62)
    host, devc = _dev(arrs), _dev(arrs)
    words = torch.zeros(3, dtype=torch.int64, device=DEV)
    for t in range(1, 13):
        arrs[1] = (rng.standard_normal(n) * 1e-3).astype(np.float32)
        for tens in (host, devc):
            tens[1].copy_(torch.from_numpy(arrs[1]))
        assert _step(host, segs, t) == 0 and _step_device(devc, segs, words, t - 1) == 0
        arrs = _expected(arrs, segs, t)
        got = _host(devc)
        _same_bits(got, _host(host))
        _same_bits(got, arrs)
        assert int(words[t & 1]) == t
    for preset in (99, 999, 29_999):
        arrs = _arrays(n, preset)
        host, devc = _dev(arrs), _dev(arrs)
        words = torch.tensor([preset, -5, 0], dtype=torch.int64, device=DEV)
        assert _step(host, segs, preset + 1) == 0 and _step_device(devc, segs, words, 0) == 0
        got = _host(devc)
        _same_bits(got, _host(host))
        _same_bits(got, _expected(arrs, segs, preset + 1))
        assert words.tolist() == [preset, preset + 1, 0]


@pytest.mark.gpu
def test_skipped_calls_do_not_count():
    """Guard words 0,1,1,0,1,0: three steps taken, at t = 1, 2, 3; a skipped call leaves parameters and moments alone and clears the
    gradients of its segments (only those)."""
    from segs_slam_amd.gaussian_trainer import DeviceStepCount
    segs, n = _device_layout()
    rng = np.random.default_rng(63)
    arrs = _arrays(n, 64)
    tens = _dev(arrs)
    count = DeviceStepCount(DEV)
    taken = 0
    for flag in (0, 1, 1, 0, 1, 0):
        arrs[1] = (rng.standard_normal(n) * 1e-3).astype(np.float32)
        tens[1].copy_(torch.from_numpy(arrs[1]))
        skip = torch.tensor([flag], dtype=torch.int32, device=DEV)
        assert _step_device(tens, segs, count.words, count.eager_call(), skip=skip) == 0
        if flag:
            for o, c, _ in segs:
                arrs[1][o:o + c] = 0.0
        else:
            taken += 1
            arrs = _expected(arrs, segs, taken)
        _same_bits(_host(tens), arrs)
        assert count.value() == taken and count.dropped() == count.calls - taken
    assert (count.value(), count.dropped(), count.calls) == (3, 3, 6)


@pytest.mark.gpu
def test_empty_shard_advances_the_count_unless_skipped():
    from segs_slam_amd.gaussian_trainer import DeviceStepCount
    arrs = _arrays(64, 65)
    tens = _dev(arrs)
    count = DeviceStepCount(DEV)
    want = 0
    for flag in (0, 1, 0, 0, 1):
        skip = torch.tensor([flag], dtype=torch.int32, device=DEV)
        assert _step_device(tens, [(0, 0, 0.0)], count.words, count.eager_call(), skip=skip) == 0
        want += 1 - flag
        assert count.value() == want
    assert (count.value(), count.dropped()) == (3, 2)
    _same_bits(_host(tens), arrs)
    assert _step(tens, [(0, 0, 0.0)], 1) == 0          # host-count form: nothing to do, no launch
    _same_bits(_host(tens), arrs)


# ---- 7. graph form, called eagerly ----------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_set_doubles():
    from segs_slam_amd import _capi
    lib = _capi.lib()
    vals = [0.1 + 1.0 / (3 + i) for i in range(17)]
    for k in (1, 9, 16):
        dst = torch.full((16 + 2 * GUARD,), -7.0, dtype=torch.float64, device=DEV)
        assert lib.segs_set_doubles(_ptr(dst[GUARD:]), (C.c_double * k)(*vals[:k]), k, _stream()) == 0
        torch.cuda.synchronize()
        assert dst[GUARD:GUARD + k].tolist() == vals[:k]
        assert (dst[:GUARD] == -7.0).all() and (dst[GUARD + k:] == -7.0).all()
    dst = torch.full((32,), -7.0, dtype=torch.float64, device=DEV)
    assert lib.segs_set_doubles(_ptr(dst), (C.c_double * 17)(*vals), 17, _stream()) == ERR
    assert lib.segs_set_doubles(_ptr(dst), (C.c_double * 17)(*vals), -1, _stream()) == ERR
    assert lib.segs_set_doubles(_ptr(dst), (C.c_double * 17)(*vals), 0, _stream()) == 0
    torch.cuda.synchronize()
    assert (dst == -7.0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("nseg", [1, 9, 16])
def test_graph_form_reads_the_device_learning_rates(nseg):
    """segs_adam_step_graph outside a capture: learning rates from the device table (segments[i].lr, set to a wrong value, is
    ignored), word [2] grows by one per call, skipped ones included, and alternating with segs_adam_step_device after
    sync_device_calls() keeps the bits of the host-count form."""
    from segs_slam_amd import _capi
    from segs_slam_amd.gaussian_trainer import DeviceStepCount
    where, n = _lay([((i + 1) % 4, c) for i, c in enumerate(([4099, 5, 0, 1027, 2, 9, 130, 3, 64, 1, 7, 8, 33, 4, 260, 6])[:nseg])])
    segs = [(o, c, lr) for (o, c), lr in zip(where, _lrs(nseg))]
    wrong = [(o, c, 123.0) for o, c, _ in segs]
    rng = np.random.default_rng(71 + nseg)
    arrs = _arrays(n, 72)
    tens = _dev(arrs)
    count = DeviceStepCount(DEV)
    table = torch.full((16,), 55.0, dtype=torch.float64, device=DEV)
    taken = 0
    #            form,    guard word
    plan = [("graph", 0), ("graph", 1), ("eager", 0), ("graph", 0), ("eager", 1), ("eager", 0), ("graph", 0), ("graph", 0)]
    for call, (form, flag) in enumerate(plan):
        arrs[1] = (rng.standard_normal(n) * 1e-3).astype(np.float32)
        tens[1].copy_(torch.from_numpy(arrs[1]))
        skip = torch.tensor([flag], dtype=torch.int32, device=DEV)
        lrs = [lr * (1.0 + 0.01 * call) for _, _, lr in segs]              # refreshed before every call, like a schedule
        now = [(o, c, lr) for (o, c, _), lr in zip(segs, lrs)]
        if form == "graph":
            assert _capi.lib().segs_set_doubles(_ptr(table), (C.c_double * nseg)(*lrs), nseg, _stream()) == 0
            count.sync_device_calls()
            assert int(count.words[2]) == call
            assert _step_graph(tens, wrong, table, count.words, skip=skip) == 0
            count.calls += 1
            assert int(count.words[2]) == call + 1
        else:
            assert _step_device(tens, now, count.words, count.eager_call(), skip=skip) == 0
        if flag:
            for o, c, _ in segs:
                arrs[1][o:o + c] = 0.0
        else:
            taken += 1
            arrs = _expected(arrs, now, taken)
        _same_bits(_host(tens), arrs)
        assert count.value() == taken
    assert (count.value(), count.dropped()) == (6, 2)
    assert _step_graph(tens, wrong, None, count.words) == ERR and _step_graph(tens, wrong, table, None) == ERR


# ---- 8. shards ------------------------------------------------------------------------------------------------------------

def _clip(segs, lo, hi):
    """keyframe_parallel.BucketExchange.clip_segments' arithmetic: a plain intersection."""
    out = []
    for off, cnt, lr in segs:
        a, b = max(off, lo), min(off + cnt, hi)
        if b > a:
            out.append((a, b - a, lr))
    return out


def _field_layout():
    from segs_slam_amd.gaussian_trainer import field_segments
    segs = field_segments(dict(zip(("means3D", "scales", "rotations", "opacity", "colors"), _lrs(5))), 777)
    return segs, 14 * 777


def _scaffold_layout():
    """The nine Adam groups of a Scaffold model of the shipped shape (feat_dim 32, 10 offsets, appearance 32, feature bank): the four
    per-anchor groups, laid out for a capacity above the live anchor count (so with gaps), and the five MLP groups by
    segs_neural_param_layout."""
    from segs_slam_amd.neural_gaussians import ModelDims, ScaffoldModel
    model = ScaffoldModel(41, ModelDims(), DEV, capacity=44)
    names = ("anchor", "offset", "anchor_feat", "scaling", "mlp_opacity", "mlp_cov", "mlp_color", "appearance", "mlp_featurebank")
    segs = model.adam_groups(dict(zip(names, _lrs(9))))
    assert len(segs) == 9 and segs[-1][0] + segs[-1][1] == model.n_params
    return segs, model.n_params


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["fields", "scaffold"])
@pytest.mark.parametrize("world", [2, 3, 8])
def test_shards_touch_only_their_range(layout, world):
    """Every rank's clipped launch leaves all four arrays outside its range alone, and the shards together give the bits of one
    full launch.  The shard length takes every residue modulo 4, so the cuts fall at every alignment."""
    base, n = _field_layout() if layout == "fields" else _scaffold_layout()
    base = [(GUARD + o, c, lr) for o, c, lr in base]
    arrs = _arrays(n + 2 * GUARD, 81 + world)
    full = _dev(arrs)
    words = torch.tensor([6, 0, 0], dtype=torch.int64, device=DEV)
    assert _step_device(full, base, words, 0, 1.0 / world) == 0
    want = _host(full)
    _same_bits(want, _expected(arrs, base, 7, 1.0 / world))
    per = -(-n // world)
    for residue in range(4):
        shard_len = per + (residue - per) % 4
        assert shard_len % 4 == residue
        union = [a.copy() for a in arrs]
        covered = np.zeros(n + 2 * GUARD, dtype=bool)
        for rank in range(world):
            lo = GUARD + min(rank * shard_len, n)
            hi = GUARD + min(rank * shard_len + shard_len, n)
            segs = _clip(base, lo, hi)
            tens = _dev(arrs)
            words = torch.tensor([6, 0, 0], dtype=torch.int64, device=DEV)
            assert _step_device(tens, segs or [(0, 0, 0.0)], words, 0, 1.0 / world) == 0
            got = _host(tens)
            assert int(words[1]) == 7
            for a, b, w, u in zip(got, arrs, want, union):
                assert np.array_equal(a[:lo].view(np.int32), b[:lo].view(np.int32))
                assert np.array_equal(a[hi:].view(np.int32), b[hi:].view(np.int32))
                assert np.array_equal(a[lo:hi].view(np.int32), w[lo:hi].view(np.int32))
                u[lo:hi] = a[lo:hi]
            covered[lo:hi] = True
        assert covered[GUARD:GUARD + n].all() and not covered[:GUARD].any() and not covered[GUARD + n:].any()
        _same_bits(union, want)
