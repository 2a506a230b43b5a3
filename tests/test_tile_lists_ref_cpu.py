"""The float64 reference of the resident tile lists (tests/_tile_lists_ref.py) has teeth -- checked without a GPU.

(a) its vectorised classification equals a per-pixel Python loop, and its rectangle minimum is attained and below a dense sampling;
(b) a float32 restatement of the project's own tight rectangle and quadrant test passes the checker on every scene the GPU tests
    use; (c) four mutations of that restatement each fail it on at least one of those scenes; (d) on every scene the UNDECIDED
quadrants -- where the reference's margin, not the arithmetic, decides -- are at most 2 % of the MUST quadrants: a condition on
the INPUTS, which keeps the margin from excusing a failure (a scene that exceeds it is to be changed, not the cap)."""
import math

import numpy as np
import pytest

from tests import _tile_lists_ref as T

WITH_PAIRS = [n for n in T.SCENES if n not in ("nothing_visible", "single_hidden")]


def emulated(name, ref=None, **mutation):
    sc, o, shared = T.oracle_case(name)
    ref = shared if ref is None else ref
    ranges, values = T.emulate_lists(sc, o, ref, **mutation)
    return T.compare_lists(ref, ranges, values, keep_dead=False, R=ref.R)


def test_vectorised_reference_equals_a_per_pixel_loop():
    from oracle import gs_oracle
    from segs_slam_amd import scenes
    sc = scenes.make_scene(60, 48, 40, 40.0, 40.0, seed=77)
    sc.scales *= 3.0
    sc.scales[:20] *= np.array([8.0, 0.2, 0.2], dtype=np.float32)
    sc.opacity[:10] = np.linspace(0.003, 0.006, 10, dtype=np.float32).reshape(-1, 1)      # around 1/255
    o, _ = gs_oracle.run_scene(sc, backward=False)
    ref = T.reference_of(o)
    assert ref.R >= 100 and 0 < ref.stats["must_quadrants"] < ref.stats["may_quadrants"] <= 4 * ref.R
    xy, co = o.get("means2D").astype(np.float64), o.get("conic_opacity").astype(np.float64)
    W, H, u = 48, 40, 2.0 ** -24
    for i in range(ref.R):
        g, t = int(ref.point_list[i]), int(ref.pair_tile[i])
        A, B, C, op = (float(v) for v in co[g])
        thr = math.log2(255.0 * op) if 255.0 * op > 1.0 else None
        must, und = [False] * 4, [False] * 4
        for y in range(16):
            for x in range(16):
                X, Y = (t % ref.gx) * 16 + x, (t // ref.gx) * 16 + y
                if X >= W or Y >= H or thr is None:
                    continue
                dx, dy = X - xy[g, 0], Y - xy[g, 1]
                q = T.LOG2E * (0.5 * (A * dx * dx + C * dy * dy) + B * dx * dy)
                tol = 8.0 * u * (T.LOG2E * (0.5 * (abs(A) * dx * dx + abs(C) * dy * dy) + abs(B * dx * dy)) + abs(thr)) + 1e-5
                qd = (y // 8) * 2 + x // 8
                if 0 <= q <= thr - tol:
                    must[qd] = True
                elif -tol <= q <= thr + tol:
                    und[qd] = True
        assert must == ref.must[i].tolist(), i
        assert [a and not b for a, b in zip(und, must)] == ref.undecided[i].tolist(), i
        # MAY: the minimum is attained inside the rectangle and no point of a dense sampling lies below it
        s = np.linspace(0.0, 7.0, 141)
        for qd in range(4):
            x_lo, y_lo = (t % ref.gx) * 16 + 8 * (qd & 1) - xy[g, 0], (t // ref.gx) * 16 + 8 * (qd >> 1) - xy[g, 1]
            one = lambda v: np.array([v])      # noqa: E731
            qmin, mx, my = (float(v[0]) for v in T.rect_min(one(A), one(B), one(C), one(x_lo), one(x_lo + 7), one(y_lo), one(y_lo + 7)))
            assert x_lo <= mx <= x_lo + 7 and y_lo <= my <= y_lo + 7
            at = T.LOG2E * (0.5 * (A * mx * mx + C * my * my) + B * mx * my)
            assert abs(at - qmin) <= 1e-12 * (1.0 + float(T.term_magnitude(A, B, C, mx, my)))
            dx, dy = (x_lo + s)[None, :], (y_lo + s)[:, None]
            sampled = float((T.LOG2E * (0.5 * (A * dx * dx + C * dy * dy) + B * dx * dy)).min())
            assert qmin <= sampled + 1e-9 * (1.0 + abs(sampled))
            if thr is None:
                assert not ref.may[i, qd]
            else:
                tol = 8.0 * u * (float(T.term_magnitude(A, B, C, mx, my)) + abs(thr)) + 1e-5
                assert bool(ref.may[i, qd]) == (qmin <= thr * 1.0001 + 1e-3 + tol)


@pytest.mark.parametrize("name", list(T.SCENES))
def test_restated_emitter_passes_and_undecided_quadrants_stay_under_the_cap(name):
    sc, o, ref = T.oracle_case(name)
    print(name, ref.stats)
    assert ref.stats["undecided_quadrants"] <= 0.02 * ref.stats["must_quadrants"], ref.stats
    if name in WITH_PAIRS:
        assert ref.stats["must_quadrants"] > 0
    else:
        assert ref.R == 0 and o.R == 0
    stats, fails = emulated(name)
    assert not fails, (fails, stats)
    assert stats["listed"] <= ref.stats["may_pairs"] <= ref.R


def test_the_scenes_hold_what_they_are_for():
    sc, o, ref = T.oracle_case("huge")
    per_gaussian = np.bincount(ref.point_list[ref.may.any(1)], minlength=sc.P)
    assert (per_gaussian > 512).sum() >= 2 and (per_gaussian > 200).sum() >= 12      # owners of more than one 512-slot emitter sub-batch; many that straddle two
    sc, o, ref = T.oracle_case("streaks_faint")
    faint, below = np.arange(sc.P // 4), np.arange(sc.P - 40, sc.P)
    assert np.all(sc.opacity[faint] * 255 > 1) and np.all(sc.opacity[below] * 255 <= 1)
    binned = o.get("radii") > 0
    assert binned[below].sum() >= 20 and not np.isin(ref.point_list[ref.may.any(1)], below).any()      # below 1/255: binned by the oracle, no MAY pair
    has_must, has_may = (np.isin(faint, ref.point_list[m.any(1)]) for m in (ref.must, ref.may))
    assert has_must.sum() >= 50 and (binned[faint] & ~has_may).sum() >= 10      # just above 1/255: some contribute, some reach no quadrant at all
    sc, o, ref = T.oracle_case("ties")
    d = o.get("depths").view(np.uint32)
    assert np.array_equal(d[200:], d[:100]) and (o.get("radii")[200:] > 0).sum() >= 30
    sc, o, ref = T.oracle_case("generic")
    assert (ref.gx, ref.gy) == (25, 21) and sc.camera.width % 16 == 12 and sc.camera.height % 16 == 10
    edge = (ref.pair_tile % ref.gx == ref.gx - 1) | (ref.pair_tile // ref.gx == ref.gy - 1)
    assert (ref.must[edge].any(1)).sum() > 100      # the cut tiles hold MUST pairs


MUTATIONS = {
    "qx and qy swapped": dict(swap=True),
    "quadrant span 8 instead of 7 on the high side": dict(high_span=8.0),
    "all masks 0xF": dict(all_bits=True),
}


@pytest.mark.parametrize("what", list(MUTATIONS))
def test_mutations_of_the_restated_emitter_fail(what):
    failed = {}
    for name in WITH_PAIRS:
        stats, fails = emulated(name, **MUTATIONS[what])
        if fails:
            failed[name] = fails
    print(what, "fails on", failed)
    assert failed, what


def test_emitter_without_inflation_fails_a_reference_without_margin():
    """The inflation removed AND tol set to 0: float32 rounding alone then drops a quadrant that float64 says contributes."""
    failed = {}
    for name in ("streaks_faint", "generic", "huge", "ties", "two_pass", "single"):
        sc, o, _ = T.oracle_case(name)
        bare = T.reference_of(o, tol_factor=0.0, tol_abs=0.0)
        stats, fails = emulated(name, ref=bare, inflate=False)
        if stats["must_bits_missing"] or stats["must_pairs_missing"]:
            failed[name] = (stats["must_pairs_missing"], stats["must_bits_missing"])
            break
    print("MUST (pairs, bits) missing without inflation and margin:", failed)
    assert failed


def test_checker_rejects_lists_broken_in_every_way_it_names():
    """Each clause of check_tight_lists on its own: the restated emitter's lists of the ties scene, broken one way at a time."""
    sc, o, ref = T.oracle_case("ties")
    ranges, values = T.emulate_lists(sc, o, ref)
    assert T.check_tight_lists(ref, ranges, values, keep_dead=False, R=ref.R)["listed"] == values.shape[0]

    def broken(r, v, keep_dead=False, R=None):
        return T.compare_lists(ref, r, v, keep_dead, ref.R if R is None else R)[1]

    long_tile = int(np.argmax(ranges[:, 1] - ranges[:, 0]))
    s, e = (int(x) for x in ranges[long_tile])
    assert e - s >= 3
    # order: two neighbours of one list exchanged; the duplicated Gaussians (equal depth bits) exchanged
    v = values.copy(); v[[s, s + 1]] = v[[s + 1, s]]
    assert any("subsequence" in f for f in broken(ranges, v))
    ids = (values & T.ID_MASK).astype(np.int64)
    tile_of = np.repeat(np.arange(ranges.shape[0]), ranges[:, 1] - ranges[:, 0])
    twins = [(i, j) for i in range(values.shape[0] - 1) for j in (i + 1,) if tile_of[i] == tile_of[j] and ids[j] == ids[i] + 200]
    assert twins                                      # a duplicate directly behind its original: only the index orders them
    v = values.copy(); v[list(twins[0])] = v[list(twins[0])[::-1]]
    assert any("subsequence" in f for f in broken(ranges, v))
    # a listed instance twice; an instance of another tile; a Gaussian the oracle does not list there
    v = values.copy(); v[s + 1] = v[s]
    assert broken(ranges, v)
    v = values.copy(); v[s] = (v[s] & ~np.uint32(T.ID_MASK)) | np.uint32(sc.P - 1 if ids[s] != sc.P - 1 else 0)
    assert broken(ranges, v)
    # a MUST pair dropped (the ranges closed up behind it); a MUST bit cleared; an empty mask listed
    pair_must = ref.must[np.flatnonzero(ref.pair_tile == long_tile)]
    listed_pos = np.flatnonzero(np.isin(ref.point_list[ref.pair_tile == long_tile], ids[s:e]))
    k = int(np.flatnonzero(pair_must[listed_pos].any(1))[0])
    r = ranges.copy(); r[long_tile, 1] -= 1; r[long_tile + 1:][r[long_tile + 1:, 1] > 0] -= 1
    assert any("MUST pairs are not listed" in f for f in broken(r, np.delete(values, s + k), R=ref.R))
    bit = int(np.flatnonzero(pair_must[listed_pos][k])[0])
    v = values.copy(); v[s + k] &= ~np.uint32(1 << (T.ID_BITS + bit))
    assert any("MUST quadrant bits are clear" in f for f in broken(ranges, v))
    v = values.copy(); v[s + k] &= np.uint32(T.ID_MASK)
    assert any("empty mask" in f for f in broken(ranges, v))
    assert not any("empty mask" in f for f in broken(ranges, v, keep_dead=True))
    # a bit outside MAY
    outside = np.flatnonzero(~ref.may.all(1) & ref.may.any(1))
    pos = {(int(t), int(g)): i for i, (t, g) in enumerate(zip(tile_of, ids))}
    i = next(pos[(int(ref.pair_tile[p]), int(ref.point_list[p]))] for p in outside if (int(ref.pair_tile[p]), int(ref.point_list[p])) in pos)
    v = values.copy(); v[i] |= np.uint32(0xF << T.ID_BITS)
    assert any("outside MAY" in f for f in broken(ranges, v))
    # the tight lists are not the oracle's; an empty tile that does not read {0, 0}; ranges that do not partition; the counts
    assert any("not the oracle's" in f for f in broken(ranges, values, keep_dead=True))
    empty = int(np.flatnonzero(ranges[:, 1] == 0)[0])
    r = ranges.copy(); r[empty] = (7, 7)
    assert any("{0, 0}" in f for f in broken(r, values))
    r = ranges.copy(); r[long_tile, 0] += 1
    assert any("partition" in f for f in broken(r, values))
    assert any("partition" in f for f in broken(ranges, values[:-1]))
    assert any("does not hold" in f for f in broken(ranges, values, R=values.shape[0] - 1))
    assert any("does not hold" in f for f in broken(ranges, values, R=ref.R + 1))
