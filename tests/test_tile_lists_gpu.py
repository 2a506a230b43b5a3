"""The device's resident tile lists and quadrant masks against the float64 reference of tests/_tile_lists_ref.py.

The training path never walks the reference's instance lists: the resident forward, and the reference-shaped entry under
SEGS_RASTER_TIGHT_BINNING, bin a shrunken rectangle, give every instance a 4-bit quadrant mask and drop the instances whose mask
is empty.  Image equality with the synchronising path bounds those lists from below only, and the
synchronising path shares the emitter.  Here every scene's lists are held, per (Gaussian, tile, quadrant), between MUST (float64
says a pixel of the quadrant contributes, outside a margin that scales with the magnitude of the cancelling terms) and MAY (the
emitter's own inflated test in float64 plus that margin), and to the oracle's order exactly.

Scenes (tests/_tile_lists_ref.py; all 396x330 = 25x21 tiles with a cut right and bottom edge unless stated): generic (3000
Gaussians), huge (40 at 40x scale: owners of more than one emitter sub-batch), streaks + faint (1000: half thin streaks, a quarter
with an opacity just above 1/255, forty below it), ties (100 exact duplicates: the index decides), two-pass (752x720 = 2115 tiles:
the tile-id sort takes two 8-bit passes and the last one fills the range table; every other scene is sorted by one 11-bit pass
and the range kernel), nothing visible, and P = 1 hidden and visible.
Forms: (i) the resident engine, (ii) with keep_dead_instances (lists equal the oracle's), (iii) after set_active(0.8 P) against an
oracle run on the first rows, (iv) the reference-shaped entry under segs_raster_set_flags(32), whose binning and image buffers
serve the same two debug calls (its live count is the end of the last non-empty range: the entry returns only the emitted count).
The two-pass, nothing-visible and P = 1 scenes go through (i) only.

profiles/r10_tile_list_reference.txt records the figures (python -m tests.test_tile_lists_gpu record FILE writes them)."""
import ctypes as C
import functools
import sys

import numpy as np
import pytest
import torch

from tests import _tile_lists_ref as T
from tests.test_backward_written_rows_gpu import DEV, _t
from tests.test_render_fwd_lane_mask_gpu import resident_forward

pytestmark = pytest.mark.gpu

FORMS = ("resident", "keep_dead", "active_rows", "tight_flag")


def higher_msb(n):
    """getHigherMsb (csrc/capi.hip)."""
    msb = step = 16
    while step > 1:
        step //= 2
        msb = msb + step if n >> msb else msb - step
    return msb + 1 if n >> msb else msb


def tile_sort_passes(tiles, capacity):
    """The pass-count rule of run_binning (csrc/capi.hip): one 11-bit pass when the tile ids have at most 11 bits and the
    instance capacity fits SORT_WIDE_MAX_TILES = 1024 sort tiles of 2048 keys, 8-bit passes otherwise.  It keys on the tile count
    (and the capacity), not on R: 2115 tiles have 12 bits at any P."""
    bit = higher_msb(tiles)
    digit = 11 if bit <= 11 and (capacity + 2047) // 2048 <= 1024 else 8
    return (bit + digit - 1) // digit


def tight_flag_forward(sc):
    """Lists of the reference-shaped forward under SEGS_RASTER_TIGHT_BINNING, read with the two debug calls."""
    from segs_slam_amd import _capi, rasterize_points as rp
    cam = sc.camera
    lib = _capi.lib()
    e = torch.empty(0, device=DEV)
    old = lib.segs_raster_set_flags(32)
    try:
        R, color, radii, geom, binning, img = rp.RasterizeGaussiansCUDA(
            _t(sc.bg), _t(sc.means3D), _t(sc.colors), _t(sc.opacity), _t(sc.scales), _t(sc.rotations), 1.0, e, _t(cam.world_view_transform),
            _t(cam.full_proj_transform), cam.tanfovx, cam.tanfovy, cam.height, cam.width, e, 0, _t(cam.camera_center), False)
    finally:
        assert lib.segs_raster_set_flags(old) == 32
    tiles = ((cam.width + 15) // 16) * ((cam.height + 15) // 16)
    ranges = torch.zeros((tiles, 2), dtype=torch.int32, device=DEV)
    vals = torch.zeros(max(R, 1), dtype=torch.int32, device=DEV)
    st = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    _capi.check(lib.segs_debug_unpack_image(p(img), cam.width, cam.height, p(ranges), None, None, st), "unpack_image")
    _capi.check(lib.segs_debug_instance_values(p(binning), R, p(vals), st), "instance_values")
    torch.cuda.synchronize()
    ranges = ranges.cpu().numpy().astype(np.int64)
    live = int(ranges[:, 1].max())
    assert live <= R
    return dict(out_color=color.cpu().numpy(), ranges=ranges, values=vals.cpu().numpy().view(np.uint32)[:live],
                counts=np.array([R, live, 0, R], dtype=np.int64))


@functools.lru_cache(maxsize=None)
def measure(name, form):
    """(reference, device outputs, statistics, failures) of one scene in one form: computed once, shared, never changed."""
    sc, o, ref = T.oracle_case(name)
    if form == "resident":
        g = resident_forward(sc)
    elif form == "keep_dead":
        g = resident_forward(sc, keep_dead_instances=True)
    elif form == "active_rows":
        n = int(0.8 * sc.P)
        g = resident_forward(sc, active=n)
        _, o, ref = T.oracle_case(name, rows=n)
    else:
        g = tight_flag_forward(sc)
    stats, fails = T.compare_lists(ref, g["ranges"], g["values"], keep_dead=(form == "keep_dead"), R=int(g["counts"][0]))
    if int(g["counts"][1]) != g["values"].shape[0]:
        fails.append(f"R_live {int(g['counts'][1])} is not the number of values {g['values'].shape[0]}")
    return ref, g, stats, fails


def line(name, form, ref, g, stats):
    return (f"{name:16s} {form:12s} oracle_pairs {stats['oracle_pairs']:7d}  must_pairs {stats['must_pairs']:6d}  must_quadrants {stats['must_quadrants']:6d}  "
            f"may_pairs {stats['may_pairs']:6d}  emitted {int(g['counts'][0]):7d}  listed {stats['listed']:6d}  undecided_quadrants {stats['undecided_quadrants']:4d}  "
            f"device_must_pairs_missing {stats['must_pairs_missing']}  device_must_bits_missing {stats['must_bits_missing']}  "
            f"device_bits_outside_may {stats['bits_outside_may']}  float64_pass_s {ref.seconds:.2f}")


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", T.ALL_FORMS)
def test_device_lists_lie_between_must_and_may_in_the_oracles_order(name, form):
    ref, g, stats, fails = measure(name, form)
    print(line(name, form, ref, g, stats))
    assert not fails, (fails, stats)
    sc = T.oracle_case(name)[0]
    cam = sc.camera
    assert tile_sort_passes(ref.gx * ref.gy, int(g["counts"][3])) == 1      # (the two-pass regime has its own scene)
    if form == "keep_dead":
        assert stats["listed"] == ref.R == int(g["counts"][0])
    else:
        assert stats["must_pairs"] <= stats["listed"] <= stats["may_pairs"] < ref.R      # shorter than the reference's, per pair no longer than MAY
    assert cam.width == ref.W and cam.height == ref.H


def test_two_pass_tile_sort_gives_the_same_specified_lists():
    ref, g, stats, fails = measure("two_pass", "resident")
    print(line("two_pass", "resident", ref, g, stats))
    assert ref.gx * ref.gy == 2115 and tile_sort_passes(2115, int(g["counts"][3])) == 2      # 12 bits of tile id: two 8-bit passes
    assert not fails, (fails, stats)
    assert stats["must_pairs"] <= stats["listed"] <= stats["may_pairs"] < ref.R


def test_single_visible_gaussian():
    ref, g, stats, fails = measure("single", "resident")
    print(line("single", "resident", ref, g, stats))
    assert not fails, (fails, stats)
    assert 0 < stats["must_pairs"] <= stats["listed"] <= stats["may_pairs"]


@pytest.mark.parametrize("name", ["nothing_visible", "single_hidden"])
def test_nothing_visible_gives_empty_lists_and_the_background(name):
    ref, g, stats, fails = measure(name, "resident")
    print(line(name, "resident", ref, g, stats))
    assert not fails, (fails, stats)
    assert ref.R == 0 and g["values"].shape[0] == 0 and not g["ranges"].any() and int(g["counts"][0]) == 0
    sc = T.oracle_case(name)[0]
    assert np.array_equal(g["out_color"], np.broadcast_to(sc.bg.reshape(3, 1, 1), g["out_color"].shape))
    assert not g["n_contrib"].any() and np.all(g["final_T"] == 1.0)


def record(path):
    rows = [(n, f) for n in T.ALL_FORMS for f in FORMS] + [(n, "resident") for n in T.SCENES if n not in T.ALL_FORMS]
    bad = 0
    with open(path, "w") as out:
        for name, form in rows:
            ref, g, stats, fails = measure(name, form)
            text = line(name, form, ref, g, stats) + (f"  FAILS {fails}" if fails else "")
            bad += bool(fails)
            print(text)
            out.write(text + "\n")
            out.flush()
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(record(sys.argv[2]) if sys.argv[1] == "record" else 2)
