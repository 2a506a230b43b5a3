"""The tile forward retires pixels by lane mask (csrc/render.hip, render_fwd_body): a pixel takes a list entry only while it is
inside the image, not yet saturated (`live`) and reached by the Gaussian; a saturating pixel leaves the mask with T, the sums and
`last` as they stood before that Gaussian, and takes nothing of it.  One test of the mask per group of four entries ends a wave's
walk.

What is compared.  The parent commit's library cannot be built from a checkout of this one, so the committed test takes the second
route: one RESIDENT forward per scene against the CPU oracle -- n_contrib exactly (as Gaussian ids: the resident lists are the
oracle's without the dead instances, so positions differ while the Gaussian at the position does not), final_T and the image at
the tolerance of tests/test_raster_gpu.py (1e-4 relative + 2e-6, off the pixels the oracle reports within 1e-5 of a threshold).
The depth form is held to the plain form BIT FOR BIT on everything they share (same arithmetic, one more sum), out_alpha to
1 - final_T exactly, and out_depth to the plain render of colours (z, z, z) on black at the bound of tests/test_depth_render_gpu.py
(1e-6 of the largest depth: the two are the same sums, but a colour passes through the projection kernel's clamp and the two
template instantiations need not contract alike).  The forward has no atomics, so none of this has run-to-run noise.

The bit-for-bit comparison against another build of the library (the parent's) is this module run as a script, once per library:
    SEGS_RASTER_LIB=/path/to/libsegs_raster.so python -m tests.test_render_fwd_lane_mask_gpu dump a.npz
    python -m tests.test_render_fwd_lane_mask_gpu dump b.npz && python -m tests.test_render_fwd_lane_mask_gpu compare a.npz b.npz
over the same scenes, both forms; profiles/r08_render_fwd_lane_mask.txt records its result for the parent of this change.

Scenes (the smallest at which the walk can go wrong; at most 2 000 Gaussians): 64x64 with 1 000 and 2 000 Gaussians and the
quadrant scene; 40x24 and 17x17, whose right and bottom edges cut a tile and a quadrant, so lanes outside the image exist; the
layered scene, whose 0.99 front layer saturates whole quadrants inside their first group -- asserted below to stop pixels at all
four positions of a group; a scene in which nothing saturates (opacity <= 0.05); and one quadrant whose list is 1, 3, 4, 5, 63, 64
and 65 entries long (group and chunk edges)."""
import functools
import sys

import numpy as np
import pytest
import torch

from tests.test_backward_packed_rows_gpu import generic_scene, quadrant_scene
from tests.test_backward_written_rows_gpu import DEV, FOCAL, _t, layered_scene
from tests.test_depth_render_gpu import close_to_max

pytestmark = pytest.mark.gpu

ID_MASK = (1 << 28) - 1      # csrc/gs_layout.h: Gaussian index | reachable quadrants << 28
LIST_LENGTHS = (1, 3, 4, 5, 63, 64, 65)


# ---------------------------------------------------------------------------------------------------------------- scenes
def faint_scene():
    """Nothing saturates: 1 500 Gaussians of opacity 0.01-0.05 (the deepest pile of a pixel would need 180 of them at 0.05)."""
    sc = generic_scene(1500, 64, 64, seed=5)
    sc.opacity[:] = (0.01 + 0.04 * np.random.default_rng(5).random((sc.P, 1))).astype(np.float32)
    return sc


def stacked_scene(n):
    """n faint Gaussians (opacity 0.02-0.05, sigma below half a pixel) on the centre of the top left 8x8 quadrant of a 32x32
    image, each deeper than the one before: that quadrant's list is n entries long, every other list is empty."""
    sc = generic_scene(n, 32, 32, seed=100 + n)
    cam = sc.camera
    rng = np.random.default_rng(100 + n)
    for i in range(n):
        z = np.float32(2.0 + 0.02 * i)
        sc.means3D[i] = ((2 * 3.5 + 1) / 32 - 1) * z * cam.tanfovx, ((2 * 3.5 + 1) / 32 - 1) * z * cam.tanfovy, z
        sc.scales[i] = (0.3 + 0.15 * rng.random(3)) * z / FOCAL
        sc.opacity[i] = 0.02 + 0.03 * rng.random()
    return sc


SCENES = {
    "generic_1000": lambda: generic_scene(1000, 64, 64, seed=11),
    "generic_2000": lambda: generic_scene(2000, 64, 64, seed=12),
    "quadrant": lambda: quadrant_scene("vfvvdb" * 150 + "f" * 100),
    "edge_40x24": lambda: generic_scene(600, 40, 24, seed=13),
    "edge_17x17": lambda: generic_scene(300, 17, 17, seed=14),
    "layered": lambda: layered_scene(2000),
    "faint": faint_scene,
    **{f"stacked_{n}": functools.partial(stacked_scene, n) for n in LIST_LENGTHS},
}


# ---------------------------------------------------------------------------------------------------------------- engine
def resident_forward(sc, render_depth=False, colors=None, bg=None, keep_dead_instances=False, active=None):
    """Outputs of one resident forward (the second forward of a fresh engine; the first one calibrates through the synchronising
    path): image, final_T, n_contrib, the tile ranges and instance values the kernel walked, and the depth form's two maps.
    keep_dead_instances: the engine's switch; active: rasterize only the first `active` rows (RasterEngine.set_active)."""
    import ctypes as C
    from segs_slam_amd import _capi
    from segs_slam_amd.raster_engine import RasterEngine
    cam = sc.camera
    eng = RasterEngine(sc.P, cam.width, cam.height, DEV, resident=True, render_depth=render_depth, keep_dead_instances=keep_dead_instances)
    if active is not None:
        eng.set_active(active)
    args = (_t(sc.bg if bg is None else bg), _t(sc.means3D), _t(sc.colors if colors is None else colors), _t(sc.opacity), _t(sc.scales),
            _t(sc.rotations), _t(cam.world_view_transform), _t(cam.full_proj_transform), _t(cam.camera_center), cam.tanfovx, cam.tanfovy)
    eng.forward(*args)
    eng.forward(*args)
    assert eng._last_resident and eng.check()
    lib = _capi.lib()
    tiles = ((cam.width + 15) // 16) * ((cam.height + 15) // 16)
    ranges = torch.zeros((tiles, 2), dtype=torch.int32, device=DEV)
    final_T = torch.zeros((cam.height, cam.width), dtype=torch.float32, device=DEV)
    n_contrib = torch.zeros((cam.height, cam.width), dtype=torch.int32, device=DEV)
    vals = torch.zeros(eng.capacity, dtype=torch.int32, device=DEV)
    st = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    _capi.check(lib.segs_debug_unpack_image(p(eng._img_r), cam.width, cam.height, p(ranges), p(final_T), p(n_contrib), st), "unpack_image")
    _capi.check(lib.segs_debug_instance_values(p(eng._bin_r), eng.capacity, p(vals), st), "instance_values")
    torch.cuda.synchronize()
    out = dict(out_color=eng.out_color.cpu().numpy(), final_T=final_T.cpu().numpy(), n_contrib=n_contrib.cpu().numpy().view(np.uint32),
               ranges=ranges.cpu().numpy().astype(np.int64), values=vals.cpu().numpy().view(np.uint32)[:eng.R_live],
               counts=np.array([eng.R, eng.R_live, eng.R_reference, eng.capacity], dtype=np.int64))      # emitted, live, calibrating call's, capacity
    if render_depth:
        out.update(out_depth=eng.out_depth.cpu().numpy(), out_alpha=eng.out_alpha.cpu().numpy())
    return out


@functools.lru_cache(maxsize=None)
def case(name):
    """Scene, the oracle's forward and the plain resident forward: computed once per scene and shared, never changed."""
    from oracle import gs_oracle
    sc = SCENES[name]()
    o, _ = gs_oracle.run_scene(sc, backward=False)
    return sc, o, resident_forward(sc)


def tile_view(a, tile, tiles_x):
    ty, tx = divmod(tile, tiles_x)
    return a[ty * 16:ty * 16 + 16, tx * 16:tx * 16 + 16]


def last_contributor_ids(n_contrib, ranges, ids, width):
    """Per pixel the Gaussian its n_contrib points at in its tile's list (-1: none)."""
    out = np.full(n_contrib.shape, -1, dtype=np.int64)
    tiles_x = (width + 15) // 16
    for tile, (s, _e) in enumerate(ranges):
        nc = tile_view(n_contrib, tile, tiles_x).astype(np.int64)
        view = tile_view(out, tile, tiles_x)
        hit = nc > 0
        view[hit] = ids[s + nc[hit] - 1]
    return out


def stop_positions(sc, o, g):
    """Where in a group of four each saturating pixel stops, from the oracle's per-Gaussian floats walked over the lists as the
    kernel groups them: per tile 64 entries at a time, of which a wave sees those with its quadrant's bit, four at a time.
    Returns (count of saturated pixels per position 0..3, pixels that saturate, pixels inside the image)."""
    w, h = sc.camera.width, sc.camera.height
    xy, co = o.get("means2D").astype(np.float64), o.get("conic_opacity").astype(np.float64)
    tiles_x = (w + 15) // 16
    counts, stopped_px, total_px = np.zeros(4, dtype=np.int64), 0, 0
    for tile, (s, e) in enumerate(g["ranges"]):
        ty, tx = divmod(tile, tiles_x)
        for q in range(4):
            ys, xs = np.meshgrid(np.arange(8) + ty * 16 + (q >> 1) * 8, np.arange(8) + tx * 16 + (q & 1) * 8, indexing="ij")
            inside = (xs < w) & (ys < h)
            T, live = np.ones((8, 8)), inside.copy()
            total_px += int(inside.sum())
            for c0 in range(s, e, 64):
                chunk = g["values"][c0:min(c0 + 64, e)]
                mine = chunk[(chunk >> (28 + q)) & 1 == 1] & ID_MASK
                for k, i in enumerate(mine):
                    dx, dy = xy[i, 0] - xs, xy[i, 1] - ys
                    power = -0.5 * (co[i, 0] * dx * dx + co[i, 2] * dy * dy) - co[i, 1] * dx * dy
                    alpha = np.minimum(0.99, co[i, 3] * np.exp(power))
                    ok = live & (power <= 0) & (alpha >= 1.0 / 255.0)
                    stop = ok & (T * (1 - alpha) < 1e-4)
                    counts[k % 4] += int(stop.sum())
                    stopped_px += int(stop.sum())
                    live &= ~stop
                    T = np.where(ok & ~stop, T * (1 - alpha), T)
                if not live.any():
                    break
    return counts, stopped_px, total_px


# ---------------------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("name", list(SCENES))
def test_resident_forward_against_the_oracle(name):
    sc, o, g = case(name)
    w = sc.camera.width
    unstable = o.unstable_pixels(1e-5)
    assert unstable.mean() < 0.01
    ok = ~unstable
    want = last_contributor_ids(o.get("n_contrib"), o.get("ranges").astype(np.int64), o.get("point_list").astype(np.int64), w)
    got = last_contributor_ids(g["n_contrib"], g["ranges"], (g["values"] & ID_MASK).astype(np.int64), w)
    assert np.array_equal(got[ok], want[ok])
    for k in ("final_T", "out_color"):
        a, b = g[k], o.get(k)
        err = np.abs(a - b)[..., ok]
        assert np.all(err <= 1e-4 * np.abs(b)[..., ok] + 2e-6), (k, float(err.max()))


def test_layered_scene_stops_pixels_at_every_position_of_a_group():
    sc, o, g = case("layered")
    counts, stopped, total = stop_positions(sc, o, g)
    print("saturating pixels by position in the group of four:", counts.tolist(), "of", total, "pixels")
    assert np.all(counts >= 20), counts.tolist()      # far from the few pixels a last-bit difference of exp could move
    assert stopped >= 0.4 * total                     # the layer covers 57 % of the image
    # and the saturated pixels report the state before the Gaussian that saturated them: T well above the 1e-4 they would have fallen under
    sat = (g["final_T"] < 0.05) & (g["n_contrib"] > 0)
    assert sat.sum() >= 0.4 * total and float(g["final_T"][sat].min()) >= 1e-4


def test_faint_scene_has_no_saturating_pixel_and_stacked_lists_have_their_lengths():
    sc, o, g = case("faint")
    assert stop_positions(sc, o, g)[1] == 0 and float(g["final_T"].min()) > 1e-2
    for n in LIST_LENGTHS:
        sc, o, g = case(f"stacked_{n}")
        s, e = g["ranges"][0]
        first_quadrant = (g["values"][s:e] >> 28) & 1
        assert int(first_quadrant.sum()) == n, (n, int(first_quadrant.sum()))
        assert int(g["n_contrib"][3, 3]) == n and int(g["n_contrib"][16:, 16:].max()) == 0      # every entry contributes at the centre


@pytest.mark.parametrize("name", ["generic_1000", "edge_40x24", "edge_17x17", "layered", "faint", "stacked_5", "stacked_65"])
def test_depth_form_is_the_plain_form_plus_one_sum(name):
    sc, o, g = case(name)
    d = resident_forward(sc, render_depth=True)
    for k in ("out_color", "final_T", "n_contrib", "ranges", "values"):
        assert np.array_equal(d[k].view(np.uint32) if d[k].dtype == np.float32 else d[k],
                              g[k].view(np.uint32) if g[k].dtype == np.float32 else g[k]), k
    assert np.array_equal(d["out_alpha"].view(np.uint32), (np.float32(1.0) - d["final_T"]).astype(np.float32).view(np.uint32))
    z = np.repeat(o.get("depths").reshape(-1, 1), 3, axis=1).astype(np.float32)
    trick = resident_forward(sc, colors=z, bg=np.zeros(3, dtype=np.float32))
    assert np.array_equal(trick["n_contrib"], g["n_contrib"])
    diff = float(np.abs(d["out_depth"] - trick["out_color"][0]).max())
    print("out_depth against the colour trick: largest difference", diff, "of", float(trick["out_color"][0].max()))
    assert close_to_max(d["out_depth"], trick["out_color"][0])
    if name != "faint":
        assert float(d["out_depth"].max()) > 0 and float(d["out_alpha"].max()) > 0


# ------------------------------------------------------------------------------------------- two builds of the library
def dump(path):
    out = {}
    for name in SCENES:
        sc = SCENES[name]()
        for depth in (False, True):
            for k, v in resident_forward(sc, render_depth=depth).items():
                out[f"{name}/{'depth' if depth else 'plain'}/{k}"] = v
    np.savez(path, **out)
    print("wrote", len(out), "arrays to", path)


def compare(path_a, path_b):
    a, b = np.load(path_a), np.load(path_b)
    assert sorted(a.files) == sorted(b.files)
    bad = [k for k in a.files if a[k].shape != b[k].shape or not np.array_equal(a[k].view(np.uint32) if a[k].dtype == np.float32 else a[k],
                                                                                 b[k].view(np.uint32) if b[k].dtype == np.float32 else b[k])]
    print(len(a.files), "arrays compared bit for bit;", "all equal" if not bad else f"DIFFERENT: {bad}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(dump(sys.argv[2]) if sys.argv[1] == "dump" else compare(sys.argv[2], sys.argv[3]))
