"""The "row written" bytes in the geometry scratch (csrc/gs_layout.h): the new region is aligned like the others, overlaps none
of them, is large enough for the whole-dword clears of the per-Gaussian backward, and the size entry point covers it."""
import ctypes as C
import os
import re

import pytest

from segs_slam_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALIGN = 256
REGIONS = 10
REC, BIN, OFFSETS, RADII, BLOCK_SUMS, CLAMPED, STATUS, GACC, TOUCHED, WRITTEN = range(REGIONS)


def layout(P):
    buf = (C.c_size_t * (2 * REGIONS))()
    _capi.check(_capi.lib().segs_debug_geometry_layout(P, C.cast(buf, C.c_void_p), REGIONS), "segs_debug_geometry_layout")
    return [(int(buf[2 * i]), int(buf[2 * i + 1])) for i in range(REGIONS)]


@pytest.mark.parametrize("P", [0, 1, 3, 63, 64, 65, 255, 256, 257, 1000, 50_001, 3_000_000])
def test_written_region_is_aligned_disjoint_and_covered_by_the_size_query(P):
    lay = layout(P)
    nblocks = (P + 255) // 256
    # what each region must hold, worked out here from P alone (not taken from the library)
    need = {REC: 64 * P, BIN: 16 * P, OFFSETS: 4 * P, RADII: 4 * P, BLOCK_SUMS: 12 * (nblocks + 1), CLAMPED: 4 * P, STATUS: 64,
            GACC: 64 * P, TOUCHED: 4 * P, WRITTEN: P}
    for i, (off, n) in enumerate(lay):
        assert off % ALIGN == 0 and n >= need[i], (i, off, n)
    spans = sorted((off, off + max(n, need[i])) for i, (off, n) in enumerate(lay))
    for (_, end), (start, _) in zip(spans, spans[1:]):
        assert end <= start, spans
    off, n = lay[WRITTEN]
    padded_end = off + (n + ALIGN - 1) // ALIGN * ALIGN
    assert off + (P + 3) // 4 * 4 <= padded_end           # the consumer clears whole dwords up to the one that holds byte P - 1
    assert all(o < off or o >= padded_end for i, (o, _) in enumerate(lay) if i != WRITTEN)
    assert _capi.lib().segs_geometry_bytes(P) >= padded_end + ALIGN


def test_size_query_is_the_end_of_the_last_region_plus_the_alignment_slack():
    for P in (0, 1, 257, 50_001, 3_000_000):
        lay = layout(P)
        end = max((off + n + ALIGN - 1) // ALIGN * ALIGN for off, n in lay)
        assert _capi.lib().segs_geometry_bytes(P) == end + ALIGN      # slack: the caller's base pointer is aligned up inside the buffer
        assert max(off for off, _ in lay) == lay[WRITTEN][0]          # appended behind the regions that were there before


def test_bad_arguments_are_refused():
    buf = (C.c_size_t * (2 * REGIONS))()
    lib = _capi.lib()
    assert lib.segs_debug_geometry_layout(-1, C.cast(buf, C.c_void_p), REGIONS) != 0
    assert lib.segs_debug_geometry_layout(4, C.cast(buf, C.c_void_p), REGIONS - 1) != 0
    assert lib.segs_debug_geometry_layout(4, None, REGIONS) != 0


def test_flag_and_region_count_in_the_header():
    text = open(os.path.join(ROOT, "include", "segs_raster.h")).read()
    assert re.search(r"^#define\s+SEGS_RASTER_NO_WRITTEN_BYTES\s+128u\b", text, flags=re.M)
    assert re.search(r"^#define\s+SEGS_GEOMETRY_REGIONS\s+%d\b" % REGIONS, text, flags=re.M)
    flags = [int(v) for v in re.findall(r"^#define\s+SEGS_RASTER_[A-Z_]+\s+(\d+)u\b", text, flags=re.M)]
    assert len(flags) == len(set(flags)) and all(f & (f - 1) == 0 for f in flags)      # one bit each, none shared
