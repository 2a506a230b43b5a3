"""The NumPy restatement of the stereo matcher (tests/_sgm_ref.py) held to ground truth, so that the GPU test, which compares the
kernels with that restatement bit for bit, cannot be satisfied by two copies of one mistake.  No GPU and no library call here."""
import numpy as np
import pytest

from tests import _sgm_ref as ref

H, W, D = 40, 160, 64


@pytest.fixture(scope="module")
def pair():
    return ref.shifted_pair(H, W, 7, 19, seed=7)


def _region():
    reg = np.zeros((H, W), dtype=bool)
    reg[3:H - 3, 23:W - 4] = True
    reg[H // 2 - 4:H // 2 + 4] = False            # four rows either side of the seam between the two disparities
    return reg


@pytest.mark.parametrize("paths", [4, 8])
@pytest.mark.parametrize("dmin", [0, 5])
def test_shifted_pair_is_recovered(pair, paths, dmin):
    left, right, truth = pair
    st = ref.sgm(left, right, D=D, dmin=dmin, P1=10, P2=120, u=5, paths=paths, lr_max_diff=1, median=True)
    disp16 = st["disp16"].astype(np.int64)
    valid = disp16 != 16 * (dmin - 1)
    reg = _region()
    frac_valid = valid[reg].mean()
    within = (np.abs(disp16 - 16 * truth)[reg & valid] <= 16).mean()
    print(f"paths={paths} dmin={dmin}: valid {frac_valid:.4f}, within one pixel {within:.4f}")
    assert frac_valid >= 0.99
    assert within >= 0.99
    # A valid pixel has a right pixel: its rounded disparity, min_disparity included, never exceeds its column (stage 7), so
    # no pixel with x < min_disparity is valid and no pixel with x < d_t is valid at its true disparity.  (That EVERY pixel with
    # x < d_t is invalid does not follow from the specification: the census-less rows 0-2 tie at d* = 0, which passes both
    # checks from x = min_disparity on, and below the seam a few pixels left of x = 19 pass with a false match -- 52 such pixels
    # at 4 paths and 74 at 8 with min_disparity 5, none of them at the true disparity.)
    xs = np.arange(W)[None, :] * np.ones((H, 1), dtype=np.int64)
    assert (((disp16 + 8) >> 4)[valid] <= xs[valid]).all()
    assert not valid[:, :dmin].any()
    assert not (valid & (xs < truth) & (np.abs(disp16 - 16 * truth) < 8)).any()
    # invalid pixels carry exactly the marker that the reference's `disp / 16 > min_disparity` drops
    assert ((disp16[valid] > 16 * dmin - 16) & (disp16[valid] <= 16 * (dmin + D))).all()


def test_vectorised_aggregation_equals_the_per_pixel_recurrence(pair):
    """aggregate() walks whole lines at once; this is stage 4 read literally, one pixel at a time."""
    left, right, _ = pair
    C = ref.cost_volume(ref.census(left[:12, :30]), ref.census(right[:12, :30]), 64, 3)
    h, w, d = C.shape
    for dx, dy in ref.DIRECTIONS:
        L = np.zeros_like(C)
        for y in (range(h) if dy >= 0 else range(h - 1, -1, -1)):
            for x in (range(w) if dx >= 0 else range(w - 1, -1, -1)):
                py, px = y - dy, x - dx
                if not (0 <= py < h and 0 <= px < w):
                    L[y, x] = C[y, x]
                    continue
                p = L[py, px]
                m = p.min()
                best = np.minimum(p, m + 120)
                best[1:] = np.minimum(best[1:], p[:-1] + 10)
                best[:-1] = np.minimum(best[:-1], p[1:] + 10)
                L[y, x] = C[y, x] + best - m
        assert np.array_equal(L, ref.aggregate(C, dx, dy, 10, 120)), (dx, dy)
        assert L.max() <= 255


def test_census_bit_order_and_border():
    img = np.zeros((7, 9), dtype=np.uint8)
    assert ref.census(img).sum() == 0
    img[0, 0] = 1                                   # offset (dy, dx) = (-3, -4) of the one census pixel (3, 4): bit 0
    c = ref.census(img)
    assert c[3, 4] == 1 and np.count_nonzero(c) == 1
    img[:] = 0
    img[3, 3] = 1                                   # (0, -1), the last offset: bit 30
    assert ref.census(img)[3, 4] == 1 << 30
    img[:] = 0
    img[6, 8] = 1                                   # the mirror of bit 0 is larger: no bit
    assert ref.census(img)[3, 4] == 0
    assert ref.census(np.ones((6, 8), dtype=np.uint8)).shape == (6, 8) and not ref.census(np.ones((6, 20), dtype=np.uint8)).any()


def test_subpixel_offset_is_a_floor():
    # num = -3, den = 8: (16 * -3 + 8) / 16 = -2.5 -> -3 (truncation would give -2)
    assert int(ref.floor_frac(-3, 8)) == -3
    assert int(ref.floor_frac(3, 8)) == 3           # 56 / 16 = 3.5 -> 3
    assert int(ref.floor_frac(-1, 1)) == -8 and int(ref.floor_frac(1, 1)) == 8      # the ends of [-8, 8]
    assert int(ref.floor_frac(5, 0)) == 0 and int(ref.floor_frac(0, 7)) == 0
    # and through the winner stage: S = (.., 9, 4, 12, ..) around d* = 2 -> num = -3, den = 13: floor(-35 / 26) = -2
    S = np.full((1, 1, 64), 50, dtype=np.int64)
    S[0, 0, 1:4] = (9, 4, 12)
    assert int(ref.winner(S, 0)[0, 0]) == 16 * 2 - 2


def test_constant_image_ties_everywhere():
    img = np.full((20, 40), 93, dtype=np.uint8)
    st = ref.sgm(img, img, D=64, dmin=0, u=5, paths=8)
    assert not st["census_left"].any() and not st["S"][:, :, 0].any()
    assert (st["raw_winner"] == 0).all() and (st["raw_median"] == 0).all()
    # d_r ties at 0 too, so the check keeps every pixel: disparity 0, which is not a depth
    st = ref.sgm(img, img, D=64, dmin=0, u=5, paths=4, fb16=ref.fb16_of(400.0, 0.1))
    assert (st["disp16"] == 0).all() and not st["depth"].any()


def test_grey_conversion_rounds_half_to_even_and_clamps():
    k = np.arange(0, 255, dtype=np.float32)
    halves = (k + np.float32(0.5)) / np.float32(255.0)
    rgb = np.stack([halves, halves, halves]).reshape(3, 1, -1)
    got = ref.rgb_to_gray_u8(rgb)
    g = (np.float32(0.299) * halves + np.float32(0.587) * halves) + np.float32(0.114) * halves
    assert np.array_equal(got[0], np.rint(g * np.float32(255.0)).astype(np.uint8))
    odd = np.array([[-1.0, 2.0, np.nan, 0.0, 1.0]], dtype=np.float32)
    assert ref.rgb_to_gray_u8(np.stack([odd, odd, odd])).tolist() == [[0, 255, 0, 0, 255]]
