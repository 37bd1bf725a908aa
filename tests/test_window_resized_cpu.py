"""The numpy restatement of the resized window decode's contract (tests/window_resized.py) against itself and against float64 bilinear interpolation, without a GPU:
the three consequences the header states (identity, pure level, flip), the AUTO level for a table of sizes, the clamp for a rectangle that ends in the columns a level
drops, and the derived bound of 1.52 byte steps at level 0 on noise.  The GPU tests compare the library with this restatement bit for bit."""
import numpy as np
import pytest
import torch

import window_resized as R
import window_scaled as WS


@pytest.fixture(scope="module")
def noise():
    rng = np.random.RandomState(1)
    img = rng.randint(0, 2 ** 32, size=(104, 168), dtype=np.uint64).astype(np.uint32)
    return img, WS.pyramid(img)


def test_identity(noise):
    img, pyr = noise
    for rect in ((5, 3, 40, 30), (0, 0, 168, 104), (167, 103, 1, 1), (0, 50, 168, 1)):
        r, L = R.resize(pyr, rect, rect[2], rect[3], 0)
        assert L == 0 and np.array_equal(r, img[rect[1]:rect[1] + rect[3], rect[0]:rect[0] + rect[2]]), rect


def test_pure_level(noise):
    img, pyr = noise
    for L in (1, 2, 3):
        k = 1 << L
        for x, y, w, h in ((2, 3, 10, 7), (0, 0, 168 >> L, 104 >> L), (1, 0, 1, 1)):
            r, _ = R.resize(pyr, (x * k, y * k, w * k, h * k), w, h, L)
            assert np.array_equal(r, pyr[L][y:y + h, x:x + w]), (L, x, y, w, h)
            r2, chosen = R.resize(pyr, (x * k, y * k, w * k, h * k), w, h)
            assert chosen == L and np.array_equal(r, r2), (L, chosen)


def test_flip_is_the_column_reversal(noise):
    _, pyr = noise
    for rect, ow, oh, L in (((7, 9, 77, 55), 20, 12, None), ((7, 9, 77, 55), 131, 90, 0), ((0, 0, 168, 104), 33, 9, 2), ((160, 100, 8, 4), 5, 5, 3)):
        a, _ = R.resize(pyr, rect, ow, oh, L)
        b, _ = R.resize(pyr, rect, ow, oh, L, flip=True)
        assert np.array_equal(b, a[:, ::-1]), (rect, ow, oh, L)


def test_auto_level_table():
    for (sw, sh, ow, oh), want in (((168, 104, 20, 12), 3), ((160, 96, 21, 13), 2), ((168, 104, 84, 52), 1), ((100, 100, 51, 33), 0), ((167, 103, 20, 12), 3), ((1792, 1792, 224, 224), 3),
                                   ((1791, 1792, 224, 224), 2), ((224, 224, 224, 224), 0), ((10, 10, 40, 40), 0), ((4096, 16, 16, 16), 0), ((4096, 32, 16, 16), 1), ((1, 1, 1, 1), 0),
                                   ((32768, 32768, 1, 1), 3)):
        assert R.auto_level(sw, sh, ow, oh) == want, (sw, sh, ow, oh)
        L = R.auto_level(sw, sh, ow, oh)
        assert L == 0 or ((sw >> L) >= ow and (sh >> L) >= oh)
        assert L == 3 or not ((sw >> (L + 1)) >= ow and (sh >> (L + 1)) >= oh)


def test_taps_clamp_to_the_level_pixels_the_rectangle_touches(noise):
    """168 x 104 at level 3 is 21 x 13; 531 wide at level 3 keeps 66 columns and drops 3: a rectangle that ends there taps column 65 at most.  A rectangle in the
    middle never taps outside its own level pixels, whatever the output size"""
    a, b, f = R.axis(500, 31, 13, 3, 531 >> 3)
    assert a.min() >= 500 >> 3 and b.max() == 65 and a.max() <= 65 and ((f >= 0) & (f <= 256)).all()
    for s0, length, out, L, size in ((40, 33, 100, 0, 168), (41, 33, 7, 1, 168), (3, 1, 9, 0, 168), (100, 68, 5, 2, 168), (0, 168, 400, 3, 168)):
        a, b, f = R.axis(s0, length, out, L, size >> L)
        lo, hi = s0 >> L, min((s0 + length - 1) >> L, (size >> L) - 1)
        assert a.min() >= lo and b.max() <= hi and (b - a <= 1).all() and (b >= a).all() and ((f >= 0) & (f <= 256)).all()
        assert (np.diff(a) >= 0).all() and (np.diff(b) >= 0).all()  # what lets a tile's footprint come from its first and last column
    _, pyr = noise
    assert R.level_ok(168, 104, (160, 96, 8, 8), 3) and not R.level_ok(531, 19, (528, 0, 3, 19), 3) and not R.level_ok(5, 3, (0, 0, 5, 3), 2)


def test_mixed_jobs_cover_every_level_size_and_flip():
    """the GPU tests' mixed batch, on the images it uses: all explicit levels and AUTO, both flips, up- and down-scaling occur"""
    for sizes in (((531, 19), (72, 40), (64, 64)), ((96, 72), (67, 45), (64, 48))):
        jobs = R.mixed_jobs([(None, 0, w, h, None) for w, h in sizes])
        assert {j[4] for j in jobs} == {0, 1, 2, 3, None} and {j[5] for j in jobs} == {False, True} and {j[6] for j in jobs} == {False, True}
        assert any(j[2] > j[1][2] for j in jobs) and any(j[2] < j[1][2] for j in jobs)
        assert all(j[4] is None or R.level_ok(j[0][2], j[0][3], j[1], j[4]) for j in jobs)


def test_level0_is_within_1_52_of_float64_bilinear(noise):
    """weights rounded to 1 / 256 (at most 1 / 512 off, plus two floors of 2^-16) cost less than 0.506 byte steps per axis, the final rounding 0.5: below 1.52 in all"""
    img, pyr = noise
    rng = np.random.RandomState(2)
    worst = 0.0
    for _ in range(300):
        sw, sh = int(rng.randint(1, 100)), int(rng.randint(1, 80))
        x0, y0 = int(rng.randint(0, 168 - sw + 1)), int(rng.randint(0, 104 - sh + 1))
        ow, oh = int(rng.randint(1, 130)), int(rng.randint(1, 100))
        r, _ = R.resize(pyr, (x0, y0, sw, sh), ow, oh, 0)
        crop = np.ascontiguousarray(img[y0:y0 + sh, x0:x0 + sw]).view(np.uint8).reshape(sh, sw, 4).astype(np.float64)
        ref = torch.nn.functional.interpolate(torch.from_numpy(crop).permute(2, 0, 1)[None], size=(oh, ow), mode="bilinear", align_corners=False, antialias=False)[0]
        worst = max(worst, float(np.abs(r.view(np.uint8).reshape(oh, ow, 4).astype(np.float64) - ref.permute(1, 2, 0).numpy()).max()))
    print("worst |fixed - float64 bilinear| at level 0:", worst)
    assert worst <= 1.52, worst
