"""What the tests of the stream error entries and of the stream encode to a quality target share (tests/test_stream_error_cpu.py, tests/test_gpu_stream_error.py,
tests/test_gpu_blocked_stream_error.py, tests/test_gpu_stream_quality.py): the reference's per-pixel colour error restated in numpy, and the search of
include/limg_hip.h ("stream encode to a quality target") restated in Python as tests/rate_search.py restates the budget's.  Not a test module."""
import numpy as np


def pixel_error(decoded, original, channels):
    """(h, w) uint32 pixels x 2 -> (h, w) int64: red^2 x (2 | 3) + green^2 x 4 + blue^2 x (3 | 2) + alpha^2 x 3, the red and blue weights swapped where red^2 >= 0x4000,
    the alpha term with 4 channels only"""
    d, o = (np.ascontiguousarray(a, dtype=np.uint32) for a in (decoded, original))
    assert d.shape == o.shape and channels in (3, 4)
    e = [((d >> (8 * c)) & 0xFF).astype(np.int64) - ((o >> (8 * c)) & 0xFF).astype(np.int64) for c in range(4)]
    red = e[0] * e[0]
    low = red < 0x4000
    err = red * np.where(low, 2, 3) + e[1] * e[1] * 4 + e[2] * e[2] * np.where(low, 3, 2)
    if channels == 4:
        err = err + e[3] * e[3] * 3
    return err


def error_sum(decoded, original, channels, win=None):
    """The sum over window win = (x, y, w, h) of the image (None: all of it); `original` has the image's shape."""
    err = pixel_error(decoded, original, channels)
    if win is not None:
        x, y, w, h = win
        err = err[y:y + h, x:x + w]
    return int(err.sum())


def restated_quality_search(E, h_lo, h_hi, limit):
    """E(h): the error sum of the stream at errorFactor 2 h -> (result h, within, the h values asked for in order, E(result)).  Every value is asked for once."""
    asked, memo = [], {}

    def e(h):
        if h not in memo:
            asked.append(h)
            memo[h] = E(h)
        return memo[h]

    if e(h_lo) > limit:
        return h_lo, 0, asked, e(h_lo)
    if e(h_hi) <= limit:
        return h_hi, 1, asked, e(h_hi)
    lo, hi = h_lo, h_hi
    while hi - lo > 1:
        mid = hi - (hi - lo) // 2
        if e(mid) <= limit:
            lo = mid
        else:
            hi = mid
    return lo, 1, asked, e(lo)


def oracle_error_sum(oracle, img, alpha, error_factor, **kw):
    """E of the oracle's stream at error_factor: mse x pixels of compare(img, pDecoded), an integer far below 2^53"""
    dec = oracle.encode3d(img, alpha, error_factor=error_factor, **kw)["pDecoded"]
    return int(round(oracle.compare(img, dec, alpha)[1] * img.size))
