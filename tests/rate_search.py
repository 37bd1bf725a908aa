"""What the tests of the stream's size probe and budget search share (tests/test_rate_step_cpu.py, tests/test_gpu_stream_budget.py): the search of
include/limg_hip.h ("stream encode to a byte budget") restated in Python, and the oracle's stream sizes.  Not a test module."""
from oracle import stream as S


def restated_search(size, h_lo, h_hi, budget):
    """size(h): the stream's bytes at errorFactor 2 h -> (result h, within, the h values asked for in order, size(result)).  Every value is asked for once."""
    asked, memo = [], {}

    def sz(h):
        if h not in memo:
            asked.append(h)
            memo[h] = size(h)
        return memo[h]

    if sz(h_hi) > budget:
        return h_hi, 0, asked, sz(h_hi)
    if sz(h_lo) <= budget:
        return h_lo, 1, asked, sz(h_lo)
    lo, hi = h_lo, h_hi
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if sz(mid) <= budget:
            hi = mid
        else:
            lo = mid
    return hi, 1, asked, sz(hi)


def max_probes(h_lo, h_hi):
    """2 + ceil(log2(hHi - hLo)); a range of one value: 1"""
    d = h_hi - h_lo
    return 1 if d == 0 else 2 + (d - 1).bit_length()


def oracle_size(oracle, img, alpha, error_factor, **kw):
    """64 + 56 blocks + 8 x the blocks' field bits: the length of S.pack of the oracle's encode, without packing"""
    enc = oracle.encode3d(img, alpha, planes=False, extras=True, error_factor=error_factor, **kw)
    by, bx = enc["shifts"].shape[:2]
    words = sum(sum(S.field_bits(enc["shifts"][j, i], enc["records"][j, i], 4 if alpha else 3)[0]) for j in range(by) for i in range(bx))
    return 64 + 56 * bx * by + 8 * words
