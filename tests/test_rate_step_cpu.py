"""limg_amd/csrc/limg_hip_rate_step.h -- the search of the budgeted stream encode, one function for k_rate_step and for the fallback host loop -- without a GPU:
tests/helpers/rate_step_check.cpp is built by the host compiler alone, reads a size curve and a budget, runs rate_step until it is done and prints the result and
the values it asked for.  Compared with the algorithm of include/limg_hip.h restated in Python (tests/rate_search.py) on size curves computed from the oracle
(Oracle.encode3d + stream.field_bits) and on synthetic ones for ranges of one and two values.  The cases must reach every branch of the algorithm, and the
gradient's curve shows that the result is the algorithm's, not an exhaustive minimum: the stream's size is not monotone in errorFactor."""
import os
import shutil
import subprocess

import pytest

from rate_search import max_probes, oracle_size, restated_search

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "helpers", "rate_step_check.cpp")


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("needs g++")
    exe = str(tmp_path_factory.mktemp("rate") / "rate_step_check")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-static-libubsan", SRC, "-o", exe])

    def run(curve, h_lo, budget):
        """curve[i] = size(h_lo + i) -> (result, within, probes, bytes, max probes, [asked ...]) from the header's function"""
        text = "%d %d %d\n%s\n" % (h_lo, h_lo + len(curve) - 1, budget, " ".join(str(v) for v in curve))
        r = subprocess.run([exe], input=text, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
        assert r.returncode == 0, (r.returncode, r.stdout)
        head, asked = r.stdout.strip().split(":")
        return tuple(int(v) for v in head.split()) + ([int(v) for v in asked.split()],)

    return run


def _agree(check, curve, h_lo, budget):
    """the header's search against the restatement; -> (branch, result, within, asked)"""
    h_hi = h_lo + len(curve) - 1
    want_h, want_within, want_asked, want_bytes = restated_search(lambda h: curve[h - h_lo], h_lo, h_hi, budget)
    h, within, probes, nbytes, most, asked = check(curve, h_lo, budget)
    ctx = (h_lo, h_hi, budget)
    assert (h, within, asked, nbytes) == (want_h, want_within, want_asked, want_bytes), ctx
    assert probes == len(asked) <= most == max_probes(h_lo, h_hi), ctx
    if within:
        assert curve[h - h_lo] <= budget, ctx  # only a measured value is ever returned
    branch = "refused" if not within else ("lo" if h == h_lo and len(asked) <= 2 and curve[0] <= budget else "bisected")
    return branch, h, within, asked


@pytest.fixture(scope="module")
def curves(oracle):
    """{name: (hLo, [size(h) for h in hLo .. hHi])} from the oracle: errorFactor = 2 h"""
    noise = oracle.photo_noise(264, 24, 3)
    gradient = oracle.random_gradient(256, 32, 5, True)
    return {"noise_rgba": (1, [oracle_size(oracle, noise, True, 2 * h) for h in range(1, 513)]),
            "gradient_rgb": (1, [oracle_size(oracle, gradient, False, 2 * h) for h in range(1, 129)])}


def test_search_on_oracle_curves(check, curves):
    branches = set()
    for name, (h_lo, curve) in curves.items():
        floor, top = min(curve), curve[0]
        assert floor < curve[-1] or floor < top, name
        budgets = [floor - 8, curve[-1] - 8, curve[-1], top, top + 8, top - 8, (top + curve[-1]) // 2] + sorted(set(curve))[1:-1:7]
        for budget in budgets:
            branch, h, within, asked = _agree(check, curve, h_lo, budget)
            branches.add(branch)
            if budget < floor:
                assert not within and h == h_lo + len(curve) - 1 and asked == [h], (name, budget)
            if budget >= top:
                assert within and h == h_lo and len(asked) == 2, (name, budget)
            if curve[-1] <= budget < top:
                assert within and h_lo < h and len(asked) > 2, (name, budget)
    assert branches == {"refused", "lo", "bisected"}


def test_the_result_is_the_algorithms_not_an_exhaustive_minimum(check, curves):
    """256 x 32 opaque gradient as RGB: 10264 bytes at errorFactor 34, 10280 at 36, 10304 from 66 on.  A budget of 10270 over [2, 256] is refused -- size(128) does not
    fit -- although h = 17 would; and where the bisection does run it may land above the smallest h that fits."""
    h_lo, curve = curves["gradient_rgb"]
    size = lambda h: curve[h - h_lo]  # noqa: E731
    assert (size(17), size(18), size(33), size(128)) == (10264, 10280, 10304, 10304)
    assert any(a < b for a, b in zip(curve, curve[1:])), "this curve is not monotone: that is what the case is about"
    branch, h, within, asked = _agree(check, curve, h_lo, 10270)
    assert (branch, h, within, asked) == ("refused", 128, 0, [128])
    # over [2, 34] the same budget is met at the upper end; exhaustive search gives the same or a smaller h
    branch, h, within, asked = _agree(check, curve[:17], h_lo, 10270)
    assert within and size(h) <= 10270 and min(k for k in range(1, 18) if size(k) <= 10270) <= h


def test_ranges_of_one_and_two_values(check):
    seen = set()
    for curve, budget in (([500], 499), ([500], 500), ([900, 500], 499), ([900, 500], 500), ([900, 500], 899), ([900, 500], 900), ([500, 900], 700), ([500, 900], 900)):
        for h_lo in (1, 7, 0x7FFFFFFE):
            branch, h, within, asked = _agree(check, curve, h_lo, budget)
            seen.add((len(curve), branch))
            assert len(asked) <= len(curve)
    assert seen == {(1, "refused"), (1, "lo"), (2, "refused"), (2, "lo"), (2, "bisected")}


def test_probe_bound_on_long_ranges(check):
    """a strictly falling curve over ranges whose length is and is not a power of two: every budget between two values, never more than 2 + ceil(log2(hHi - hLo)) probes"""
    for n in (3, 4, 5, 8, 9, 31, 33, 512):
        curve = [10000 - 8 * i for i in range(n)]
        for budget in [curve[i] + 4 for i in range(0, n, max(1, n // 16))] + [curve[-1] - 1]:
            _agree(check, curve, 5, budget)
