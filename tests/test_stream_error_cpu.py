"""The stream error entries and the quality search, as far as they go without a GPU:
  - the numpy restatement of the reference's per-pixel colour error (tests/stream_error_ref.py) against the oracle's limg_compare on the pair kinds of
    tests/test_gpu_compare.py, with 3 and 4 channels -- the GPU tests then compare the kernels with the restatement;
  - what the random originals of the GPU tests are for: red differences on both sides of 128 and alpha differences, which an image against its own decode never has;
  - limg_amd/csrc/limg_hip_quality_step.h built by the host compiler alone (tests/helpers/quality_step_check.cpp) against the search restated in Python, on random and
    non-monotone curves, with the probe bound;
  - limg_hip_error_sum_for_psnr (host only, no context) against the formula in Python doubles."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import limg_amd
from rate_search import max_probes
from stream_error_cases import Version, images, random_original
from stream_error_ref import error_sum, oracle_error_sum, restated_quality_search
from test_gpu_compare import SHAPES, _pairs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "helpers", "quality_step_check.cpp")


@pytest.mark.parametrize("w,h", SHAPES)
@pytest.mark.parametrize("channels", [4, 3])
def test_restatement_against_the_oracles_compare(oracle, w, h, channels):
    pairs = _pairs(w, h)
    for kind in ("random", "extremes", "alpha_only", "red_edge"):
        a, b = pairs[kind]
        mse = oracle.compare(a, b, channels == 4)[1]
        got = error_sum(a, b, channels)
        assert got == round(mse * w * h) and got / (w * h) == mse, (kind, got, mse * w * h)
        assert got == error_sum(b, a, channels), kind  # (symmetric)
        if kind == "alpha_only":
            assert (got == 0) == (channels == 3)
        if kind == "red_edge":
            red = np.abs((a & 0xFF).astype(int) - (b & 0xFF).astype(int))
            assert w * h < 4 or ((red >= 128).any() and (red < 128).any()), "both sides of a red difference of 128"
        # a window of the pair is the sum over its pixels
        win = (w // 3, h // 2, w - w // 3, h - h // 2)
        x, y, ww, hh = win
        assert error_sum(a, b, channels, win) == error_sum(a[y:y + hh, x:x + ww], b[y:y + hh, x:x + ww], channels)


@pytest.mark.parametrize("blocked", [False, True], ids=["version1", "version2"])
def test_the_random_originals_reach_the_weight_swap_and_the_alpha_term(oracle, blocked):
    """what the encoded image as its own original never does here: a red difference of 128 or more, and (4 channels) an alpha term that counts"""
    for name, (img, alpha, channels, dec) in images(oracle, Version(blocked)).items():
        h, w = img.shape
        rnd = random_original(w, h, 100)
        red = np.abs((dec & 0xFF).astype(int) - (rnd & 0xFF).astype(int))
        assert (red >= 128).any() and (red < 128).any(), name
        if channels == 4:
            assert error_sum(dec, rnd, 4) > error_sum(dec, rnd, 3), name
        assert not (np.abs((dec & 0xFF).astype(int) - (img & 0xFF).astype(int)) >= 128).any(), name


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("needs g++")
    exe = str(tmp_path_factory.mktemp("quality") / "quality_step_check")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-static-libubsan", SRC, "-o", exe])

    def run(curve, h_lo, limit):
        """curve[i] = E(h_lo + i) -> (result, within, probes, error sum, max probes, [asked ...]) from the header's functions"""
        text = "%d %d %d\n%s\n" % (h_lo, h_lo + len(curve) - 1, limit, " ".join(str(v) for v in curve))
        r = subprocess.run([exe], input=text, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
        assert r.returncode == 0, (r.returncode, r.stdout)
        head, asked = r.stdout.strip().split(":")
        return tuple(int(v) for v in head.split()) + ([int(v) for v in asked.split()],)

    return run


def _agree(check, curve, h_lo, limit):
    """the header's search against the restatement; -> (branch, result, within, asked)"""
    h_hi = h_lo + len(curve) - 1
    want_h, want_within, want_asked, want_sum = restated_quality_search(lambda h: curve[h - h_lo], h_lo, h_hi, limit)
    h, within, probes, esum, most, asked = check(curve, h_lo, limit)
    ctx = (h_lo, h_hi, limit)
    assert (h, within, asked, esum) == (want_h, want_within, want_asked, want_sum), ctx
    assert probes == len(asked) <= most == max_probes(h_lo, h_hi) and len(set(asked)) == len(asked), ctx
    assert bool(within) == (curve[h - h_lo] <= limit), ctx  # only a measured value is ever returned
    branch = "refused" if not within else ("upper bound" if h == h_hi and len(asked) <= 2 else "bisected")
    return branch, h, within, asked


def test_search_on_random_curves(check):
    rng = np.random.default_rng(7)
    branches = set()
    for n in (1, 2, 3, 4, 5, 8, 9, 31, 33, 64, 512):
        for shape in ("rising", "noisy", "random"):
            if shape == "rising":
                curve = np.cumsum(rng.integers(1, 1000, n))
            elif shape == "noisy":  # rising on the whole, not from step to step: what E() looks like
                curve = np.cumsum(rng.integers(1, 1000, n)) + rng.integers(0, 3000, n)
            else:
                curve = rng.integers(0, 2 ** 40, n)
            curve = [int(v) for v in curve]
            limits = {curve[0] - 1, curve[0], curve[-1], curve[-1] + 1, curve[-1] - 1, (curve[0] + curve[-1]) // 2, curve[n // 2], 0, 2 ** 64 - 1}
            for limit in sorted(v for v in limits if v >= 0):
                for h_lo in (1, 7):
                    branch, h, within, asked = _agree(check, curve, h_lo, limit)
                    branches.add(branch)
                    if shape == "rising" and within:  # on a rising curve the result IS the largest value that meets the limit
                        assert h == h_lo + max(i for i in range(n) if curve[i] <= limit), (n, limit)
    assert branches == {"refused", "upper bound", "bisected"}
    # bounds near the top of the 32-bit range: the mirrored axis does not wrap
    _agree(check, [5, 9, 7, 30], 0xFFFFFFF0, 8)


def test_search_on_the_oracles_non_monotone_curve(check, oracle):
    """520 x 16 RGB photo-noise, seed 11: E(36) = 654054, E(37) = 672780, E(38) = 670651 -- the limit 670651 returns h = 36 after 8 probes although h = 38 meets it too"""
    img = oracle.photo_noise(520, 16, 11)
    curve = [oracle_error_sum(oracle, img, False, 2 * h) for h in range(1, 65)]
    assert (curve[35], curve[36], curve[37]) == (654054, 672780, 670651)
    assert any(a > b for a, b in zip(curve, curve[1:])), "this curve is not monotone: that is what the case is about"
    branch, h, within, asked = _agree(check, curve, 1, 670651)
    assert (branch, h, within, asked) == ("bisected", 36, 1, [1, 64, 33, 49, 41, 37, 35, 36])
    assert max(k for k in range(1, 65) if curve[k - 1] <= 670651) >= 38


def test_error_sum_for_psnr():
    lib = limg_amd.load_library()
    f = lib.limg_hip_error_sum_for_psnr
    for w, h in ((1, 1), (8, 8), (75, 21), (1024, 618), (8192, 8192), (32768, 32768)):
        for alpha in (0, 1):
            for db in (0.0, 10.0, 27.5, 38.0, 40.0, 55.25, 99.0, -3.0):
                want = math.floor(255.0 ** 2 * (12 if alpha else 9) * w * h / 10.0 ** (db / 10.0))
                got = f(w, h, alpha, db)
                assert abs(got - want) <= 1, (w, h, alpha, db, got, want)
    assert f(0, 8, 1, 30.0) == 0 and f(8, 0, 1, 30.0) == 0 and f(8, 8, 1, float("nan")) == 0 and f(8, 8, 1, float("inf")) == 0
    assert f(8, 8, 1, float("-inf")) == 2 ** 64 - 1 and f(1 << 32, 1 << 32, 1, -200.0) == 2 ** 64 - 1
    assert f(8, 8, 1, 40.0) < f(8, 8, 1, 38.0) < f(8, 8, 0, 30.0)
