"""red_select_dead (limg_amd/csrc/limg_hip_encode_rules.h): below a pixel limit of 0x8000 the packed trial's red-weight select decides nothing, so a launch whose
host knows the limit takes the trial without it.  Without a GPU: tests/helpers/red_select_check.cpp is built by the host compiler alone (a program of its own, under
the undefined-behaviour sanitizer), walks all 256^3 difference triples with both weightings and prints what it counts."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "helpers", "red_select_check.cpp")


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("needs g++")
    exe = str(tmp_path_factory.mktemp("redsel") / "red_select_check")
    subprocess.check_call([gxx, "-std=c++17", "-O2", "-Wall", "-Werror", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-static-libubsan", SRC, "-o", exe])

    def run(questions):
        r = subprocess.run([exe], input="\n".join(questions) + "\n", stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
        assert r.returncode == 0, (r.returncode, r.stdout)
        lines = r.stdout.strip().split("\n")
        assert len(lines) == len(questions), r.stdout
        return [tuple(int(v) for v in line.split()) for line in lines]

    return run


def test_the_two_weightings_agree_below_the_bound_and_not_at_it(ask):
    """all 256^3 (|dR|, |dG|, |dB|): for every limit up to 32767 the same pixel verdict and, where the pixel passes, the same value; at 32768 not -- the bound is tight"""
    limits = [0, 42, 2100, 32759, 32767]
    got = ask(["w %d" % t for t in limits + [32768]])
    high_red = 128 * 256 * 256  # |dR| >= 128: the triples the select acts on are part of the walk
    for t, (verdicts, values, seen) in zip(limits, got):
        assert (verdicts, values, seen) == (0, 0, high_red), t
    verdicts, values, seen = got[-1]
    assert verdicts > 0 and seen == high_red, got[-1]


def test_red_select_dead_by_error_factor(ask):
    dead, alive = [0, 100, 1560, 1561], [1562, 1563, 3000, 4000000000]
    got = ask(["d %d" % ef for ef in dead + alive])
    assert [g[0] for g in got] == [1] * len(dead) + [0] * len(alive), got
    at = dict(zip(dead + alive, (g[1] for g in got)))
    assert at[100] == 2100 and at[1561] == 32760 and at[1562] == 32802 and at[4000000000] == 0xFFFFFFFF
