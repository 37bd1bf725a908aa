"""limg_amd/csrc/limg_hip_encode_rules.h -- the bit-crush thresholds of an error factor, the forced shift triple and the images of one launch pair of a list, each
one function for the host units and the kernels -- without a GPU: tests/helpers/encode_rules_check.cpp is built by the host compiler alone (a program of its own,
under the undefined-behaviour sanitizer) and prints the header's answers, which are compared with the rules restated here."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "helpers", "encode_rules_check.cpp")
U32 = 0xFFFFFFFF


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("needs g++")
    exe = str(tmp_path_factory.mktemp("rules") / "encode_rules_check")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-static-libubsan", SRC, "-o", exe])

    def run(questions):
        """["t 100", "f 8 8 8", ...] -> one tuple of ints per question"""
        r = subprocess.run([exe], input="\n".join(questions) + "\n", stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
        assert r.returncode == 0, (r.returncode, r.stdout)
        lines = r.stdout.strip().split("\n")
        assert len(lines) == len(questions), r.stdout
        return [tuple(int(v) for v in line.split()) for line in lines]

    return run


def restated_thresholds(error_factor):
    """the reference's formulas (src/limg.cpp:2190-2212) -> (maxPixel32, maxBlock, blockLimitFull, crushBits)"""
    h = error_factor // 2
    return min(42 * h, U32), 28 * h, min(112 * h, U32), int(error_factor != 0)


def test_thresholds(ask):
    efs = [0, 1, 2, 3, 100, 1024, U32]
    # the last fitting and the first clamped h of maxPixel32 and of blockLimitFull, each as an even and an odd error factor
    edges = [102261126, 102261127, 38347922, 38347923]
    efs += [2 * h + odd for h in edges for odd in (0, 1)]
    got = ask(["t %d" % ef for ef in efs])
    for ef, g in zip(efs, got):
        assert g == restated_thresholds(ef), ef
    at = dict(zip(efs, got))
    assert at[0] == (0, 0, 0, 0) and at[1] == (0, 0, 0, 1) and at[2] == (42, 28, 112, 1) and at[3] == at[2]
    assert at[100] == (2100, 1400, 5600, 1) and at[1024] == (21504, 14336, 57344, 1)
    assert at[2 * 102261126][0] == 4294967292 and at[2 * 102261127][0] == U32
    assert at[2 * 38347922][2] == 4294967264 and at[2 * 38347923][2] == U32
    assert at[U32] == (U32, 28 * (U32 // 2), U32, 1) and at[U32][1] > U32, "maxBlock is 64 bits and never clamps"


def test_forced_shifts(ask):
    cases = {(8, 8, 8): (8, 8, 8), (0, 0, 0): (0, 0, 0), (7, 8, 1): (7, 8, 1), (-1, -1, -1): (-1, -1, -1), (9, 0, 0): (-1, -1, -1), (0, -1, 0): (-1, -1, -1)}
    got = ask(["f %d %d %d" % k for k in cases])
    assert got == list(cases.values())


def restated_chunk(blocks, strips, hook, record):
    chunk = (1 << 30) // (blocks * record)
    if chunk * strips > 0x7FFFFFFF:
        chunk = 0x7FFFFFFF // strips
    if hook > 0:
        chunk = min(chunk, hook)
    return max(chunk, 1)


def test_list_chunk(ask):
    """blocks and strips are one image's.  An image has at most as many work strips as blocks, so for every real shape -- one-block images, which have the most strips
    per record byte, included -- the 1 GiB rule is at or below the strip rule's limit: that rule decides only for arguments no image has, and is tested with such."""
    (record,), = ask(["r"])
    assert record == 64
    gib = (512 * 512, 16 * 512)  # 4096 x 4096: the 1 GiB rule decides
    one_block = (1, 1)           # 8 x 8: still the 1 GiB rule, 2^30 / 64 images
    strip_rule = (1, 1000)       # (no image): 2^24 x 1000 strip ids do not fit 31 bits
    huge = ((1 << 30) // record + 1, 1 << 19)  # one image's records alone exceed 1 GiB: the quotient is 0
    cases = [gib, one_block, strip_rule, huge]
    got = ask(["c %d %d %d" % (b, s, hook) for b, s in cases for hook in (0, 3)])
    want = [(restated_chunk(b, s, hook, record),) for b, s in cases for hook in (0, 3)]
    assert got == want
    free = dict(zip(cases, [g[0] for g in got[0::2]]))
    assert free[gib] == (1 << 30) // (gib[0] * record) == 64 and free[gib] * gib[1] <= 0x7FFFFFFF
    assert free[one_block] == 1 << 24
    assert free[strip_rule] == 0x7FFFFFFF // 1000 < (1 << 30) // record
    assert free[huge] == 1
    # the hook asks for fewer images per pair and never lifts a bound (list_chunk_end's rule for a list of mixed shapes: tests/test_list_plan_cpu.py)
    assert [g[0] for g in got[1::2]] == [3, 3, 3, 1], "the hook overrides each but the image that is alone over a bound"
