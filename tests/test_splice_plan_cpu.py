"""limg_amd/csrc/limg_hip_splice_plan.h -- which piece lists a stream splice accepts and the runs it cuts them into -- without a GPU: tests/helpers/splice_plan_check.cpp
is built by the host compiler alone (a program of its own, under the undefined-behaviour sanitizer) and prints the header's answers, which are compared with the rules
as tests/stream_splice_ref.py restates them block by block."""
import os
import shutil
import subprocess

import pytest

import stream_splice_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "helpers", "splice_plan_check.cpp")


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("needs g++")
    exe = str(tmp_path_factory.mktemp("splice") / "splice_plan_check")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-static-libubsan", SRC, "-o", exe])

    def run(questions):
        """questions: (w, h, pieces) -> per question None (refused) or (runs, item prefix)"""
        text = "".join("%d %d %d %s\n" % (w, h, len(pieces), " ".join(str(v) for p in pieces for v in p)) for w, h, pieces in questions)
        r = subprocess.run([exe], input=text, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
        assert r.returncode == 0, (r.returncode, r.stdout[-2000:])
        lines = r.stdout.split("\n")[:-1]
        assert len(lines) == len(questions), (len(lines), len(questions))
        out = []
        for line in lines:
            v = [int(t) for t in line.split()]
            if v[0] == 0:
                assert v == [0], line
                out.append(None)
                continue
            n = v[1]
            assert len(v) == 3 + 5 * n, line
            out.append(([tuple(v[3 + 5 * i:7 + 5 * i]) for i in range(n)], [v[7 + 5 * i] for i in range(n)] + [v[2]]))
        return out

    return run


def whole(w, h):
    """the whole w x h image as one piece of itself"""
    return (w, h, 0, 0, 0, 0, R.blocks(w), R.blocks(h))


def tiling(w, h, cuts_x, cuts_y, sources=None):
    """the tiles of a w x h image cut at the block columns / rows cuts_x / cuts_y; every tile from a source of exactly its own size (sources None), or from the
    image itself at its own place"""
    xs, ys = [0] + list(cuts_x) + [R.blocks(w)], [0] + list(cuts_y) + [R.blocks(h)]
    pieces = []
    for j in range(len(ys) - 1):
        for i in range(len(xs) - 1):
            bw, bh = xs[i + 1] - xs[i], ys[j + 1] - ys[j]
            if sources == "self":
                pieces.append((w, h, xs[i], ys[j], xs[i], ys[j], bw, bh))
            else:
                pieces.append((min(8 * bw, w - 8 * xs[i]), min(8 * bh, h - 8 * ys[j]), 0, 0, xs[i], ys[j], bw, bh))
    return pieces


ACCEPTED = [
    ("one piece", 64, 64, [whole(64, 64)]),
    ("one piece, both edges partial", 261, 20, [whole(261, 20)]),
    ("one block", 8, 8, [whole(8, 8)]),
    ("smaller than a block", 3, 5, [whole(3, 5)]),
    ("a crop from the interior", 24, 16, [(261, 44, 4, 2, 0, 0, 3, 2)]),
    ("a crop that keeps the source's partial corner", 21, 12, [(261, 44, 30, 4, 0, 0, 3, 2)]),
    ("2 x 2 from four sources", 261, 20, tiling(261, 20, [16], [1])),
    ("2 x 2 of itself", 261, 20, tiling(261, 20, [16], [1], "self")),
    ("strips", 264, 48, tiling(264, 48, [], [2, 4])),
    ("strips, the last one partial", 264, 45, tiling(264, 45, [], [1, 5])),
    ("unequal pieces", 72, 40, [(72, 8, 0, 0, 0, 0, 9, 1), (16, 32, 0, 0, 0, 1, 2, 4), (56, 16, 0, 0, 2, 1, 7, 2), (100, 100, 3, 5, 2, 3, 7, 2)]),
    ("pieces listed out of order", 72, 40, [(100, 100, 3, 5, 2, 3, 7, 2), (56, 16, 0, 0, 2, 1, 7, 2), (72, 8, 0, 0, 0, 0, 9, 1), (16, 32, 0, 0, 0, 1, 2, 4)]),
    ("130 blocks wide", 1040, 16, [whole(1040, 16)]),
    ("130 blocks wide, beside a narrow one", 1048, 16, [(1040, 16, 0, 0, 0, 0, 130, 2), (8, 16, 0, 0, 130, 0, 1, 2)]),
    ("1025 runs", 16, 8200, [whole(16, 8200)]),
]

T22 = tiling(64, 32, [4], [2])  # 2 x 2 tiles of 4 x 2 blocks each
REFUSED = [
    ("count == 0", 64, 64, []),
    ("a gap", 64, 32, T22[:3]),
    ("a gap inside a row", 64, 32, T22[:1] + [(24, 16, 0, 0, 5, 0, 3, 2)] + T22[2:]),
    ("an overlap", 64, 32, T22 + [T22[3]]),
    ("an overlap of one block", 64, 32, T22[:1] + [(40, 16, 0, 0, 3, 0, 5, 2)] + T22[2:]),
    ("overlap and gap of equal area", 64, 32, T22[:3] + [T22[2]]),
    ("a piece outside its source in x", 64, 32, T22[:3] + [(24, 16, 0, 0, 4, 2, 4, 2)]),
    ("a piece outside its source in y", 64, 32, T22[:3] + [(32, 8, 0, 0, 4, 2, 4, 2)]),
    ("a piece that starts outside its source", 64, 32, T22[:3] + [(32, 16, 4, 0, 4, 2, 4, 2)]),
    ("a piece outside the output", 64, 32, T22[:3] + [(64, 16, 0, 0, 4, 2, 5, 2)]),
    ("zero-width piece", 64, 32, T22 + [(32, 16, 0, 0, 0, 0, 0, 2)]),
    ("zero-height piece", 64, 32, T22 + [(32, 16, 0, 0, 0, 0, 4, 0)]),
    ("a zero-size source", 64, 32, T22[:3] + [(0, 16, 0, 0, 4, 2, 4, 2)]),
    # the edge rule, on each axis, both ways round
    ("x: a clipped output column from a whole source column", 61, 32, [(64, 32, 0, 0, 0, 0, 8, 4)]),
    ("x: a clipped output column from an interior source column", 61, 32, [(128, 32, 0, 0, 0, 0, 8, 4)]),
    ("x: a clipped output column from a column clipped otherwise", 61, 32, [(62, 32, 0, 0, 0, 0, 8, 4)]),
    ("x: a whole output column from a clipped source column", 64, 32, [(61, 32, 0, 0, 0, 0, 8, 4)]),
    ("x: an interior output column from a clipped source column", 64, 32, [(29, 32, 0, 0, 0, 0, 4, 4), (32, 32, 0, 0, 4, 0, 4, 4)]),
    ("y: a clipped output row from a whole source row", 64, 29, [(64, 32, 0, 0, 0, 0, 8, 4)]),
    ("y: a clipped output row from an interior source row", 64, 29, [(64, 64, 0, 0, 0, 0, 8, 4)]),
    ("y: a clipped output row from a row clipped otherwise", 64, 29, [(64, 30, 0, 0, 0, 0, 8, 4)]),
    ("y: a whole output row from a clipped source row", 64, 32, [(64, 29, 0, 0, 0, 0, 8, 4)]),
    ("y: an interior output row from a clipped source row", 64, 32, [(64, 13, 0, 0, 0, 0, 8, 2), (64, 16, 0, 0, 0, 2, 8, 2)]),
]


def test_accepted_tilings_and_their_runs(ask):
    got = ask([(w, h, p) for _, w, h, p in ACCEPTED])
    for (name, w, h, pieces), answer in zip(ACCEPTED, got):
        want = R.runs(pieces, w, h)
        assert want is not None, (name, "the restatement refuses it")
        assert answer is not None, (name, "refused")
        runs, item_base = answer
        assert runs == want, name
        assert item_base == R.items(want), name
        # what the order means: the runs abut in the output's raster order and cover it
        at = 0
        for _, _, dst, count in runs:
            assert dst == at, name
            at += count
        assert at == R.blocks(w) * R.blocks(h), name


def test_run_shapes(ask):
    """the cases by number: a run per block row of a piece; a 130-block run is three items; 1025 runs for the 16 x 8200 strip"""
    by_name = {name: (w, h, p) for name, w, h, p in ACCEPTED}
    wide, beside, tall, unequal = ask([by_name["130 blocks wide"], by_name["130 blocks wide, beside a narrow one"], by_name["1025 runs"], by_name["unequal pieces"]])
    assert wide == ([(0, 0, 0, 130), (0, 130, 130, 130)], [0, 3, 6])
    assert beside[0] == [(0, 0, 0, 130), (1, 0, 130, 1), (0, 130, 131, 130), (1, 1, 261, 1)] and beside[1] == [0, 3, 4, 7, 8]
    assert len(tall[0]) == 1025 and tall[0][1024] == (0, 2048, 2048, 2) and tall[1][-1] == 1025
    # the four pieces of "unequal pieces", row by row: 9 | 2 + 7 | 2 + 7 | 2 + 7 | 2 + 7, the last two rows' sevens from source blocks (3, 5) and (3, 6) of a 13-wide grid
    assert unequal[0] == [(0, 0, 0, 9), (1, 0, 9, 2), (2, 0, 11, 7), (1, 2, 18, 2), (2, 7, 20, 7), (1, 4, 27, 2), (3, 68, 29, 7), (1, 6, 36, 2), (3, 81, 38, 7)]


def test_every_refusal(ask):
    got = ask([(w, h, p) for _, w, h, p in REFUSED])
    for (name, w, h, pieces), answer in zip(REFUSED, got):
        assert R.runs(pieces, w, h) is None, (name, "the restatement accepts it")
        assert answer is None, (name, "accepted")


def test_one_block_moved_or_resized_refuses_an_accepted_tiling(ask):
    """every accepted small tiling, with one number of one piece changed by one: the header and the restatement agree on each"""
    questions = []
    for name, w, h, pieces in ACCEPTED:
        if len(pieces) > 4 or R.blocks(w) * R.blocks(h) > 200:
            continue
        for k in range(len(pieces)):
            for field in range(8):
                for d in (-1, 1):
                    p = list(pieces[k])
                    p[field] += d
                    if p[field] >= 0:
                        questions.append((w, h, pieces[:k] + [tuple(p)] + pieces[k + 1:]))
    assert len(questions) > 200
    accepted = 0
    for (w, h, pieces), answer in zip(questions, ask(questions)):
        want = R.runs(pieces, w, h)
        assert (answer is None) == (want is None), (w, h, pieces)
        if want is not None:
            accepted += 1
            assert answer[0] == want, (w, h, pieces)
    assert 0 < accepted < len(questions)
