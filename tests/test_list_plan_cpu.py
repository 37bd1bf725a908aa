"""limg_amd/csrc/limg_hip_list_plan.h -- the layout of a stream-encode list of mixed shapes: per image its blocks, strips, float-stage units and where each starts,
its OWN 16-byte access flags and dither-chain partition; per chunk the totals, the noise need (the maximum over the images, not the sum), the chunk boundaries and
eligibility; the layout of a chunk's table block and what a list grows before its first launch -- without a GPU: tests/helpers/list_plan_check.cpp is built by
the host compiler alone (under the undefined-behaviour sanitizer) and prints the header's answers, which are compared with the rules restated here on the lists
tests/test_gpu_stream_list.py encodes."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "helpers", "list_plan_check.cpp")

LISTS = {
    "edges": ((264, 24), (8, 8), (256, 8), (520, 16), (8, 512), (24, 40), (512, 32)),
    "one_strip_each": ((256, 8), (8, 8), (248, 8), (16, 8), (256, 8)),
    "scan_slices": ((256, 32), (512, 16), (256, 24), (1024, 8), (8, 8), (512, 32)),
    "rgb": ((512, 32), (40, 24), (264, 8)),
    "pool": ((128, 256), (64, 24), (8, 8), (256, 40)),
    "ragged_inside": ((264, 24), (13, 9), (256, 20), (8, 8)),
}
VEC_IN, VEC_PLANES, VEC_FACTORS8, VEC_DECODED, VEC_FACTORS = 1, 2, 4, 8, 16


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("needs g++")
    exe = str(tmp_path_factory.mktemp("list_plan") / "list_plan_check")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-static-libubsan", SRC, "-o", exe])

    def run(questions):
        r = subprocess.run([exe], input="\n".join(questions) + "\n", stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
        assert r.returncode == 0, (r.returncode, r.stdout[-2000:])
        lines = r.stdout.split("\n")[:-1]
        assert len(lines) == len(questions), (len(lines), len(questions))
        return lines

    return run


def partition(size_y, pool):
    """src/limg.cpp:2114-2134 in block rows: (chains, block rows of each but the last)"""
    if pool <= 0:
        return 1, 0
    for threads in (pool * 4, pool):
        rows = (size_y // 8) // threads
        if rows:
            return threads, rows
    return 1, 0


def restate(shapes, pool, aligns):
    """what the header must say of the chunk made of `shapes` (aligns: per image the offsets of its input and of its factor planes from a 16-byte boundary)"""
    per, blocks, strips, units, noise, vec_all = [], 0, 0, 0, 0, True
    for (w, h), (ia, fa) in zip(shapes, aligns):
        bx, by = (w + 7) // 8, (h + 7) // 8
        sx = (bx + 31) // 32
        chains, rows = partition(h, pool)
        vec = (VEC_IN if w % 4 == 0 and ia % 16 == 0 else 0) | (VEC_FACTORS8 if w % 8 == 0 and fa % 8 == 0 else 0) | (VEC_FACTORS if w % 16 == 0 and fa % 16 == 0 else 0)
        per.append((blocks, strips, sx * by, units, bx, by, sx, bx * by, chains, rows, vec))
        longest = by if chains <= 1 or (chains - 1) * rows >= by else by - (chains - 1) * rows
        noise = max(noise, longest * bx * 3)
        vec_all = vec_all and bool(vec & VEC_IN)
        blocks += bx * by
        strips += sx * by
        units += ((bx + 63) // 64) * by
    return per, (blocks, strips, units, noise, int(vec_all))


def parse(line, n):
    left, right = line.split("|")
    v = [int(x) for x in left.split()]
    assert len(v) == 11 * n, line
    return [tuple(v[11 * i:11 * i + 11]) for i in range(n)], tuple(int(x) for x in right.split())


@pytest.mark.parametrize("name", sorted(LISTS))
def test_layout(ask, name):
    """prefixes, per-image flags and chainRows: aligned pointers, then image 1's input 4 bytes and image 2's factor planes 8 bytes off a 16-byte boundary; with and
    without a thread pool; the list, reversed and rotated by one"""
    shapes = LISTS[name]
    n = len(shapes)
    questions, wants = [], []
    for order in (list(range(n)), list(range(n))[::-1], [(i + 1) % n for i in range(n)]):
        for pool in (0, 2, 3):
            for aligns in ([(0, 0)] * n, [(4 if i == 1 else 0, 8 if i == 2 else 0) for i in range(n)]):
                sh = [shapes[i] for i in order]
                questions.append("L %d %d " % (pool, n) + " ".join("%d %d %d %d" % (w, h, ia, fa) for (w, h), (ia, fa) in zip(sh, aligns)))
                wants.append(restate(sh, pool, aligns))
    for q, line, want in zip(questions, ask(questions), wants):
        assert parse(line, n) == want, q


def test_flags_are_per_image(ask):
    """264 (no multiple of 16) beside 256: today's list takes the & over the list, which would deny the second image its 16-byte factor accesses"""
    per, _ = parse(ask(["L 0 2 264 24 0 0 256 8 0 0"])[0], 2)
    assert per[0][10] == VEC_IN | VEC_FACTORS8 and per[1][10] == VEC_IN | VEC_FACTORS8 | VEC_FACTORS


def test_noise_need_is_the_maximum(ask):
    """every image starts its own chains: the table must reach the longest chain of any image, not the sum over the images; a pool shortens an image's chains"""
    _, tot = parse(ask(["L 0 3 128 256 0 0 64 24 0 0 256 40 0 0"])[0], 3)
    assert tot[3] == 16 * 32 * 3 and tot[3] < (16 * 32 + 8 * 3 + 32 * 5) * 3
    _, tot = parse(ask(["L 2 3 128 256 0 0 64 24 0 0 256 40 0 0"])[0], 3)
    # pool 2: 128 x 256 has 8 chains of 4 block rows (16 x 4 blocks); 256 x 40 (5 block rows) has 2 chains of 2 rows, the last takes 3 (32 x 3 blocks)
    assert tot[3] == max(16 * 4, 8 * 2, 32 * 3) * 3  # (64 x 24: 2 chains of 1 block row, the last takes 2)


def test_pool_list_partitions(ask):
    """`pool`: chainRows differs per image, and 8 x 8 has fewer block rows than chains (one chain)"""
    per, _ = parse(ask(["L 2 4 128 256 0 0 64 24 0 0 8 8 0 0 256 40 0 0"])[0], 4)
    assert [(p[8], p[9]) for p in per] == [(8, 4), (2, 1), (1, 0), (2, 2)]


def test_eligibility(ask):
    cases = [((w, h, fast, split, legacy), int(w % 8 == 0 and h % 8 == 0 and w > 0 and h > 0 and fast and not split and not legacy))
             for (w, h) in ((264, 24), (13, 9), (256, 20), (8, 8), (261, 24), (0, 8), (8, 0)) for fast in (0, 1) for split in (0, 1) for legacy in (0, 1)]
    got = ask(["E %d %d %d %d %d" % c for c, _ in cases])
    assert [int(g) for g in got] == [w for _, w in cases]
    assert [int(g) for g in ask(["E %d 8 1 0 0" % (1 << 31), "E %d 8 1 0 0" % 0x7FFFFFF8])] == [0, 1]


def chunk_ends(blocks, strips, hook):
    ends, i0, n = [], 0, len(blocks)
    while i0 < n:
        b = s = 0
        i = i0
        while i < n:
            if hook and i - i0 >= hook:
                break
            if i > i0 and (b + blocks[i] > (1 << 30) // 64 or s + strips[i] > 0x7FFFFFFF):
                break
            b += blocks[i]
            s += strips[i]
            i += 1
        ends.append(i)
        i0 = i
    return ends


def test_chunk_boundaries(ask):
    """a forced chunk size; the 1 GiB of block records (2^24 blocks); the 32-bit strip limit -- with synthetic counts and no memory; an image that alone is over
    a limit is a chunk of its own"""
    M = (1 << 30) // 64
    cases = [
        (3, [10] * 7, [2] * 7),
        (3, [1] * 66, [1] * 66),
        (0, [M // 2, M // 2, 1, M, 1, M + 5, 1], [1] * 7),
        (0, [1] * 5, [0x7FFFFFFF - 1, 1, 1, 0x7FFFFFFF, 1]),
        (0, [1] * 4, [0x40000000] * 4),
        (2, [M, 1, 1, 1], [1, 0x7FFFFFFF, 1, 1]),
        (0, [5], [5]),
    ]
    got = ask(["C %d %d " % (hook, len(b)) + " ".join("%d %d" % p for p in zip(b, s)) for hook, b, s in cases])
    for line, (hook, b, s) in zip(got, cases):
        ends = [int(x) for x in line.split()]
        assert ends == chunk_ends(b, s, hook), (hook, b, s, line)
        assert ends[-1] == len(b) and all(e1 > e0 for e0, e1 in zip([0] + ends, ends))
    assert [int(x) for x in got[0].split()] == [3, 6, 7] and [int(x) for x in got[2].split()] == [2, 3, 4, 5, 6, 7] and [int(x) for x in got[3].split()] == [2, 3, 4, 5]


ENTRY_SIZES = (160, 64, 96, 32, 32, 4, 4)  # view, ListImage, ImageIO, RatedImage, StreamImage, two prefix words (limg_hip_context.h asserts each sizeof)


def test_table_layout(ask):
    """a chunk's table block with the real entry sizes: every part starts on a 16-byte boundary, no two parts overlap, `bytes` covers them all"""
    ns = (1, 2, 3, 64, 65)
    got = ask(["T %d " % n + " ".join(str(e) for e in ENTRY_SIZES) for n in ns])
    for n, line in zip(ns, got):
        v = [int(x) for x in line.split()]
        assert len(v) == 8, line
        offsets, total = v[:7], v[7]
        assert all(o % 16 == 0 for o in offsets) and total % 16 == 0, (n, line)
        spans = sorted((o, o + n * e) for o, e in zip(offsets, ENTRY_SIZES))
        assert spans[0][0] == 0 and all(a1 <= b0 for (_, a1), (b0, _) in zip(spans, spans[1:])), (n, spans)
        assert spans[-1][1] <= total < spans[-1][1] + 16, (n, spans, total)
        assert offsets == sorted(offsets), (n, line)  # the order the device code is given: views, images, io, rated, streams, the prefix words


def needs(blocks, strips, fac, hook):
    """the largest chunk of more than one image, member by member"""
    most, i0 = [0, 0, 0, 0], 0
    for i1 in chunk_ends(blocks, strips, hook):
        if i1 - i0 > 1:
            most = [max(most[0], i1 - i0), max(most[1], sum(blocks[i0:i1])), max(most[2], sum(strips[i0:i1])), max(most[3], sum(fac[i0:i1]))]
        i0 = i1
    return tuple(most)


def test_needs(ask):
    """what a list grows before its first launch: on the `edges` and `sixty_six` lists of tests/test_gpu_stream_list.py, whole and in chunks of three, and on a
    synthetic list whose chunks break on the 1 GiB of block records (the members' maxima come from different chunks)"""
    small = ((264, 24), (8, 8), (256, 8), (24, 40), (512, 32))
    cases = []
    for shapes in (LISTS["edges"], tuple(small[i % 5] for i in range(66))):
        planes = [int(x) for x in ask(["P %d %d" % s for s in shapes])]
        assert planes == [(w * h + 255) // 256 * 256 for w, h in shapes]
        blocks = [(w // 8) * (h // 8) for w, h in shapes]
        strips = [((w // 8 + 31) // 32) * (h // 8) for w, h in shapes]
        for hook in (0, 3):
            cases.append((hook, blocks, strips, [3 * p for p in planes]))
    M = (1 << 30) // 64
    cases.append((0, [M // 2, M // 2, 1, M, 1, M + 5, 1, 1, 1], [70, 70, 1, 1, 1, 1, 9, 9, 1], [100, 100, 1, 1, 1, 1, 50, 50, 200]))
    cases.append((1, [4, 4, 4], [1, 1, 1], [256, 256, 256]))  # every chunk one image: nothing to grow
    got = ask(["N %d %d " % (hook, len(b)) + " ".join("%d %d %d" % t for t in zip(b, s, f)) for hook, b, s, f in cases])
    for line, (hook, b, s, f) in zip(got, cases):
        assert tuple(int(x) for x in line.split()) == needs(b, s, f, hook), (hook, b, s, f, line)
    assert got[0].split()[0] == "7" and got[1].split()[0] == "3" and got[2].split()[0] == "66" and got[3].split()[0] == "3"
    assert [int(x) for x in got[4].split()] == [3, M, 140, 300] and got[5].split() == ["0"] * 4
