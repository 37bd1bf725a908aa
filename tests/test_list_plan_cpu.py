"""limg_amd/csrc/limg_hip_list_plan.h -- the layout of a stream-encode list of mixed shapes: per image its blocks, strips, float-stage units and where each starts,
its OWN 16-byte access flags and dither-chain partition; per chunk the totals, the noise need (the maximum over the images, not the sum), the chunk boundaries and
eligibility; the layout of a chunk's table block and what a list grows before its first launch -- without a GPU: tests/helpers/list_plan_check.cpp is built by
the host compiler alone (under the undefined-behaviour sanitizer) and prints the header's answers, which are compared with the rules restated here on the lists
tests/test_gpu_stream_list.py encodes.

The ROUTE of every list entry of the stream encode family (list_route: which items go through which launches, in which order, what restarts the statistics, what the
largest chunk needs) is asked three times: the header's plan, the decisions of the five walkers as they stood before the plan (lifted into the helper), and the rules
restated in route() below.  All three agree on every list of one to four of five shapes under every option, hook, job and entry form that exists: there is no
same-shape entry for the sizes and no items entry at a shared factor, so those two combinations are not asked."""
import itertools
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


# ---- the route ----
SHARED, OWN, BUDGET, SIZES = 0, 1, 2, 3
ROUTE_SHAPES = ((8, 8), (256, 8), (264, 24), (13, 9), (256, 20))


def _blocks(shape):
    return ((shape[0] + 7) // 8) * ((shape[1] + 7) // 8)


def _strips(shape):
    return (((shape[0] + 7) // 8 + 31) // 32) * ((shape[1] + 7) // 8)


def list_chunk(blocks, strips, hook):
    chunk = (1 << 30) // (blocks * 64)
    if chunk * strips > 0x7FFFFFFF:
        chunk = 0x7FFFFFFF // strips
    if hook:
        chunk = min(chunk, hook)
    return max(chunk, 1)


def route(shapes, efs, job, same, fast, split, legacy, hook):
    """the rules, restated: -> (steps [(kind, own, restart, item indices)], most (images, blocks, strips, facBytes), inPlace)"""
    steps = []
    encode = job in (SHARED, OWN)

    def pair(idx):
        w, h = shapes[idx[0]]
        return w % 8 == 0 and h % 8 == 0 and not split and not legacy

    def chunk_of(idx):
        return list_chunk(_blocks(shapes[idx[0]]), _strips(shapes[idx[0]]), hook)

    def cut(idx, chunk, own, restart):
        for i0 in range(0, len(idx), chunk):
            part = tuple(idx[i0:i0 + chunk])
            steps.append(("S", False, restart, part) if len(part) == 1 else ("C", own, restart, part))
            restart = False

    def same_shape(idx, own, restart):
        """-> cut in list order by the chunk rule"""
        pairs = len(idx) > 1 and pair(idx)
        if own and (not pairs or not fast):
            for _, group in itertools.groupby(sorted(idx, key=lambda i: efs[i]), key=lambda i: efs[i]):  # (sorted is stable)
                same_shape(list(group), False, True)
            return False
        cut(idx, chunk_of(idx) if pairs else 1, own, restart)
        return pairs

    def budget_same(idx):
        cut(idx, chunk_of(idx) if len(idx) > 1 and pair(idx) and fast else 1, False, not steps)

    in_place = False
    everything = list(range(len(shapes)))
    if same:
        if job == BUDGET:
            budget_same(everything)
        else:
            in_place = same_shape(everything, job == OWN, True)
    else:
        eligible = [i for i in everything if fast and pair([i])]
        others = [i for i in everything if i not in eligible]
        if len(eligible) == 1:
            steps.append(("S", False, True, (eligible[0],)))
        elif eligible and job != SIZES and len({shapes[i] for i in eligible}) == 1:
            if job == BUDGET:
                budget_same(eligible)
            else:
                same_shape(eligible, True, True)
        elif eligible:
            i0 = 0
            for i1 in chunk_ends([_blocks(shapes[i]) for i in eligible], [_strips(shapes[i]) for i in eligible], hook):
                part = tuple(eligible[i0:i1])
                steps.append(("S" if len(part) == 1 else "M", True, not steps, part))
                i0 = i1
        for i in others:
            steps.append(("S", False, not steps, (i,)))
    most = [0, 0, 0, 0]
    for _, _, _, part in steps:
        if len(part) > 1:
            need = (len(part), sum(_blocks(shapes[i]) for i in part), sum(_strips(shapes[i]) for i in part),
                    sum(3 * ((shapes[i][0] * shapes[i][1] + 255) // 256 * 256) for i in part) if encode else 0)
            most = [max(a, b) for a, b in zip(most, need)]
    return steps, tuple(most), in_place


def route_line(shapes, efs, job, same, fast, split, legacy, hook):
    steps, most, in_place = route(shapes, efs, job, same, fast, split, legacy, hook)
    text = "".join("%s%s%s %s;" % ("!" if restart and job in (SHARED, OWN) else "", kind, int(own) if kind == "C" else "", " ".join(str(i) for i in part))
                   for kind, own, restart, part in steps)
    return "%s | %d %d %d %d | %d" % ((text,) + most + (int(in_place),))


def route_question(shapes, efs, job, same, fast, split, legacy, hook):
    return "%d %d %d %d %d %d %d " % (job, same, fast, split, legacy, hook, len(shapes)) + " ".join("%d %d %d" % (w, h, ef) for (w, h), ef in zip(shapes, efs))


def factor_patterns(n):
    """all equal, the first two equal, all distinct"""
    return sorted({(100,) * n, ((100, 100, 40, 20)[:n]), ((100, 40, 20, 60)[:n])})


def route_cases():
    for n in (1, 2, 3, 4):
        for shapes in itertools.product(ROUTE_SHAPES, repeat=n):
            forms = [(False, OWN, p) for p in factor_patterns(n)] + [(False, BUDGET, (0,) * n), (False, SIZES, (0,) * n)]
            if len(set(shapes)) == 1:
                forms += [(True, SHARED, (100,) * n), (True, BUDGET, (0,) * n)] + [(True, OWN, p) for p in factor_patterns(n)]
            for same, job, efs in forms:
                for fast, split, legacy in itertools.product((0, 1), repeat=3):
                    for hook in (0, 1, 2, 3):
                        yield shapes, efs, job, int(same), fast, split, legacy, hook


def test_route_three_ways(ask):
    """the header's plan = the walkers' decisions as they stood = the rules restated here, on every question"""
    cases = list(route_cases())
    assert len({c[0] for c in cases}) == 780 and len(cases) > 100000
    new = ask(["R " + route_question(*c) for c in cases])
    old = ask(["O " + route_question(*c) for c in cases])
    for c, a, b in zip(cases, new, old):
        assert a == b == route_line(*c), (c, a, b, route_line(*c))


def _steps(line):
    return line.split(" |")[0]


def test_route_named_lists(ask):
    """the lists tests/test_gpu_stream_list.py encodes, whole and in chunks of three, for every job of the items entries -- and what a reader expects of them"""
    cases = [(LISTS[name], tuple(20 + 10 * i for i in range(len(LISTS[name]))), job, 0, 1, 0, 0, hook)
             for name in ("edges", "ragged_inside", "one_strip_each") for job in (OWN, BUDGET, SIZES) for hook in (0, 3)]
    new = ask(["R " + route_question(*c) for c in cases])
    old = ask(["O " + route_question(*c) for c in cases])
    for c, a, b in zip(cases, new, old):
        assert a == b == route_line(*c), (c, a, b, route_line(*c))
    got = {(name, job, hook): _steps(line) for (name, job, hook), line in
           zip([(name, job, hook) for name in ("edges", "ragged_inside", "one_strip_each") for job in (OWN, BUDGET, SIZES) for hook in (0, 3)], new)}
    assert got[("edges", OWN, 0)] == "!M 0 1 2 3 4 5 6;" and got[("edges", OWN, 3)] == "!M 0 1 2;M 3 4 5;S 6;"
    assert got[("edges", BUDGET, 0)] == got[("edges", SIZES, 0)] == "M 0 1 2 3 4 5 6;" and got[("edges", BUDGET, 3)] == got[("edges", SIZES, 3)] == "M 0 1 2;M 3 4 5;S 6;"
    # one mixed chunk of (264, 24) and (8, 8), then (13, 9) and (256, 20) through the single call, in that order
    assert got[("ragged_inside", OWN, 0)] == got[("ragged_inside", OWN, 3)] == "!M 0 3;S 1;S 2;"
    assert got[("one_strip_each", OWN, 0)] == "!M 0 1 2 3 4;" and got[("one_strip_each", OWN, 3)] == "!M 0 1 2;M 3 4;"


def test_route_same_shape_by_hand(ask):
    """three (264, 24) images: own factors (20, 20, 400) under the accurate search are a shared-factor chunk of the first two, then a single, each with statistics of
    its own; under the default search one own-factor chunk, cut in list order; four at a shared factor in chunks of three: a chunk and a last chunk of one"""
    three = ((264, 24),) * 3
    got = ask(["R " + route_question(three, (20, 20, 400), OWN, 1, 0, 0, 0, 0), "R " + route_question(three, (400, 20, 20), OWN, 1, 0, 0, 0, 0),
               "R " + route_question(three, (20, 20, 400), OWN, 1, 1, 0, 0, 0), "R " + route_question(three, (20, 20, 400), OWN, 1, 1, 1, 0, 0),
               "R " + route_question(((264, 24),) * 4, (100,) * 4, SHARED, 1, 1, 0, 0, 3), "R " + route_question(((264, 24),) * 5, (0,) * 5, BUDGET, 1, 1, 0, 0, 2),
               "R " + route_question(three, (20, 100, 400), OWN, 0, 0, 0, 0, 0)])
    plane = (264 * 24 + 255) // 256 * 256
    assert got[0] == "!C0 0 1;!S 2; | 2 198 12 %d | 0" % (2 * 3 * plane)
    assert _steps(got[1]) == "!C0 1 2;!S 0;"
    assert got[2] == "!C1 0 1 2; | 3 297 18 %d | 1" % (3 * 3 * plane)
    assert _steps(got[3]) == "!S 0;S 1;!S 2;"  # the split path: no launch pair, the group of two is two singles
    assert got[4] == "!C0 0 1 2;S 3; | 3 297 18 %d | 1" % (3 * 3 * plane)
    assert got[5] == "C0 0 1;C0 2 3;S 4; | 2 198 12 0 | 0"
    assert _steps(got[6]) == "!S 0;S 1;S 2;"  # an items entry under the accurate search: nothing is eligible


def test_chunk_rules_agree_on_one_shape(ask):
    """list_chunk(blocks, strips, hook) images at a time = the chunks of list_chunk_end over n equal items, with synthetic counts and no shapes behind them"""
    cases = [(hook, n, b, s) for b in (1, 5, 1 << 23, (1 << 24) - 1, 1 << 24, (1 << 24) + 5) for s in (1, 0x3FFFFFFF, 0x40000000, 0x7FFFFFFF) for hook in (0, 1, 3)
             for n in range(1, 10)]
    by_count = ask(["K %d %d %d %d" % c for c in cases])
    by_end = ask(["C %d %d " % (hook, n) + " ".join(["%d %d" % (b, s)] * n) for hook, n, b, s in cases])
    for (hook, n, b, s), a, e in zip(cases, by_count, by_end):
        chunk = list_chunk(b, s, hook)
        want = [min(i0 + chunk, n) for i0 in range(0, n, chunk)]
        assert [int(x) for x in a.split()] == [int(x) for x in e.split()] == want == chunk_ends([b] * n, [s] * n, hook), (hook, n, b, s, a, e)
