"""limg_amd/csrc/limg_hip_encode_plan.h -- which launch path an 8x8 encode takes or why it is refused, the shape of an image in blocks and strips, the plane set, the
16-byte access flags, the advance of the plane pointers, the chain partition, "a list in one launch pair" -- without a GPU: tests/helpers/encode_plan_check.cpp is built
by the host compiler alone (a program of its own, under the undefined-behaviour sanitizer) and prints the header's answers, which are compared with the rules restated
here.  The helper also answers every plan question from the conditions as they stood in encode_device / encode_params / sub_batch_images / band_count before the
header existed (question `P`): the header, those conditions and this file must agree on every question.

What is enumerated.  The facts are 20 booleans, the plane set and 8 numbers; the product of every value listed for each is beyond 10^9 questions, so it is cut along
what the rules let meet, each part a full product:
  ROUTES  every shape x plane set x chainPhase x batchCount x batch_sub_images x poolThreads x checkpoint_reach on both sides of the shape's need, under each of the
          boolean settings a caller of encode_device makes (and each steering option alone);
  CUBE    every combination of the booleans that take part in a route or a refusal, x plane set, at a single image of whole blocks, a list of them and a
          height-ragged image;
  SIDES   the booleans that only set a flag, the event quota or the band count (float_mode, fitFloatMode, collect_stats, innerLast, dPrevDesc) in every combination
          with what they meet: fitOnly, inner, chainPhase, plane set, poolThreads, ragged_bands and the shapes, with three more that reach the band rules.
A boolean of CUBE never meets chainPhase != 0, poolThreads != 0 or a width-ragged shape in more than the ROUTES settings; that is the cut."""
import itertools
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "helpers", "encode_plan_check.cpp")

SUCCESS, INVALID_PARAMETER, ARGUMENT_NULL = 0, 101, 102  # limg_hip_result (include/limg_hip.h)
NONE, COMPACT, FULL, INVALID = 0, 1, 2, 3
HEIGHT_RAGGED, SUB_BATCHES, FUSED, CHAIN_PHASE2, SPLIT, RAGGED = range(6)
R_NULL, R_SIZE, R_PLANES, R_CHAIN, R_LIST, R_ERROR_FACTORS, ACCEPTED = range(7)

FACTS = ["nullArgument", "sizeX", "sizeY", "planes", "callerRecords", "callerShifts", "recordsAligned", "poolThreads", "fast", "chainPhase", "batchCount", "inner", "innerLast",
         "fitOnly", "fitFloatMode", "streamRaw", "stripWords", "errorFactors", "ratedTable", "dPrevDesc", "force_split_kernels", "legacy_float_stage", "dither_pcg", "float_mode",
         "collect_stats", "batch_sub_images", "ragged_bands", "whole_image_ragged", "checkpoint_reach"]
PLAIN = dict.fromkeys(FACTS, 0)
PLAIN.update(sizeX=264, sizeY=24, planes=FULL, fast=1, batchCount=1, checkpoint_reach=1 << 40)

SHAPES = [(264, 24), (264, 20), (261, 24), (8, 8), (8, 20), (3, 3)]  # whole, height-ragged, width-ragged, one block, sizeY > 8 with one block column, smaller than a block
BAND_SHAPES = [(261, 40), (261, 520), (264, 516)]  # 33 x 5 blocks; 33 x 65: bands without being asked; the last one height-ragged


def build(tmp, opt):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("needs g++")
    exe = str(tmp / ("encode_plan_check" + opt))
    subprocess.check_call([gxx, "-std=c++17", opt, "-Wall", "-Werror", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-static-libubsan", SRC, "-o", exe])

    def run(questions):
        """one answer line (a string) per question"""
        r = subprocess.run([exe], input="\n".join(questions) + "\n", stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
        assert r.returncode == 0, (r.returncode, r.stdout[-2000:])
        lines = r.stdout.split("\n")[:-1]
        assert len(lines) == len(questions), (len(lines), len(questions))
        return lines

    return run


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    return build(tmp_path_factory.mktemp("plan"), "-O1")


def partition(size_y, pool):
    """tests/test_host.py::test_partition_rule's restatement (src/limg.cpp:2114-2134): (chains, block rows of each but the last)"""
    if pool <= 0:
        return 1, 0
    for threads in (pool * 4, pool):
        rows = (size_y // 8) // threads
        if rows:
            return threads, rows
    return 1, 0


def shape(x, y):
    bx, by = -(-x // 8), -(-y // 8)
    sx = -(-bx // 32)
    return bx, by, sx, bx * by, sx * by, int(0 < x <= 0x7FFFFFF8 and 0 < y <= 0x7FFFFFF8), int(x % 8 == 0 and y % 8 == 0)


def restated(f):
    """the issue's rules 1 .. 14 -> the helper's `p` line as a tuple; refused: (code, verdict, -1, 0 ...)"""
    def refused(code, verdict):
        return (code, verdict, -1) + (0,) * 12
    if f["nullArgument"]:
        return refused(ARGUMENT_NULL, R_NULL)                                                     # 1
    x, y = f["sizeX"], f["sizeY"]
    bx, by, _, blocks, _, valid, whole = shape(x, y)
    if not valid:
        return refused(INVALID_PARAMETER, R_SIZE)                                                 # 2
    if f["planes"] == INVALID:
        return refused(ARGUMENT_NULL, R_PLANES)                                                   # 3
    stored, full, ragged = f["planes"] != NONE, f["planes"] != COMPACT, not whole
    cp, n = f["chainPhase"], f["batchCount"]
    if (x % 8 == 0 and y % 8 != 0 and y > 8 and stored and cp == 0 and n == 1 and not f["inner"] and not f["fitOnly"] and not f["force_split_kernels"]
            and not f["legacy_float_stage"] and not f["dither_pcg"] and not f["whole_image_ragged"] and blocks * 3 <= f["checkpoint_reach"]):
        return (SUCCESS, ACCEPTED, HEIGHT_RAGGED, 0, 0, 0, 0, 0, 0, int(f["collect_stats"] != 0), 0, 0, 0, 0, 1)  # 4
    if cp != 0 and (ragged or not stored or f["poolThreads"] != 0):
        return refused(INVALID_PARAMETER, R_CHAIN)                                                # 5
    prefit = not ragged and not f["legacy_float_stage"] and (not f["callerRecords"] or bool(f["recordsAligned"]))  # 6
    fused = stored and not ragged and (not f["force_split_kernels"] or n > 1) and cp == 0          # 7
    want_stats = bool(f["collect_stats"]) and stored and cp == 0                                  # 8
    float_fast = f["float_mode"] == 1 and (not f["fitOnly"] or bool(f["fitFloatMode"]))           # 9
    fit_only = bool(f["fitOnly"]) and not stored
    stream_list = not full and f["streamRaw"] and f["stripWords"] and f["callerRecords"] and f["callerShifts"]
    if n > 1:                                                                                     # 10
        fit_list = fit_only and prefit and whole and cp == 0
        plane_list = fused and prefit and (full or stream_list)
        if not fit_list and not plane_list:
            return refused(INVALID_PARAMETER, R_LIST)
    if f["errorFactors"] and not (f["ratedTable"] and n > 1 and stream_list and fused and prefit and f["fast"] and cp == 0):  # 11
        return refused(INVALID_PARAMETER, R_ERROR_FACTORS)
    sub = 0
    if fused and prefit and n > 1:                                                                # 12
        opt = f["batch_sub_images"]
        sub = opt if opt > 0 else ((8 if n >= 32 else 4 if n >= 16 else 0) if opt == 0 else 0)
        if sub >= n:
            sub = 0
    bands = rows = 0
    if sub:                                                                                       # 13
        path = SUB_BATCHES
    elif fused:
        path = FUSED
    elif cp == 2:
        path = CHAIN_PHASE2
    elif not ragged:
        path = SPLIT
    else:
        path = RAGGED                                                                             # 14
        chains = partition(y, f["poolThreads"])[0]
        want = f["ragged_bands"]
        bands = 1
        if stored and not f["dPrevDesc"] and chains <= 1 and want >= 0 and bx >= 2 and by >= 2 and (want > 0 or (bx >= 32 and by >= 64)):
            bands = want if want > 0 else 16
        bands = min(bands, max(by // 2, 1), 64)
        rows = -(-by // bands)
        bands = -(-by // rows)
    marks = 2 if cp != 0 else 4 if not f["inner"] else 0 if f["innerLast"] else 3
    return (SUCCESS, ACCEPTED, path, sub, bands, rows, int(prefit), int(fused), int(float_fast), int(want_stats), int(full), int(stored), int(f["streamRaw"] and not full),
            int(fit_only), marks)


def need(shape_xy):
    """dither calls the height-ragged route asks the embedded checkpoints to reach"""
    return shape(*shape_xy)[3] * 3


def settings():
    """the boolean settings of ROUTES: what the callers of encode_device set (limg_hip_encode.hip, limg_hip_stream_encode_api.hip, limg_hip_blocked_api.hip), then each option alone"""
    stream = dict(streamRaw=1, stripWords=1, callerRecords=1, callerShifts=1, recordsAligned=1)
    yield {}                                                               # the plain call
    yield dict(fast=0)
    yield stream                                                           # a stream encode, single or as a list
    yield dict(stream, stripWords=0)                                       # ... without the strip form
    yield dict(stream, recordsAligned=0)
    yield dict(stream, errorFactors=1, ratedTable=1)                       # a list with one error factor per image
    yield dict(stream, errorFactors=1, ratedTable=1, fast=0)
    yield dict(stream, errorFactors=1)
    yield dict(fitOnly=1, fitFloatMode=1)                                  # the size probes' records
    yield dict(fitOnly=1)                                                  # pass 1 of the merged-block encoder
    yield dict(inner=1)                                                    # the two parts of a height-ragged image
    yield dict(inner=1, innerLast=1, dPrevDesc=1)
    for option in ("force_split_kernels", "legacy_float_stage", "dither_pcg", "whole_image_ragged"):
        yield {option: 1}


def questions():
    out = []

    def add(**changed):
        f = dict(PLAIN)
        f.update(changed)
        out.append(f)

    # ROUTES
    for setting in settings():
        for (x, y), planes, cp, n, sub, pool, short in itertools.product(SHAPES, (NONE, COMPACT, FULL), (0, 1, 2), (1, 2, 15, 16, 31, 32), (-1, 0, 1, 4), (0, 2), (0, 1)):
            add(sizeX=x, sizeY=y, planes=planes, chainPhase=cp, batchCount=n, batch_sub_images=sub, poolThreads=pool, checkpoint_reach=need((x, y)) - short, **setting)
    # CUBE
    cube = ["callerRecords", "callerShifts", "recordsAligned", "fast", "inner", "fitOnly", "streamRaw", "stripWords", "errorFactors", "ratedTable", "force_split_kernels",
            "legacy_float_stage", "dither_pcg", "whole_image_ragged"]
    for bits in itertools.product((0, 1), repeat=len(cube)):
        setting = dict(zip(cube, bits))
        for planes in (NONE, COMPACT, FULL):
            add(planes=planes, **setting)
            add(planes=planes, batchCount=2, **setting)
            add(planes=planes, sizeY=20, checkpoint_reach=need((264, 20)), **setting)
    # SIDES
    sides = ["float_mode", "fitFloatMode", "collect_stats", "innerLast", "dPrevDesc", "fitOnly", "inner"]
    for bits in itertools.product((0, 1), repeat=len(sides)):
        setting = dict(zip(sides, bits))
        for (x, y), planes, cp, pool, bands in itertools.product(SHAPES + BAND_SHAPES, (NONE, COMPACT, FULL), (0, 1, 2), (0, 2), (-1, 0, 2, 100)):
            add(sizeX=x, sizeY=y, planes=planes, chainPhase=cp, poolThreads=pool, ragged_bands=bands, **setting)
    # rules 1 .. 3 in their order: each alone, then with the one behind it
    for null, size, planes in itertools.product((0, 1), ((264, 24), (0, 24), (264, 0), (0x7FFFFFF8, 8), (0x7FFFFFF9, 8), (8, 0x7FFFFFF9)), (NONE, COMPACT, FULL, INVALID)):
        add(nullArgument=null, sizeX=size[0], sizeY=size[1], planes=planes)
        add(nullArgument=null, sizeX=size[0], sizeY=size[1], planes=planes, chainPhase=1, poolThreads=2)
    return out


@pytest.fixture(scope="module")
def asked():
    qs = questions()
    return qs, [" ".join([str(f[k]) for k in FACTS]) for f in qs]


def test_plan(ask, asked):
    qs, lines = asked
    want = [" ".join(map(str, restated(f))) for f in qs]
    got = ask(["p " + line for line in lines])
    wrong = [(line, w, g) for line, w, g in zip(lines, want, got) if w != g]
    assert not wrong, (len(wrong), wrong[:5])
    # every path, every refusal and every event quota is among the answers
    answers = set(tuple(int(v) for v in w.split()) for w in set(want))
    assert {a[2] for a in answers} == {-1, HEIGHT_RAGGED, SUB_BATCHES, FUSED, CHAIN_PHASE2, SPLIT, RAGGED}
    assert {a[1] for a in answers} == {R_NULL, R_SIZE, R_PLANES, R_CHAIN, R_LIST, R_ERROR_FACTORS, ACCEPTED}
    assert {a[14] for a in answers if a[1] == ACCEPTED} == {0, 1, 2, 3, 4}
    assert {a[3] for a in answers} == {0, 1, 4, 8} and {a[4] for a in answers} >= {0, 1, 2, 13}


def test_plan_is_the_old_conditions(ask, asked):
    """the conditions encode_device and what it called were made of, lifted into the helper: the same answers (they had no word for the verdict)"""
    qs, lines = asked
    want = [" ".join(map(str, [a for i, a in enumerate(restated(f)) if i != 1])) for f in qs]
    got = ask(["P " + line for line in lines])
    wrong = [(line, w, g) for line, w, g in zip(lines, want, got) if w != g]
    assert not wrong, (len(wrong), wrong[:5])


def test_plan_unoptimised(tmp_path, asked):
    """the helper at -O0: what the sanitizer sees does not depend on the optimiser"""
    qs, lines = asked
    run = build(tmp_path, "-O0")
    step = 7  # (a seventh of the questions: every seventh, so all three parts)
    assert run(["p " + line for line in lines[::step]]) == [" ".join(map(str, restated(f))) for f in qs[::step]]


def test_named_calls(ask):
    """the calls the GPU suite makes, by name: what each is expected to become"""
    def one(**changed):
        f = dict(PLAIN)
        f.update(changed)
        (line,) = ask(["p " + " ".join(str(f[k]) for k in FACTS)])
        got = tuple(int(v) for v in line.split())
        assert got == restated(f)
        return got
    assert one()[2] == FUSED and one()[6] == 1 and one()[14] == 4
    assert one(legacy_float_stage=1)[2] == FUSED and one(legacy_float_stage=1)[6] == 0
    assert one(force_split_kernels=1)[2] == SPLIT
    assert one(planes=NONE)[2] == SPLIT
    assert one(sizeX=261)[2:6] == (RAGGED, 0, 1, 3)
    assert one(sizeX=261, sizeY=40, ragged_bands=2)[2:6] == (RAGGED, 0, 2, 3)
    assert one(sizeX=261, sizeY=520)[2:6] == (RAGGED, 0, 13, 5), "16 bands asked for 65 block rows: 5 rows each make 13"
    assert one(sizeY=20)[2] == HEIGHT_RAGGED and one(sizeY=20)[14] == 1
    assert one(sizeY=20, checkpoint_reach=need((264, 20)) - 1)[2] == RAGGED
    assert one(sizeY=16, inner=1)[14] == 3 and one(sizeY=4, inner=1, innerLast=1)[14] == 0
    assert one(batchCount=2)[2] == FUSED and one(batchCount=3, batch_sub_images=1)[2:4] == (SUB_BATCHES, 1)
    assert one(batchCount=32)[2:4] == (SUB_BATCHES, 8) and one(batchCount=16)[2:4] == (SUB_BATCHES, 4) and one(batchCount=15)[2] == FUSED
    assert one(batchCount=32, batch_sub_images=-1)[2] == FUSED
    assert one(chainPhase=1)[2] == SPLIT and one(chainPhase=2)[2] == CHAIN_PHASE2 and one(chainPhase=1)[14] == 2
    assert one(chainPhase=1, poolThreads=2)[:2] == (INVALID_PARAMETER, R_CHAIN)
    assert one(batchCount=2, planes=COMPACT)[:2] == (INVALID_PARAMETER, R_LIST)
    assert one(batchCount=2, sizeX=261)[:2] == (INVALID_PARAMETER, R_LIST)
    assert one(batchCount=2, planes=NONE, fitOnly=1)[2] == SPLIT, "the probes' records of a list"


def test_shape_and_list_rule(ask):
    sizes = [1, 3, 7, 8, 9, 255, 256, 257, 261, 264, 8192, 0x7FFFFFF8, 0x7FFFFFF9, 0]
    pairs = list(itertools.product(sizes, sizes))
    got = ask(["e %d %d" % p for p in pairs])
    assert got == [" ".join(map(str, shape(*p))) for p in pairs]
    cases = list(itertools.product(SHAPES, (0, 1), (0, 1)))
    got = ask(["l %d %d %d %d" % (x, y, fs, lf) for (x, y), fs, lf in cases])
    assert got == [str(int(x % 8 == 0 and y % 8 == 0 and not fs and not lf)) for (x, y), fs, lf in cases]


def test_plane_set(ask):
    """all 2^11 NULL patterns: the three factor planes (bits 8 .. 10) are required, the eight word planes are all there or all absent"""
    got = ask(["s %d" % m for m in range(1 << 11)])
    for m, g in enumerate(got):
        words, factors = m & 0xFF, m >> 8
        want = INVALID if factors != 7 or words not in (0, 0xFF) else (FULL if words else COMPACT)
        assert int(g) == want, m
    assert [int(got[m]) for m in (0x7FF, 0x700, 0, 0xFF)] == [FULL, COMPACT, INVALID, INVALID]


def test_vec_access(ask):
    """16-byte access: the width in pixels and every pointer concerned; 8-byte access to the factor planes from multiples of 8"""
    offsets, widths = (0, 4, 8, 16), (4, 8, 12, 16, 17)
    cases = []
    for width, full, info in itertools.product(widths, (0, 1), (0, 1)):
        cases.append((width, full, info, [0] * 12))
        for k, off in itertools.product(range(12), offsets[1:]):  # one pointer off
            cases.append((width, full, info, [off if i == k else 0 for i in range(12)]))
        for off in offsets[1:]:  # all of them off
            cases.append((width, full, info, [off] * 12))
    got = ask(["v %d %d %d %s" % (w, full, info, " ".join(map(str, o))) for w, full, info, o in cases])
    for (w, full, info, o), g in zip(cases, got):
        word_planes, decoded, factors = o[2:9], o[1], o[9:12]
        want = (w % 4 == 0 and o[0] % 16 == 0,
                bool(info and full) and w % 4 == 0 and all(v % 16 == 0 for v in word_planes),
                bool(info) and w % 8 == 0 and all(v % 8 == 0 for v in factors),
                bool(info and full) and w % 4 == 0 and decoded % 16 == 0,
                bool(info) and w % 16 == 0 and all(v % 16 == 0 for v in factors))
        assert g == " ".join(str(int(v)) for v in want), (w, full, info, o)


def test_advance_planes(ask):
    masks = [0x7FF, 0x700, 0x701, 0x0FF, 0, 0x400, 0x2AA]
    cases = list(itertools.product(masks, (0, 1, 5, 64)))
    got = ask(["a %d %d" % c for c in cases])
    for (mask, pixels), g in zip(cases, got):
        want = [(pixels * (4 if i < 8 else 1)) if mask >> i & 1 else -1 for i in range(11)]
        assert g == " ".join(map(str, want)), (mask, pixels)


def test_partition(ask):
    """the cases of tests/test_host.py::test_partition_rule"""
    cases = [(8192, 0), (8192, 2), (618, 8), (200, 2), (64, 3), (24, 8), (8, 1), (1000, 7)]
    cases += [(y, t) for y in (8, 16, 64, 100, 512, 4096) for t in (0, 1, 2, 3, 4, 16, 64)]
    got = ask(["n %d %d" % c for c in cases])
    assert got == ["%d %d" % partition(*c) for c in cases]
