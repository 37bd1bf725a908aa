"""The two shift-search automata as data (tools/make_search_table.py -> limg_search_table.h, limg_search_table_accurate.h -> the library's expansion of the latter,
limg_hip_host_accurate_table): the committed headers are what the generator emits; every state and edge of the expanded table is what the generator says, its edge
masks exactly the factors that change; a model of search_accurate_automaton's walk over the expanded table (root triple, state 0's mask, then only what the edge
masks name) ends where the generator's walk does; and the inputs of tests/test_gpu_search_tables.py (tests/search_table_inputs.py), replayed with the oracle's
trial, reach every class of edges of the accurate automaton and of the default table outside its hot subtree.  CPU only."""
import os
import random
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import search_table_inputs as inputs  # noqa: E402  (puts tools/ on sys.path)
import make_search_table as mst  # noqa: E402

FACTORS = "ABC"


def mask_name(m):
    return "final" if m == "final" else "rebuild " + ("+".join(FACTORS[k] for k in range(3) if m & (1 << k)) or "nothing")


def acc_class_name(c):
    m, phase, ok = c
    return "%s after a %s phase-%d trial" % (mask_name(m), "passing" if ok else "failing", phase)


def default_class_name(c):
    m, ok = c
    return "%s after a %s" % (mask_name(m), "pass" if ok else "fail")


def changed(t, n):
    return sum(1 << k for k in range(3) if t[k] != n[k])


# ---- the tables -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def acc():
    """the accurate automaton: the generator's states, its compact words, the library's expansion, the class of every edge"""
    import limg_amd
    if not os.path.exists(limg_amd.LIB_PATH):
        from limg_amd import build
        build.build_all()
    trans = mst.build_accurate()
    words = mst.encode_accurate(trans)
    wide = limg_amd.host_accurate_table(len(trans))
    cls = {}
    for s, t in enumerate(trans):
        if t[0] != "final":
            for ok in (True, False):
                n = trans[t[1 if ok else 2]]
                cls[(s, ok)] = ("final" if n[0] == "final" else changed(t[0], n[0]), t[0][3], ok)
    root = [int(v.rstrip("u"), 16) for v in re.search(r"#define LIMG_SEARCH_ROOT \{ ([^}]*) \}", open(mst.TABLE_HEADER).read()).group(1).split(", ")]
    return dict(trans=trans, words=words, wide=[tuple(int(v) for v in e) for e in wide], cls=cls, root=root)


@pytest.fixture(scope="module")
def default():
    """the default table: the generator's states and words, the hot states, the class of every edge that leaves a non-hot state"""
    trans = mst.build()
    words = mst.encode(trans)
    hot = {n["sid"] for n in mst.hot_nodes(mst.hot_tree(trans, mst.load_hot_paths()))}
    cls = {}
    for s, t in enumerate(trans):
        if t[0] != "final" and s not in hot:
            for ok in (True, False):
                n = t[1 if ok else 2]
                cls[(s, ok)] = ("final" if trans[n][0] == "final" else (words[n][0] >> 5) & 7, ok)
    return dict(trans=trans, words=words, hot=hot, cls=cls)


def test_committed_headers_are_what_the_generator_emits(acc, default):
    assert open(mst.TABLE_HEADER).read() == mst.emit_table(default["words"]), "limg_search_table.h is stale: run tools/make_search_table.py"
    assert open(mst.ACC_HEADER).read() == mst.emit_accurate(acc["words"]), "limg_search_table_accurate.h is stale: run tools/make_search_table.py"
    assert acc["root"] == list(default["words"][0])


def test_the_library_refuses_a_buffer_of_another_size(acc):
    import ctypes as C
    import limg_amd
    lib = limg_amd.load_library()
    n = len(acc["trans"]) * 8
    buf = np.full(n + 8, 0xA5A5A5A5, dtype=np.uint32)
    for dwords in (0, n - 8, n + 8):
        assert lib.limg_hip_host_accurate_table(buf.ctypes.data_as(C.c_void_p), dwords) == 101  # limg_hip_error_InvalidParameter
    assert (buf == 0xA5A5A5A5).all()
    assert lib.limg_hip_host_accurate_table(None, n) == 102  # limg_hip_error_ArgumentNull
    assert lib.limg_hip_host_accurate_table(buf.ctypes.data_as(C.c_void_p), n) == 0
    assert [tuple(int(v) for v in e) for e in buf[:n].reshape(-1, 8)] == acc["wide"] and (buf[n:] == 0xA5A5A5A5).all()


def test_expanded_table_every_state_and_both_edges(acc):
    trans, wide = acc["trans"], acc["wide"]
    assert len(wide) == len(trans) == 18878 and len(trans) * 32 < 1 << 24
    finals = 0
    for s, t in enumerate(trans):
        e = wide[s]
        if t[0] == "final":
            finals += 1
            assert e == (1 << 31, 0, 0, 0, 0, 0, 0, 0), s
            continue
        (a, b, c, phase), p, f = t
        assert e[0] == (a | (0x20 if phase == 2 else 0)) and (e[3], e[4]) == (b, c) and e[5:] == (mst.MUL[a], mst.MUL[b], mst.MUL[c]), (s, e, t)
        for k, n in ((1, p), (2, f)):
            off, mask = e[k] & 0xFFFFFF, e[k] >> 24
            assert off == n * 32 and off < 1 << 24, (s, k)
            want = 0 if trans[n][0] == "final" else changed(t[0], trans[n][0])
            assert mask == want, "state %d (%s) -> %d (%s): mask %d, changed %d" % (s, t[0], n, trans[n][0], mask, want)
    assert finals == 1
    # the classes the coverage conditions below are stated in
    assert len(set(acc["cls"].values())) == 23, sorted(map(acc_class_name, set(acc["cls"].values())))


# ---- the kernel's walk ------------------------------------------------------------------------------------------------------------------------------------------
def kernel_walk(wide, root, outcome, rebuilds=None):
    """Model of search_accurate_automaton over the expanded table: the root triple's terms first (LIMG_SEARCH_ROOT), state 0's mask by comparison with it, then per
    trial only the factors the taken edge's mask names.  `cached`: the (shift, multiplier) each factor's terms were last built with.  Asserts at every trial that
    they are the state's.  -> (shift, trials)"""
    cached = [(root[0] & 31, root[5]), (root[3], root[6]), (root[4], root[7])]
    e = wide[0]
    mask = (1 if (e[0] & 31) != (root[0] & 31) else 0) | (2 if e[3] != root[3] else 0) | (4 if e[4] != root[4] else 0)
    best, min_be, n = (0, 0, 0), 0xFFFFFFFF, 0
    while not (e[0] >> 31):
        t = (e[0] & 31, e[3], e[4])
        for k in range(3):
            if mask & (1 << k):
                cached[k] = (t[k], e[5 + k])
                if rebuilds is not None:
                    rebuilds.add((k, t[k]))
        assert cached == [(s, mst.MUL[s]) for s in t], (n, cached, t)
        ok, be = outcome(*t)
        n += 1
        off = e[2]
        if ok:
            off = e[1]
            if not (e[0] & 0x20) or be < min_be:
                best, min_be = t, be
        mask = off >> 24
        assert (off & 0xFFFFFF) % 32 == 0
        e = wide[(off & 0xFFFFFF) // 32]
    return best, n


def test_kernel_walk_equals_the_generators_on_random_outcomes(acc):
    """the generator of test_accurate_search_automaton_equals_loops_on_random_outcomes (tests/test_host.py), the pass probability drawn per walk and, for a third
    of the walks, pushed to the ends (long phase-1 climbs, long phase-2 rows); few distinct block errors, so phase-2 ties occur"""
    rnd = random.Random(11)
    longest, rebuilds = 0, set()
    for i in range(900):
        pr = rnd.random() if i % 3 else rnd.choice((0.02, 0.9, 0.97, 1.0))
        spread = rnd.choice((3, 50, 5000))
        memo = {}

        def outcome(a, b, c):
            if (a, b, c) not in memo:
                memo[(a, b, c)] = (rnd.random() < pr, rnd.randrange(1, spread + 1))
            return memo[(a, b, c)]
        got = kernel_walk(acc["wide"], acc["root"], outcome, rebuilds)
        assert got == mst.walk_accurate(acc["words"], outcome), i
        longest = max(longest, got[1])
    assert longest >= 100 and len(rebuilds) == 27


# ---- the corpus -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def acc_replay(acc, oracle):
    """every whole block of the accurate corpus walked with the oracle's trial: what the walks visit, per input"""
    words, cls = acc["words"], acc["cls"]
    per_input = []
    for name, img, alpha, ef in inputs.accurate_inputs(oracle):
        got = dict(name=name, alpha=alpha, states=set(), edges=set(), ties=set(), rebuilds=set(), longest=0)
        for outcome, want in inputs.blocks_of(oracle, img, alpha, ef, fast=False):
            s, n, shift, min_be = 0, 0, (0, 0, 0), None
            while not (words[s][0] >> 31):
                w0, w1 = words[s]
                t = (w0 & 15, (w0 >> 4) & 15, (w0 >> 8) & 15)
                ok, be = outcome(*t)
                got["states"].add(s)
                got["edges"].add((s, ok))
                n += 1
                if ok and (w0 & 0x1000):
                    got["ties"].add("better" if be < min_be else "equal" if be == min_be else "worse")
                if ok and (not (w0 & 0x1000) or be < min_be):
                    shift, min_be = t, be
                s = (w1 & 0xFFFF) if ok else (w1 >> 16)
            assert shift == want, (name, shift, want)  # the replay ends at the oracle's shifts
            assert mst.walk_accurate(words, outcome) == (shift, n), name
            assert kernel_walk(acc["wide"], acc["root"], outcome, got["rebuilds"]) == (shift, n), name
            got["longest"] = max(got["longest"], n)
        per_input.append(got)
    return per_input


def test_accurate_corpus_reaches_every_edge_class(acc, acc_replay):
    """what tests/test_gpu_search_tables.py rests on, in 3 and 4 channels taken together"""
    cls = acc["cls"]
    union = {k: set().union(*[r[k] for r in acc_replay]) for k in ("states", "edges", "ties", "rebuilds")}
    reached = {cls[e] for e in union["edges"]}
    longest = max(r["longest"] for r in acc_replay)
    print("accurate automaton: %d of %d non-final states, %d of %d edges, %d of %d classes, %d of 27 rebuilds, phase-2 passes %s, longest walk %d trials"
          % (len(union["states"]), len(acc["trans"]) - 1, len(union["edges"]), len(cls), len(reached), len(set(cls.values())), len(union["rebuilds"]),
             sorted(union["ties"]), longest))
    for alpha in (True, False):  # the kernels of 3 and of 4 channels are separate instances: each walks every class on its own inputs
        part = {cls[e] for r in acc_replay if r["alpha"] == alpha for e in r["edges"]}
        assert part == set(cls.values()), "%d channels alone do not reach: %s" % (4 if alpha else 3, "; ".join(sorted(map(acc_class_name, set(cls.values()) - part))))
    assert {r["alpha"] for r in acc_replay} == {True, False}
    missing = set(cls.values()) - reached
    assert not missing, "edge classes not reached: " + "; ".join(sorted(map(acc_class_name, missing)))
    assert union["rebuilds"] == {(k, s) for k in range(3) for s in range(9)}, sorted({(k, s) for k in range(3) for s in range(9)} - union["rebuilds"])
    assert union["ties"] == {"better", "equal", "worse"}, union["ties"]
    assert longest >= 100
    assert len(union["states"]) >= 5000


# Classes of edges that leave non-hot states of the default table and that no input reaches: {class name: what was searched}.  (None: every class is reached.)
DEFAULT_UNREACHED = {}


@pytest.fixture(scope="module")
def default_replay(default, oracle):
    words = default["words"]
    per_input = []
    for name, img, alpha, ef in inputs.default_inputs(oracle):
        got = dict(name=name, alpha=alpha, states=set(), edges=set())
        for outcome, want in inputs.blocks_of(oracle, img, alpha, ef, fast=True):
            s = 0
            while not (words[s][0] >> 31):
                w = words[s]
                ok = outcome(w[0] & 31, w[3], w[4])[0]
                got["states"].add(s)
                got["edges"].add((s, ok))
                s = (w[1] if ok else w[2]) // mst.ENTRY_BYTES
            assert (words[s][0] & 31, words[s][3], words[s][4]) == want, (name, s, want)  # the replay ends at the oracle's shifts
            assert mst.walk(words, lambda a, b, c: outcome(a, b, c)[0])[0] == want, name  # (the walk with cached terms: its masks hold along this path)
        per_input.append(got)
    return per_input


def test_default_corpus_reaches_every_edge_class_outside_the_hot_subtree(default, default_replay):
    cls, hot = default["cls"], default["hot"]
    assert len(set(cls.values())) == 14, sorted(map(default_class_name, set(cls.values())))
    states = set().union(*[r["states"] for r in default_replay]) - hot
    edges = set().union(*[r["edges"] for r in default_replay]) & set(cls)
    reached = {cls[e] for e in edges}
    print("default table outside the hot subtree: %d of %d non-final states, %d of %d edges, %d of %d classes"
          % (len(states), sum(t[0] != "final" for t in default["trans"]) - len(hot), len(edges), len(cls), len(reached), len(set(cls.values()))))
    assert {r["alpha"] for r in default_replay} == {True, False}
    missing = {default_class_name(c) for c in set(cls.values()) - reached}
    assert missing == set(DEFAULT_UNREACHED), "edge classes not reached: " + "; ".join(sorted(missing ^ set(DEFAULT_UNREACHED)))
    assert set(DEFAULT_UNREACHED) <= {"rebuild B+C after a pass", "rebuild A+B+C after a pass"}  # no other class may be left out
    assert len(states) >= 480
