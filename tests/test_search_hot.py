"""The hot subtree of the default shift search as generated straight-line code (tools/search_hot_paths.json -> tools/make_search_table.py ->
limg_amd/csrc/limg_search_hot.h): the committed header is what the generator emits; the generator's model of that code (`hot_walk`: named term sets, literal
shifts, hand-over to the table loop) tries the same triples and ends at the same shifts as the literal restatement of the reference's search; and the inputs of
tests/test_gpu_search_hot.py reach every hot state and both of its edges.  CPU only."""
import itertools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import make_search_table as mst  # noqa: E402
import search_hot_inputs as inputs  # noqa: E402


@pytest.fixture(scope="module")
def hot():
    trans = mst.build()
    paths = mst.load_hot_paths()
    return dict(trans=trans, words=mst.encode(trans), paths=paths, tree=mst.hot_tree(trans, paths))


def reference_walk(outcomes):
    """the literal restatement of the reference's search on the same outcomes -> (triples tried, final shifts)"""
    it = iter(outcomes)
    g = mst.search_fast()
    tried = []
    try:
        t = next(g)
        while True:
            tried.append(tuple(t))
            t = g.send(bool(next(it)))
    except StopIteration as e:
        return tried, tuple(e.value)


def test_generated_header_is_current(hot):
    want = mst.emit_hot(hot["tree"])
    assert open(mst.HOT_HEADER).read() == want, "limg_search_hot.h is stale: run tools/make_search_table.py"
    assert "#define LIMG_SEARCH_HOT_STATES %d\n" % len(hot["paths"]) in want


def test_hot_set_is_a_prefix_closed_part_of_the_tree(hot):
    paths = hot["paths"]
    assert "" in paths and all(p[:-1] in paths for p in paths if p)
    nodes = {n["path"]: n for n in mst.hot_nodes(hot["tree"])}
    assert set(nodes) == set(paths)
    for p, n in nodes.items():  # the node's triple is the one the reference's search asks for after these outcomes
        tried, _ = reference_walk(itertools.chain([c == "P" for c in p], itertools.repeat(False)))
        assert tried[len(p)] == tuple(n["triple"]), p


def test_every_exit_hands_over_the_tables_offset(hot):
    words = hot["words"]
    exits = finals = 0
    for n in mst.hot_nodes(hot["tree"]):
        s = 0
        for c in n["path"]:
            s = words[s][1 if c == "P" else 2] // mst.ENTRY_BYTES
        assert s == n["sid"] and (words[s][0] & 31, words[s][3], words[s][4]) == tuple(n["triple"])
        for ok in (True, False):
            e = n["edge"][ok]
            nxt = words[s][1 if ok else 2]
            w = words[nxt // mst.ENTRY_BYTES]
            if e[0] == "exit":
                exits += 1
                assert e[1] == nxt and not (w[0] >> 31)
            elif e[0] == "final":
                finals += 1
                assert (w[0] >> 31) and (w[0] & 31, w[3], w[4]) == tuple(e[1])
            else:
                assert e[1]["sid"] == nxt // mst.ENTRY_BYTES
    assert exits > 0 and finals > 0


@pytest.mark.parametrize("K", [None, 0, 1, 2])
def test_hot_walk_equals_the_reference_search(hot, K):
    """every hot state with both outcomes (continued with all passes, all fails and random outcomes), and 10 000 random outcome sequences"""
    tree = hot["tree"] if K is None else mst.hot_tree(hot["trans"], hot["paths"], K)
    words = hot["words"]
    rng = np.random.default_rng(3)
    seqs = []
    for p in hot["paths"]:
        for ok in (True, False):
            head = [c == "P" for c in p] + [ok]
            seqs += [(head, True), (head, False), (head, None)]
    seqs += [([], None)] * 10000
    left_to_the_table = 0
    for head, rest in seqs:
        if rest is None:
            prob = rng.random()
            tail = (rng.random(64) < prob).tolist() + [False] * 64  # (a search is at most ~ 40 trials long; it ends on its own)
        else:
            tail = [rest] * 128
        out = head + tail
        want = reference_walk(out)
        tried, shift, builds = mst.hot_walk(out, tree, words)
        assert (tried, shift) == want, (head, rest)
        left_to_the_table += "".join("P" if o else "F" for o in out[:len(tried) - 1]) not in hot["paths"]  # the last state tried is not a hot one
    assert left_to_the_table > 1000  # (the hand-over to the table loop is exercised, not only the straight-line part)
    # reuse never builds more than the table walk does (which rebuilds exactly the changed factors)
    for p in hot["paths"]:
        out = [c == "P" for c in p] + [False] * 128
        t_tried, t_shift, t_builds = _table_walk(words, out)
        tried, shift, builds = mst.hot_walk(out, tree, words)
        assert (tried, shift) == (t_tried, t_shift) and builds <= t_builds, p


def _table_walk(words, outcomes):
    it = iter(outcomes)
    s, tried, builds = 0, [], 0
    while not (words[s][0] >> 31):
        w = words[s]
        tried.append((w[0] & 31, w[3], w[4]))
        for k in range(3):
            if (w[0] >> 5) & (1 << k) and not (k > 0 and tried[-1][k] > 7):
                builds += 1
        s = (w[1] if next(it) else w[2]) // mst.ENTRY_BYTES
    w = words[s]
    return tried, (w[0] & 31, w[3], w[4]), builds


def test_gpu_test_inputs_reach_every_hot_state_and_edge(hot, oracle):
    """the condition tests/test_gpu_search_hot.py rests on: its inputs, replayed with the oracle's trial, enter every hot state and take both of its edges"""
    need = {(p, ok) for p in hot["paths"] for ok in (True, False)}
    seen = set()
    for img, alpha, ef in inputs.coverage_inputs(oracle):
        seen |= inputs.visited_edges(oracle, img, alpha, ef) & need
        if seen == need:
            break
    assert seen == need, sorted(need - seen)
