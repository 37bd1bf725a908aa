"""CPU: the stored float-edge blocks (tests/float_edge_inputs.py) still reach, in the oracle as it is now, every edge of the float stage they were chosen for.
tests/test_gpu_float_edges.py holds the GPU to the oracle on exactly these inputs; if a test here fails after an oracle change, that file no longer proves
what it says.  The events are counted by the oracle's own fit and factor functions (oracle/limg_oracle.h, "event sink")."""
import numpy as np
import pytest

import float_edge_inputs as F


@pytest.fixture(scope="module")
def cov(oracle):
    return F.coverage(oracle)


def test_sink_counts_without_changing_results(oracle):
    """off by default and off again after the `with`; the records, shifts and factor bytes are the same with the sink on; several workers count what one counts"""
    img = F.cropped_image()
    plain = oracle.encode3d(img, True, planes=False, extras=True)
    with oracle.count_events() as ev:
        counted = oracle.encode3d(img, True, planes=False, extras=True)
    one = ev.counters.copy()
    assert one.any()
    for k in ("records", "shifts", "preA", "preB", "preC"):
        assert plain[k].tobytes() == counted[k].tobytes(), k
    oracle.encode3d(img, True, planes=False)
    assert np.array_equal(ev.counters, one)  # nothing counts once the sink is off
    with oracle.count_events() as ev4:
        oracle.encode3d(img, True, planes=False, pool_threads=1, worker_threads=4)
    assert np.array_equal(ev4.counters, one)  # the strips of a pool share no float-stage state: same blocks, same events, counted atomically


@pytest.mark.parametrize("channels", [3, 4])
def test_required_cells_on_whole_blocks(cov, channels):
    c = cov["whole"][str(channels)]
    missing = [k for k in F.required_cells(channels) if c["cells"].get(k, 0) < 1]
    assert not missing, missing
    assert c["table_indices"] == 2048


@pytest.mark.parametrize("context", ["partial", "region"])
@pytest.mark.parametrize("channels", [3, 4])
def test_required_cells_elsewhere(cov, context, channels):
    c = cov[context][str(channels)]["cells"]
    missing = [k for k in F.REQUIRED_ELSEWHERE if c.get(k, 0) < 1]
    assert not missing, missing


@pytest.mark.parametrize("context", ["whole", "partial", "tiny", "region"])
@pytest.mark.parametrize("channels", [3, 4])
def test_recorded_coverage_has_not_shrunk(cov, context, channels):
    """every cell the manifest lists is still reached, as many table indices, and an RSQRTPS argument at least as small"""
    want = F.manifest()["coverage"][context][str(channels)]
    got = cov[context][str(channels)]
    lost = [k for k in want["cells"] if got["cells"].get(k, 0) < 1]
    assert not lost, lost
    assert got["table_indices"] >= want["table_indices"]
    assert got["min_exponent"] <= want["min_exponent"]


def test_manifest_is_complete():
    """what the generator wrote: no required cell missing, 2 048 table indices with either channel count, an argument below 2^-90 (biased exponent 37)"""
    m = F.manifest()
    assert m["blocks"] == len(F.stored_blocks()) and not m["required_missing"]
    for ch in (3, 4):
        w = m["coverage"]["whole"][str(ch)]
        assert w["table_indices"] == 2048
        assert all(w["cells"].get(k, 0) >= 1 for k in F.required_cells(ch))
        for ctx in ("partial", "region"):
            assert all(m["coverage"][ctx][str(ch)]["cells"].get(k, 0) >= 1 for k in F.REQUIRED_ELSEWHERE), (ctx, ch)
    assert m["coverage"]["whole"]["4"]["min_exponent"] <= 37


# The required 4-channel cells (n == 64) that the suite's staple inputs miss -- a 512 x 64 photo-noise image, a 512 x 64 random gradient and the image of
# test_gpu_parity.py::test_degenerate_blocks together.  An `==`, so a change of an input or of the oracle shows up here.
STAPLES_MISS = ["dirA_zero_nonflat"] + ["tie.p1.%s" % t for t in ("03.lt2", "03.ge8", "12.ge8", "13.lt2", "13.ge8", "20.ge8", "21.ge8", "23.lt2", "23.ge8", "30.lt2",
                                                                  "30.ge8", "31.lt2", "31.ge8", "32.lt2", "32.ge8")]


def test_staple_inputs_do_not_replace_the_corpus(oracle):
    """The degenerate image alone reaches none of "dirA == 0 on a non-flat block", "record converted from k + 0.5" and "sign decided by the bias".  The three
    staples together still miss the first of them and 15 of the 24 tie cells, alpha lane ties all among them.  (Together they do reach the other two: gradients
    are full of exact ties, which the bias decides -- 283 pixels of this one -- and this photo-noise image has one record field on k + 0.5 in its 512 blocks.)"""
    staples = {"pn": oracle.photo_noise(512, 64, 1), "rg": oracle.random_gradient(512, 64, 1, True), "degenerate": F.degenerate_blocks_image()}
    reached = {k: F.summary(F.events_of(oracle, img, True), "whole", 4) for k, img in staples.items()}
    alone = reached["degenerate"]["cells"]
    assert [alone.get(k, 0) for k in ("dirA_zero_nonflat", "rec_tie", "bias_decides.p1")] == [0, 0, 0]
    union = set().union(*[set(r["cells"]) for r in reached.values()])
    assert [k for k in F.required_cells(4) if k not in union] == STAPLES_MISS
    assert min(r["min_exponent"] for r in reached.values()) == 89  # the corpus: 21 (tests/golden/float_edge_coverage.json)
