"""limg_hip_cli <image> --fixed-blocks --stream o.lmg3 --max-bytes N: the CLI (a program on the product library) reports the error factor the budget search chose, the
number of size probes, the bytes and whether the budget was met -- the choice of the search restated over the oracle's sizes; the file is no longer than N, equals the file that `--error-factor <that value> --stream` writes, and
equals the stream this process encodes at that error factor on the library the test runs on."""
import re
import subprocess

import numpy as np
import pytest

import lib_axis as L
from lib_axis import lib, lib_product  # noqa: F401  (fixtures: "test" / "product")
import golden_util as gu
from rate_search import oracle_size, restated_search
from test_cli import PNG

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cli():
    from limg_amd import build
    return build.build_cli()


def test_stream_to_a_byte_budget(cli, lib, oracle, tmp_path):
    img = gu.load_png(PNG)  # 1024 x 618 RGB: the CLI encodes it without alpha; partial blocks in the last row, so every size is a whole stream encode
    memo = {}

    def size(h):
        if h not in memo:
            memo[h] = oracle_size(oracle, img, False, 2 * h)
        return memo[h]

    budget = (size(1) + size(512)) // 2  # half way between the sizes at the default bounds: met, after a bisection
    want_h, want_within, asked, want_bytes = restated_search(size, 1, 512, budget)
    assert want_within == 1 and len(asked) > 2
    out, again = str(tmp_path / "o.lmg3"), str(tmp_path / "again.lmg3")
    common = [cli, PNG, "--fixed-blocks", "--single-thread", "--no-output"]
    r = subprocess.run(common + ["--stream", out, "--max-bytes", str(budget)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"Budget: %d bytes; error factor (\d+) after (\d+) size probes; (\d+) bytes; budget (met|NOT met)\." % budget, r.stdout)
    assert m and "reproduces the decoded image" in r.stdout, r.stdout
    ef, probes, nbytes, met = int(m.group(1)), int(m.group(2)), int(m.group(3)), m.group(4) == "met"
    st = np.fromfile(out, dtype=np.uint8)
    assert (ef, probes, nbytes, met) == (2 * want_h, len(asked), want_bytes, True), (r.stdout, want_h, asked, want_bytes)
    assert st.size == nbytes <= budget
    r = subprocess.run(common + ["--stream", again, "--error-factor", str(ef)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert np.array_equal(st, np.fromfile(again, dtype=np.uint8))
    g = L.open_context(lib)
    try:
        mine, res = g.encode_stream_budget(img, False, budget)
        assert (res.errorFactor, res.bytes, res.probes, res.withinBudget) == (ef, nbytes, probes, 1) and np.array_equal(mine, st)
        g.check()
    finally:
        g.close()
    # a budget nothing meets: the stream of the largest error factor, said so; the options without '--stream' are refused
    r = subprocess.run(common + ["--stream", out, "--max-bytes", "1000", "--max-error-factor", "64"], capture_output=True, text=True)
    assert r.returncode == 0 and re.search(r"error factor 64 after 1 size probes; \d+ bytes; budget NOT met\.", r.stdout), r.stdout + r.stderr
    r = subprocess.run(common + ["--max-bytes", "1000"], capture_output=True, text=True)
    assert r.returncode == 1 and "'--max-bytes' is the byte budget of '--stream'" in r.stdout


L.product_twins(globals())
