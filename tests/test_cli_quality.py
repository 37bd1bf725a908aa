"""limg_hip_cli <image> --fixed-blocks --stream o.lmg3 --min-psnr dB: the CLI (a program on the product library) reports the error factor the quality search chose, the
number of error probes, the bytes, the PSNR and whether the target was met -- the choice of the search restated over the oracle's error sums; the file equals the file
that `--error-factor <that value> --stream` writes and the stream this process encodes at that error factor on the library the test runs on.
limg_hip_cli --decode o.lmg3 --compare <image>: the reference's PSNR line for the stream, with the oracle's numbers, and no image written."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import lib_axis as L
from lib_axis import lib, lib_product  # noqa: F401  (fixtures: "test" / "product")
import golden_util as gu
from stream_error_ref import oracle_error_sum, restated_quality_search
from test_cli import PNG

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cli():
    from limg_amd import build
    return build.build_cli()


def _psnr(esum, pixels, alpha):
    return 10.0 * math.log10(255.0 * 255.0 * (12.0 if alpha else 9.0) * pixels / esum)


def test_stream_to_a_quality_target_and_compare(cli, lib, oracle, tmp_path):
    img = gu.load_png(PNG)  # 1024 x 618 RGB: the CLI encodes it without alpha; partial blocks in the last row
    memo = {}

    def E(h):
        if h not in memo:
            memo[h] = oracle_error_sum(oracle, img, False, 2 * h)
        return memo[h]

    g = L.open_context(lib)
    try:
        db = "%.4f" % ((_psnr(E(1), img.size, False) + _psnr(E(64), img.size, False)) / 2)  # half way between the bounds' PSNRs: met, after a bisection
        limit = g.error_sum_for_psnr(1024, 618, False, float(db))
        want_h, want_within, asked, want_sum = restated_quality_search(E, 1, 64, limit)
        assert want_within == 1 and len(asked) > 2
        out, again = str(tmp_path / "o.lmg3"), str(tmp_path / "again.lmg3")
        common = [cli, PNG, "--fixed-blocks", "--single-thread", "--no-output"]
        r = subprocess.run(common + ["--stream", out, "--min-psnr", db, "--min-error-factor", "2", "--max-error-factor", "128"], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        m = re.search(r"Quality: ([\d.]+) dB; error factor (\d+) after (\d+) error probes; (\d+) bytes; PSNR ([\d.]+) dB; target (met|NOT met)\.", r.stdout)
        assert m and "reproduces the decoded image" in r.stdout, r.stdout
        ef, probes, nbytes, psnr, met = int(m.group(2)), int(m.group(3)), int(m.group(4)), float(m.group(5)), m.group(6) == "met"
        st = np.fromfile(out, dtype=np.uint8)
        assert (ef, probes, met) == (2 * want_h, len(asked), True), (r.stdout, want_h, asked)
        assert st.size == nbytes and psnr == pytest.approx(_psnr(want_sum, img.size, False), abs=1e-4) and psnr >= float(db) - 1e-4
        r = subprocess.run(common + ["--stream", again, "--error-factor", str(ef)], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        assert np.array_equal(st, np.fromfile(again, dtype=np.uint8))
        mine, res = g.encode_stream_quality(img, False, limit, 2, 128)
        assert (res.errorFactor, res.bytes, res.probes, res.withinTarget, res.errorSum) == (ef, nbytes, probes, 1, want_sum) and np.array_equal(mine, st)
        g.check()
    finally:
        g.close()
    # --decode --compare: the reference's line for the stream against the image, and no image is written
    before = set(os.listdir(tmp_path))
    r = subprocess.run([cli, "--decode", out, "--compare", PNG], capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout + r.stderr
    dec = oracle.encode3d(img, False, error_factor=ef)["pDecoded"]
    p, mse = oracle.compare(img, dec, False)
    mx = 255.0 * 255.0 * 9.0
    line = "Image Perceptual RGB(A) PSNR: %4.2f dB (mean: %5.3f => %7.5f%% | sqrt: %5.3f%%)" % (p, mse, (mse / mx) * 100.0, (math.sqrt(mse) / math.sqrt(mx)) * 100.0)
    assert line in r.stdout and "1024 x 618 pixels, RGB." in r.stdout, (r.stdout, line)
    assert set(os.listdir(tmp_path)) == before
    # a target nothing meets: the stream of the smallest error factor, said so; the options' misuse is refused
    r = subprocess.run(common + ["--stream", out, "--min-psnr", "90", "--min-error-factor", "64", "--max-error-factor", "128"], capture_output=True, text=True)
    assert r.returncode == 0 and re.search(r"error factor 64 after 1 error probes; \d+ bytes; PSNR [\d.]+ dB; target NOT met\.", r.stdout), r.stdout + r.stderr
    r = subprocess.run(common + ["--min-psnr", "40"], capture_output=True, text=True)
    assert r.returncode == 1 and "'--min-psnr' is the quality target of '--stream'" in r.stdout
    r = subprocess.run(common + ["--stream", out, "--min-psnr", "40", "--max-bytes", "5000"], capture_output=True, text=True)
    assert r.returncode == 1 and "'--min-psnr' is the quality target of '--stream'" in r.stdout
    r = subprocess.run([cli, "--decode", out, "--compare", PNG, "--scale", "2"], capture_output=True, text=True)
    assert r.returncode == 1 and "'--compare' measures the whole stream" in r.stdout


L.product_twins(globals())
