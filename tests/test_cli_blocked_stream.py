"""limg_hip_cli --blocked-stream: the single-file merged-block mode writes the version 2 stream of that very encode next to its planes (no second encode), checks
that it decodes to the merged-block decoded image, and --decode reads it back.  The file the CLI (a program on the product library) wrote is also decoded in this
process, on the library the test runs on."""
import json
import os
import subprocess

import numpy as np
import pytest

import golden_util as gu
import lib_axis as L
from lib_axis import lib, lib_product  # noqa: F401  (fixtures: "test" / "product")
import limg_amd
from test_cli import PNG, _TGA, _read_tga

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cli():
    from limg_amd import build
    return build.build_cli()


def test_blocked_stream_of_the_single_file_encode(cli, lib, oracle, tmp_path):
    out = str(tmp_path / "o.lmg3")
    r = subprocess.run([cli, PNG, "--single-thread", "--out-dir", str(tmp_path), "--blocked-stream", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "decoding it reproduces the merged-block decoded image" in r.stdout
    st = np.fromfile(out, dtype=np.uint8)
    sx, sy, alpha, total, rects = limg_amd.blocked_stream_info(st)
    assert (sx, sy, alpha, total) == (1024, 618, False, st.size)
    e = json.load(open(os.path.join(gu.G, "blocked.json")))["original_rgb"]
    assert rects == e["regions"]
    # the planes it wrote still match the reference's hashes, as in test_cli.py
    names = dict(_TGA, limg_bpp="pBitsPerPixel", limg_block_idx_raw="pBlockIndex")
    for f, k in names.items():
        assert oracle.fnv(_read_tga(str(tmp_path / (f + ".tga")))) == e["planes"][k], (f, k)
    # --decode accepts the version 2 file
    r = subprocess.run([cli, "--decode", out, str(tmp_path / "again.tga")], capture_output=True, text=True)
    assert r.returncode == 0 and "1024 x 618 pixels, RGB." in r.stdout, r.stdout + r.stderr
    decoded = _read_tga(str(tmp_path / "limg_out.tga"))
    assert np.array_equal(_read_tga(str(tmp_path / "again.tga")), decoded)
    # ... and so does the library this test runs on, in this process
    g = L.open_context(lib)
    try:
        assert np.array_equal(g.blocked_decode_stream(st) | np.uint32(0xFF000000), decoded | np.uint32(0xFF000000))
        g.check()
    finally:
        g.close()


L.product_twins(globals())
