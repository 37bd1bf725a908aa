"""limg_hip_cli --decode <file> --window x,y,w,h: the CLI (a program on the product library) writes a w x h TGA that equals that slice of its full --decode output, for
a version 1 file (--stream) and a version 2 file (--blocked-stream); the same file decoded in this process by decode_stream_window, on the library the test runs on,
gives the same pixels."""
import subprocess

import numpy as np
import pytest

import lib_axis as L
from lib_axis import lib, lib_product  # noqa: F401  (fixtures: "test" / "product")
from test_cli import PNG, _read_tga

pytestmark = pytest.mark.gpu
WINDOW = (100, 50, 333, 211)


@pytest.fixture(scope="module")
def cli():
    from limg_amd import build
    return build.build_cli()


@pytest.mark.parametrize("version", [1, 2])
def test_decode_window(cli, lib, tmp_path, version):
    out = str(tmp_path / "o.lmg3")
    flags = ["--fixed-blocks", "--stream", out] if version == 1 else ["--blocked-stream", out]
    r = subprocess.run([cli, PNG, "--single-thread", "--out-dir", str(tmp_path)] + flags, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    full, part = str(tmp_path / "full.tga"), str(tmp_path / "part.tga")
    r = subprocess.run([cli, "--decode", out, full], capture_output=True, text=True)
    assert r.returncode == 0 and "1024 x 618 pixels, RGB." in r.stdout, r.stdout + r.stderr
    x, y, w, h = WINDOW
    r = subprocess.run([cli, "--decode", out, part, "--window", "%d,%d,%d,%d" % WINDOW], capture_output=True, text=True)
    assert r.returncode == 0 and "1024 x 618 pixels, RGB; window 333 x 211 at (100, 50)." in r.stdout, r.stdout + r.stderr
    want = _read_tga(full)[y:y + h, x:x + w]
    got = _read_tga(part)
    assert got.shape == (h, w) and np.array_equal(got, want)
    r = subprocess.run([cli, "--decode", out, part, "--window", "1000,50,333,211"], capture_output=True, text=True)
    assert r.returncode != 0 and "not inside the image" in r.stdout
    st = np.fromfile(out, dtype=np.uint8)
    g = L.open_context(lib)
    try:
        mine = (g.decode_stream_window if version == 1 else g.blocked_decode_stream_window)(st, x, y, w, h)
        g.check()
    finally:
        g.close()
    assert np.array_equal(mine | np.uint32(0xFF000000), want | np.uint32(0xFF000000))


L.product_twins(globals())
