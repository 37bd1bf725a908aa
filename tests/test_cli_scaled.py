"""limg_hip_cli --decode <file> <out.tga> --scale 1|2|4|8 [--window x,y,w,h]: the CLI (a program on the product library) writes the TGA of the numpy box reduction
(tests/window_scaled.py) of its full --decode output -- the whole reduced image, or the window of it, stated in reduced coordinates -- for a version 1 file (--stream)
and a version 2 file (--blocked-stream); any other scale is rejected; without --scale the decode mode does what it did.  The same file reduced in this process by
decode_stream_windows_scaled, on the library the test runs on, gives the same pixels."""
import subprocess

import numpy as np
import pytest

import lib_axis as L
from lib_axis import lib, lib_product  # noqa: F401  (fixtures: "test" / "product")
from test_cli import PNG, _read_tga
from window_scaled import reduce

pytestmark = pytest.mark.gpu
WINDOWS = {2: (51, 25, 333, 211), 8: (3, 5, 120, 70)}  # in reduced coordinates: 512 x 309 and 128 x 77


@pytest.fixture(scope="module")
def cli():
    from limg_amd import build
    return build.build_cli()


@pytest.mark.parametrize("version", [1, 2])
def test_decode_scaled(cli, lib, tmp_path, version):
    out = str(tmp_path / "o.lmg3")
    flags = ["--fixed-blocks", "--stream", out] if version == 1 else ["--blocked-stream", out]
    r = subprocess.run([cli, PNG, "--single-thread", "--out-dir", str(tmp_path)] + flags, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    full, part = str(tmp_path / "full.tga"), str(tmp_path / "part.tga")
    r = subprocess.run([cli, "--decode", out, full], capture_output=True, text=True)
    assert r.returncode == 0 and "1024 x 618 pixels, RGB.\nWrote decoded file.\n" in r.stdout and "scale" not in r.stdout, r.stdout + r.stderr  # as without the feature
    image = _read_tga(full)
    assert image.shape == (618, 1024)
    for k, level in ((2, 1), (8, 3)):
        want = reduce(image, level)
        assert want.shape == (618 >> level, 1024 >> level)
        r = subprocess.run([cli, "--decode", out, part, "--scale", str(k)], capture_output=True, text=True)
        assert r.returncode == 0 and "scale 1/%d: window %d x %d at (0, 0) of %d x %d." % (k, want.shape[1], want.shape[0], want.shape[1], want.shape[0]) in r.stdout, r.stdout + r.stderr
        got = _read_tga(part)
        assert got.shape == want.shape and np.array_equal(got, want), k
        x, y, w, h = WINDOWS[k]
        r = subprocess.run([cli, "--decode", out, part, "--window", "%d,%d,%d,%d" % WINDOWS[k], "--scale", str(k)], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        got = _read_tga(part)
        assert got.shape == (h, w) and np.array_equal(got, want[y:y + h, x:x + w]), k
    r = subprocess.run([cli, "--decode", out, part, "--scale", "3"], capture_output=True, text=True)
    assert r.returncode != 0 and "'--scale' takes 1, 2, 4 or 8." in r.stdout
    r = subprocess.run([cli, "--decode", out, part, "--scale", "8", "--window", "100,50,29,28"], capture_output=True, text=True)  # 128 x 77: one row too many
    assert r.returncode != 0 and "not inside the reduced image" in r.stdout
    st = np.fromfile(out, dtype=np.uint8)
    g = L.open_context(lib)
    try:
        mine = (g.decode_stream_windows_scaled if version == 1 else g.blocked_decode_stream_windows_scaled)(st, [(0, 0, 0, 1024, 618), (3, 0, 0, 128, 77)])
        g.check()
    finally:
        g.close()
    opaque = np.uint32(0xFF000000)
    assert np.array_equal(mine[0] | opaque, image | opaque) and np.array_equal(mine[1] | opaque, reduce(image, 3) | opaque)


L.product_twins(globals())
