"""limg_hip_cli --decode <file> <out.tga> --resize WxH [--window x,y,w,h] [--flip]: the CLI (a program on the product library) writes the TGA of the numpy statement of
the resized decode's contract (tests/window_resized.py) applied to its own full --decode output -- the whole image or the window of it, stated in full-resolution
pixels, at the level AUTO picks, mirrored with --flip -- for a version 1 file (--stream) and a version 2 file (--blocked-stream); a malformed size, --scale with
--resize and --flip alone are rejected.  The same file through decode_stream_windows_resized in this process, on the library the test runs on, gives the same pixels."""
import subprocess

import numpy as np
import pytest

import lib_axis as L
import window_resized as R
from lib_axis import lib, lib_product  # noqa: F401  (fixtures: "test" / "product")
from test_cli import PNG, _read_tga
from window_scaled import pyramid

pytestmark = pytest.mark.gpu
# (--window or None, W, H, flip): a thumbnail at level 2, an upscaled detail, a mirrored sample at level 1 with another aspect
CASES = ((None, 200, 120, False), ((700, 400, 90, 60), 153, 102, False), ((51, 25, 600, 500), 224, 224, True))


@pytest.fixture(scope="module")
def cli():
    from limg_amd import build
    return build.build_cli()


@pytest.mark.parametrize("version", [1, 2])
def test_decode_resized(cli, lib, tmp_path, version):
    out = str(tmp_path / "o.lmg3")
    flags = ["--fixed-blocks", "--stream", out] if version == 1 else ["--blocked-stream", out]
    r = subprocess.run([cli, PNG, "--single-thread", "--out-dir", str(tmp_path)] + flags, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    full, part = str(tmp_path / "full.tga"), str(tmp_path / "part.tga")
    r = subprocess.run([cli, "--decode", out, full], capture_output=True, text=True)
    assert r.returncode == 0 and "1024 x 618 pixels, RGB.\nWrote decoded file.\n" in r.stdout and "resized" not in r.stdout, r.stdout + r.stderr  # as without the feature
    image = _read_tga(full)
    assert image.shape == (618, 1024)
    pyr = pyramid(image)
    wins = []
    for win, ow, oh, flip in CASES:
        rect = win or (0, 0, 1024, 618)
        want, level = R.resize(pyr, rect, ow, oh, R.AUTO, flip)
        args = [cli, "--decode", out, part, "--resize", "%dx%d" % (ow, oh)] + (["--window", "%d,%d,%d,%d" % win] if win else []) + (["--flip"] if flip else [])
        r = subprocess.run(args, capture_output=True, text=True)
        assert r.returncode == 0 and "window %d x %d at (%d, %d) resized to %d x %d%s." % (rect[2], rect[3], rect[0], rect[1], ow, oh, ", mirrored" if flip else "") in r.stdout, r.stdout + r.stderr
        got = _read_tga(part)
        assert got.shape == (oh, ow) and np.array_equal(got, want), (win, ow, oh, flip, level)
        wins.append((R.AUTO, 1 if flip else 0, *rect, ow, oh))
    assert {R.auto_level(*(win or (0, 0, 1024, 618))[2:], ow, oh) for win, ow, oh, _ in CASES} == {0, 1, 2}
    for bad, text in ((["--resize", "200"], "'--resize' takes WxH"), (["--resize", "0x5"], "'--resize' takes WxH"), (["--resize", "20x40000"], "'--resize' takes WxH"),
                      (["--resize", "20x10", "--scale", "2"], "does not go with '--scale'"), (["--flip"], "'--flip' goes with '--resize'"),
                      (["--resize", "20x10", "--window", "1000,600,25,18"], "not inside the image")):
        r = subprocess.run([cli, "--decode", out, part] + bad, capture_output=True, text=True)
        assert r.returncode != 0 and text in r.stdout, (bad, r.stdout)
    st = np.fromfile(out, dtype=np.uint8)
    g = L.open_context(lib)
    try:
        mine = (g.decode_stream_windows_resized if version == 1 else g.blocked_decode_stream_windows_resized)(st, wins)
        g.check()
    finally:
        g.close()
    opaque = np.uint32(0xFF000000)
    for m, (win, ow, oh, flip) in zip(mine, CASES):
        assert np.array_equal(m | opaque, R.resize(pyr, win or (0, 0, 1024, 618), ow, oh, R.AUTO, flip)[0] | opaque), (win, ow, oh)


L.product_twins(globals())
