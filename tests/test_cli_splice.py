"""limg_hip_cli --crop-stream / --join-streams: the CLI (a program on the product library) crops a file written by --stream, and --decode of the result equals the
--window decode of the original; the crops of its upper and lower part, joined, are the file again, byte for byte.  The same crop made in this process by
stream_crop, on the library the test runs on, gives the same bytes."""
import subprocess

import numpy as np
import pytest

import lib_axis as L
from lib_axis import lib, lib_product  # noqa: F401  (fixtures: "test" / "product")
from test_cli import PNG, _read_tga

pytestmark = pytest.mark.gpu
WINDOW = (96, 48, 928, 570)  # of 1024 x 618: from block (12, 6) to the image's corner, whose block row is 2 pixels high


@pytest.fixture(scope="module")
def cli():
    from limg_amd import build
    return build.build_cli()


def test_crop_and_join(cli, lib, tmp_path):
    src = str(tmp_path / "o.lmg3")
    r = subprocess.run([cli, PNG, "--single-thread", "--out-dir", str(tmp_path), "--fixed-blocks", "--stream", src], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    x, y, w, h = WINDOW
    crop, want_tga, got_tga = str(tmp_path / "crop.lmg3"), str(tmp_path / "want.tga"), str(tmp_path / "got.tga")
    r = subprocess.run([cli, "--crop-stream", src, crop, "--window", "%d,%d,%d,%d" % WINDOW], capture_output=True, text=True)
    assert r.returncode == 0 and "1024 x 618 pixels; window 928 x 570 at (96, 48):" in r.stdout and "Wrote stream file." in r.stdout, r.stdout + r.stderr
    r = subprocess.run([cli, "--decode", src, want_tga, "--window", "%d,%d,%d,%d" % WINDOW], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([cli, "--decode", crop, got_tga], capture_output=True, text=True)
    assert r.returncode == 0 and "928 x 570 pixels, RGB." in r.stdout, r.stdout + r.stderr
    got = _read_tga(got_tga)
    assert got.shape == (h, w) and np.array_equal(got, _read_tga(want_tga))
    # a window the blocks cannot be copied for is refused with the reason
    for bad in ("100,48,924,570", "96,48,900,570", "96,48,1000,570"):
        r = subprocess.run([cli, "--crop-stream", src, crop + ".bad", "--window", bad], capture_output=True, text=True)
        assert r.returncode != 0 and "cannot be cropped" in r.stdout, (bad, r.stdout)
    r = subprocess.run([cli, "--crop-stream", src, crop], capture_output=True, text=True)
    assert r.returncode != 0 and "Usage:" in r.stdout
    # upper and lower part, joined: the file again
    top, bottom, joined = str(tmp_path / "top.lmg3"), str(tmp_path / "bottom.lmg3"), str(tmp_path / "joined.lmg3")
    for path, win in ((top, "0,0,1024,304"), (bottom, "0,304,1024,314")):
        r = subprocess.run([cli, "--crop-stream", src, path, "--window", win], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([cli, "--join-streams", joined, top, bottom], capture_output=True, text=True)
    assert r.returncode == 0 and "2 strips joined: 1024 x 618 pixels, RGB," in r.stdout, r.stdout + r.stderr
    st = np.fromfile(src, dtype=np.uint8)
    assert np.array_equal(np.fromfile(joined, dtype=np.uint8), st)
    r = subprocess.run([cli, "--join-streams", joined, bottom, top], capture_output=True, text=True)
    assert r.returncode != 0 and "Only the last strip" in r.stdout, r.stdout
    g = L.open_context(lib)
    try:
        mine = g.stream_crop(st, x, y, w, h)
        g.check()
    finally:
        g.close()
    assert np.array_equal(mine, np.fromfile(crop, dtype=np.uint8))


L.product_twins(globals())
