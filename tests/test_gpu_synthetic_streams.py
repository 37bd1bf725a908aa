"""The version 1 decoders on hand-built streams (tests/synthetic_streams.py): k_stream_decode, the window family (k_stream_window_decode, k_stream_windows_decode and
its tensor, scaled, resized and error forms) and k_splice_copy on streams no encoder made -- any int16 record, every shift triple with every escape pattern, groups of
8 blocks with no, one and only large blocks (the 32-bit branch of k_stream_decode), fields of every width.  Each result equals the ORACLE's decode of the same bytes
(the reference's a16 with 32-bit wrapping products), bit for bit, through the shared bodies of the window tests; each test ends with a clean check() and zero job
status words.  tests/test_synthetic_streams_cpu.py holds the corpus to what it must reach.

What these tests can and cannot see of k_stream_decode's `big` decision (tried on a scratch build with big forced to 0): the extreme and wild blocks then decode
wrongly (53 to 57 of 63 extreme blocks per stream, all wild ones), the over blocks do not -- with one value at +-2701 and 23 values within +-255 the packed form's
terms stay far below its 0x2000 bias, so it is still exact.  The over class checks that such a block, and the small blocks that share its group, come out right
through the 32-bit loop; that the loop is taken at exactly +-2701 shows in no pixel."""
import numpy as np
import pytest

import lib_axis as L
import stream_splice_ref as R
import synthetic_gpu as G
import synthetic_streams as Y
from oracle import stream as S

pytestmark = pytest.mark.gpu
NAMES = G.NAMES[1]


def _gpu(lib):
    g = L.open_context(lib)
    yield g
    g.check()
    g.close()


@pytest.fixture(scope="module")
def gpu():
    yield from _gpu("test")


@pytest.fixture(scope="module")
def gpu_product():
    yield from _gpu("product")


@pytest.mark.parametrize("name", NAMES)
def test_whole_decode(gpu, oracle, name):
    G.whole_decode(gpu, oracle, 1, name)


@pytest.mark.parametrize("name", NAMES)
def test_single_windows(gpu, oracle, name):
    G.single_windows(gpu, oracle, 1, name)


def test_batched_windows(gpu, oracle):
    G.batched_windows(gpu, oracle, 1)


@pytest.mark.parametrize("fmt", G.TENSOR_FORMATS, ids=G.fmt_id)
def test_tensor_windows(gpu, oracle, fmt):
    G.tensor_windows(gpu, oracle, 1, fmt)


@pytest.mark.parametrize("mode", G.SCALED_MODES, ids=G.fmt_id)
def test_scaled_windows(gpu, oracle, mode):
    G.scaled_windows(gpu, oracle, 1, mode)


@pytest.mark.parametrize("mode", G.SCALED_MODES, ids=G.fmt_id)
def test_resized_windows(gpu, oracle, mode):
    G.resized_windows(gpu, oracle, 1, mode)


def test_error_sums(gpu, oracle):
    G.error_sums(gpu, oracle, 1)


@pytest.mark.parametrize("name", ["v1-rgba-213x211", "v1-rgb-212x216"])
def test_splice(gpu, oracle, name):
    """a crop that cuts through every record class, and the nine tiles of a 3 x 3 cut spliced back: the bytes stream_splice_ref builds from the source's, the crop of
    the oracle's decode, and the source stream again"""
    st = G.by_name(1, name)
    want = Y.decoded(st, oracle)
    W, H = st.W, st.H
    hd = S.parse(st.bytes)[0]
    x, y, w, h = 40, 64, W - 40, 96  # 12 block rows of 22 columns, up to the right edge
    cut = set(np.array(st.classes).reshape(-1, (W + 7) // 8)[y // 8:(y + h) // 8, x // 8:].ravel())
    assert cut == set(Y.CLASSES), cut
    got = gpu.stream_crop(st.bytes, x, y, w, h)
    assert np.array_equal(got, R.crop_bytes(st.bytes, x, y, w, h))
    assert np.array_equal(gpu.decode_stream(got), want[y:y + h, x:x + w])
    pieces = []
    for dby, y0, y1 in ((0, 0, 72), (9, 72, 144), (18, 144, H)):
        for dbx, x0, x1 in ((0, 0, 72), (9, 72, 144), (18, 144, W)):
            tile = gpu.stream_crop(st.bytes, x0, y0, x1 - x0, y1 - y0)
            assert np.array_equal(gpu.decode_stream(tile), want[y0:y1, x0:x1]), (x0, y0)
            pieces.append((tile, 0, 0, dbx, dby, R.blocks(x1 - x0), R.blocks(y1 - y0)))
    back = gpu.stream_splice(pieces, W, H, st.channels == 4, int(hd["errorFactor"]), int(hd["flags"]))
    assert np.array_equal(back, R.splice_bytes(pieces, W, H, st.channels, int(hd["errorFactor"]), int(hd["flags"])))
    assert np.array_equal(back, st.bytes)
    gpu.check()


L.product_twins(globals())
