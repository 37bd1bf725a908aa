"""The version 2 decoders on hand-built streams (tests/synthetic_streams.py): the whole k_bstream_* family -- the full decode, the single and batched windows and their
tensor, scaled, resized and error forms -- on rectangle tilings no encoder made: more than 64 rectangles in shuffled table order, single blocks, strips along a whole
grid side, a rectangle of 72 blocks, rectangles with rx, ry > 1 on the clipped edges, fields whose pixels straddle 64-bit words at any bit offset (widths that are
no multiple of 8), any int16 record, every shift triple.  Each result equals the ORACLE's decode of the same bytes, bit for bit, through the shared bodies of the
window tests; each test ends with a clean check() and zero job status words."""
import pytest

import lib_axis as L
import synthetic_gpu as G

pytestmark = pytest.mark.gpu
NAMES = G.NAMES[2]


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
    G.whole_decode(gpu, oracle, 2, name)


@pytest.mark.parametrize("name", NAMES)
def test_single_windows(gpu, oracle, name):
    G.single_windows(gpu, oracle, 2, name)


def test_batched_windows(gpu, oracle):
    G.batched_windows(gpu, oracle, 2)


@pytest.mark.parametrize("fmt", G.TENSOR_FORMATS, ids=G.fmt_id)
def test_tensor_windows(gpu, oracle, fmt):
    G.tensor_windows(gpu, oracle, 2, fmt)


@pytest.mark.parametrize("mode", G.SCALED_MODES, ids=G.fmt_id)
def test_scaled_windows(gpu, oracle, mode):
    G.scaled_windows(gpu, oracle, 2, mode)


@pytest.mark.parametrize("mode", G.SCALED_MODES, ids=G.fmt_id)
def test_resized_windows(gpu, oracle, mode):
    G.resized_windows(gpu, oracle, 2, mode)


def test_error_sums(gpu, oracle):
    G.error_sums(gpu, oracle, 2)


L.product_twins(globals())
