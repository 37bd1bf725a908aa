"""Both shift-search automata on the GPU, on the inputs that tests/test_search_tables.py proves to reach every class of their edges (tests/search_table_inputs.py):
  test_accurate_corpus          the accurate search's table walk (search_accurate_automaton) in all four float / launch modes of the E step, 3 and 4 channels
  test_partial_blocks           508x61 crops through the host entry: the FULL == false walk from the root of the default and of the accurate table
  test_default_corpus           the default search on its corpus, incl. the found blocks that take the table's rarest edges outside the hot subtree
  test_generic_trial_accurate   (test build) the literal loops behind the generic 32-bit trial on the accurate corpus
  test_merged_block_accurate    the literal loops of the merged-block encoder: every written plane and the rectangle list
on the test build and on the product library, shifts first (they name the block), then every plane bit-identical to the oracle."""
import numpy as np
import pytest

import lib_axis as L
from lib_axis import lib, lib_product  # noqa: F401  (fixtures: "test" / "product")
import search_table_inputs as inputs
from oracle.bind import BLOCKED_WRITTEN, PLANES

pytestmark = pytest.mark.gpu
MODES = {"fused": {}, "split": dict(force_split=True), "legacy": dict(legacy_float_stage=True), "split_legacy": dict(force_split=True, legacy_float_stage=True)}


@pytest.fixture(scope="module")
def wanted_accurate(oracle):
    """[(name, image, has_alpha, errorFactor, the oracle's accurate encode)], computed once for every mode and both libraries"""
    return [(name, img, alpha, ef, oracle.encode3d(img, alpha, extras=True, fast=False, error_factor=ef)) for name, img, alpha, ef in inputs.accurate_inputs(oracle)]


@pytest.fixture(scope="module")
def wanted_default(oracle):
    return [(name, img, alpha, ef, oracle.encode3d(img, alpha, extras=True, error_factor=ef)) for name, img, alpha, ef in inputs.default_inputs(oracle)]


@pytest.fixture(scope="module")
def wanted_partial(oracle):
    """{fast: [(name, image, has_alpha, errorFactor, the oracle's encode)]}"""
    return {fast: [(name, img, alpha, ef, oracle.encode3d(img, alpha, extras=True, fast=fast, error_factor=ef))
                   for name, img, ef in inputs.partial_inputs(oracle) for alpha in (True, False)] for fast in (True, False)}


@pytest.fixture(scope="module")
def wanted_blocked(oracle):
    return [(name, img, alpha, ef, oracle.blocked_encode3d(img, alpha, fast=False, error_factor=ef)) for name, img, alpha, ef in inputs.blocked_inputs(oracle)]


def _check(got, shifts, want, ctx):
    if shifts is not None:
        for i in range(3):
            g, w = (shifts >> (8 * i)) & 0xFF, want["shifts"][:, :, i]
            assert np.array_equal(g, w), (ctx, "shift", "ABC"[i], "blocks", np.argwhere(g != w)[:6].tolist(), g[g != w][:6].tolist(), w[g != w][:6].tolist())
    bad = [(k, int((got[k] != want[k]).sum()), np.argwhere(got[k] != want[k])[:3].tolist()) for k in PLANES if not np.array_equal(got[k], want[k])]
    assert len(PLANES) == 11 and not bad, (ctx, bad)


def _device_corpus(g, wanted, fast, ctx):
    import torch
    for name, img, alpha, ef, want in wanted:
        h, w = img.shape
        assert w % 8 == 0 and h % 8 == 0
        planes = g.alloc_planes_device(w, h)
        sh = torch.zeros((h // 8) * (w // 8), dtype=torch.int32, device="cuda")
        g.encode3d_device(torch.from_numpy(img.view(np.int32)).cuda(), alpha, planes, error_factor=ef, fast=fast, shifts=sh)
        torch.cuda.synchronize()
        got = {k: v.cpu().numpy().view(np.uint32 if v.dtype == torch.int32 else np.uint8) for k, v in planes.items()}
        _check(got, sh.cpu().numpy().astype(np.uint32).reshape(h // 8, w // 8), want, (name,) + ctx)


@pytest.mark.parametrize("mode", list(MODES))
def test_accurate_corpus(lib, wanted_accurate, mode):
    g = L.open_context(lib)
    try:
        g.set_options(**MODES[mode])
        _device_corpus(g, wanted_accurate, False, (mode, lib))
        g.check()
    finally:
        g.close()


@pytest.mark.parametrize("mode", ["fused", "split"])
def test_default_corpus(lib, wanted_default, mode):
    g = L.open_context(lib)
    try:
        g.set_options(**MODES[mode])
        _device_corpus(g, wanted_default, True, (mode, lib))
        g.check()
    finally:
        g.close()


@pytest.mark.parametrize("fast", [True, False], ids=["default", "accurate"])
def test_partial_blocks(lib, wanted_partial, fast):
    g = L.open_context(lib)
    try:
        for name, img, alpha, ef, want in wanted_partial[fast]:
            _check(g.encode3d(img, alpha, error_factor=ef, fast=fast), None, want, (name, alpha, fast, lib))
        g.check()
    finally:
        g.close()


def test_generic_trial_accurate(lib, wanted_accurate):
    """test_record_limit = 1 sends every block through the generic 32-bit trial: search_generic -> the literal loops search_accurate (limg_hip_device.h)"""
    g = L.open_context(lib)
    try:
        g.set_options(test_record_limit=1)
        _device_corpus(g, wanted_accurate, False, ("generic", lib))
        g.check()
    finally:
        g.close()


def test_merged_block_accurate(lib, wanted_blocked):
    g = L.open_context(lib)
    try:
        for name, img, alpha, ef, want in wanted_blocked:
            got = g.blocked_encode3d(img, alpha, error_factor=ef, fast=False)
            wr, gr = want["regions"], got["regions"]
            assert len(wr) == len(gr), (name, len(wr), len(gr))
            for f in ("ox", "oy", "rx", "ry"):
                assert np.array_equal(wr[f], gr[f]), (name, f, np.argwhere(wr[f] != gr[f])[:4].ravel())
            bad = [(k, int((got[k] != want[k]).sum()), np.argwhere(got[k] != want[k])[:3].tolist()) for k in BLOCKED_WRITTEN if not np.array_equal(got[k], want[k])]
            assert not bad, (name, lib, bad)
        g.check()
    finally:
        g.close()


L.product_twins(globals())
