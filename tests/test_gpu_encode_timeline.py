"""The profiling timeline of every launch path of the 8x8 encode.  limg_hip_profile_end reads the events an encode recorded in groups of four -- bench.py's kernel
intervals are those groups --, so every path must record exactly four per encode (a chain encode over its two phases, a stream encode four more around its packer):
a path that records three or five shifts the intervals of every encode behind it without any error.  Four calls inside one profile_begin / profile_end must give
back 4 x groups encodes -- with 3 or 5 events per call they give 3 or 5 --, every interval finite and >= 0.  The group counts were read from the code and then
recorded on the libraries built from the commit before the timeline became a type (limg_hip::Timeline); they matched.  Bit parity of these paths: test_gpu_parity,
test_gpu_batch, test_gpu_fullsize, test_gpu_collective and the stream modules."""
import numpy as np
import pytest

import lib_axis as L
from lib_axis import lib, lib_product  # noqa: F401  (fixtures: "test" / "product")

pytestmark = pytest.mark.gpu

CALLS = 4


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


@pytest.fixture(scope="module")
def images(oracle):
    """photo-noise RGBA, on the device: (width, height) -> three images"""
    import torch
    cache = {}

    def get(w, h):
        if (w, h) not in cache:
            cache[(w, h)] = [torch.from_numpy(oracle.photo_noise(w, h, seed).view(np.int32)).cuda() for seed in (3, 7, 11)]
        return cache[(w, h)]
    return get


def _single(w, h, planes=True, **options):
    def call(g, images):
        img = images(w, h)[0]
        p = g.alloc_planes_device(w, h) if planes else None
        return options, lambda: g.encode3d_device(img, True, p)
    return call


def _list(n, **options):
    def call(g, images):
        imgs = images(264, 24)[:n]
        planes = [g.alloc_planes_device(264, 24) for _ in imgs]
        return options, lambda: g.encode3d_batch_device(imgs, True, planes)
    return call


def _chain(g, images):
    import torch
    img = images(264, 24)[0]
    planes = g.alloc_planes_device(264, 24)
    calls, base = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")

    def pair():
        g.encode3d_chain_device(img, True, planes, 1, calls=calls)
        g.encode3d_chain_device(img, True, planes, 2, base=base)
    return {}, pair


def _stream(g, images):
    img = images(264, 24)[0]
    return {}, lambda: g.encode_stream_device(img, True, want_size=False)


def _stream_list(g, images):
    imgs = images(264, 24)
    return {}, lambda: g.encode_stream_batch_device(imgs, True, want_sizes=False)


def _stream_list_ef(g, images):
    imgs = images(264, 24)
    return {}, lambda: g.encode_stream_batch_ef_device(imgs, True, (20, 100, 400), want_sizes=False)


def _blocked(g, images):
    img = images(64, 48)[0]
    planes = g.alloc_blocked_planes_device(64, 48)
    return {}, lambda: g.blocked_encode3d_device(img, True, planes)


# (path, the call, groups of four events per call)
PATHS = (
    ("fused", _single(264, 24), 1),                                      # k_fit_tpb first
    ("fused_float_stage_inside", _single(264, 24, legacy_float_stage=True), 1),
    ("split", _single(264, 24, force_split=True), 1),
    ("nothing_stored", _single(264, 24, planes=False), 1),
    ("width_ragged", _single(261, 24), 1),
    ("width_ragged_in_bands", _single(261, 40, ragged_bands=2), 1),
    ("height_ragged", _single(264, 20), 1),
    ("list_in_one_pair", _list(2), 1),
    ("list_as_a_pipeline", _list(3, batch_sub_images=1), 1),
    ("chain_phases", _chain, 1),                                         # per pair of phases
    ("stream", _stream, 2),                                              # the encode, then the packer
    ("stream_list", _stream_list, 2),
    ("stream_list_own_factors", _stream_list_ef, 2),
    ("merged_block_pass_1", _blocked, 1),
)


@pytest.mark.parametrize("path,call,groups", PATHS, ids=[p[0] for p in PATHS])
def test_four_events_per_encode(gpu, images, path, call, groups):
    import torch
    options, encode = call(gpu, images)
    gpu.set_options(**options)
    try:
        encode()  # (whatever the first call of a path grows or builds happens outside the timeline)
        torch.cuda.synchronize()
        gpu.profile_begin()
        for _ in range(CALLS):
            encode()
        torch.cuda.synchronize()
        ms = gpu.profile_end(64)
    finally:
        gpu.set_options()
    print("%s: %d groups from %d calls" % (path, len(ms), CALLS), ms.tolist())
    assert len(ms) == CALLS * groups, (path, len(ms))
    assert np.all(np.isfinite(ms)) and np.all(ms >= 0), (path, ms)
    gpu.check()


L.product_twins(globals())
