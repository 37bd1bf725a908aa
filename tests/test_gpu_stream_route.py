"""The route a stream-encode list takes (limg_hip_list_plan.h: list_route), as far as a GPU run can see it.  Every route gives the same bytes by contract, so the
other stream modules cannot tell a wrong route from the right one; what does differ is the number of four-event groups a call leaves on the profiling timeline: 2
per stream-encode step (the encode, then its packer), 1 more per probe grid (the float stage of a size probe).  tests/test_list_plan_cpu.py checks the plan itself,
exhaustively and without a GPU; this module checks that the walkers do what the plan says, in the form of tests/test_gpu_encode_timeline.py: one warm-up call, four
calls inside profile_begin / profile_end, the number of groups per call, every interval finite and >= 0, and a clean device status.  The counts were recorded on the
libraries built from the commit before the route became a plan; they are what the plan's steps give (ROWS names the steps).  Only eligible items where a probe is
involved: an ineligible item's search encodes once per size it asks for, which depends on the data."""
import numpy as np
import pytest

import lib_axis as L
from lib_axis import lib, lib_product  # noqa: F401  (fixtures: "test" / "product")
from budget_list_cases import LISTS

pytestmark = pytest.mark.gpu

CALLS = 4
EDGES = LISTS["edges"][1]
RAGGED_INSIDE = LISTS["ragged_inside"][1]
SAME = ((264, 24),)


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
    """photo-noise RGBA on the device: shapes -> one image per shape, image i from seed 3 + 4 i"""
    import torch
    cache = {}

    def get(shapes):
        for i, (w, h) in enumerate(shapes):
            if (w, h, i) not in cache:
                cache[(w, h, i)] = torch.from_numpy(oracle.photo_noise(w, h, 3 + 4 * i).view(np.int32)).cuda()
        return [cache[(w, h, i)] for i, (w, h) in enumerate(shapes)]
    return get


def _factors(n):
    return [(20, 100, 400, 50, 2, 200, 1000)[i % 7] for i in range(n)]


def _list(shapes, factors=None, fast=True):
    return lambda g, imgs: g.encode_stream_list_device(imgs, True, factors or _factors(len(shapes)), want_sizes=False, fast=fast)


def _batch_ef(factors, fast=True):
    return lambda g, imgs: g.encode_stream_batch_ef_device(imgs, True, factors, want_sizes=False, fast=fast)


def _batch(g, imgs):
    return g.encode_stream_batch_device(imgs, True, want_sizes=False)


def _budget_batch(g, imgs):
    return g.encode_stream_budget_batch_device(imgs, True, 11500, 2, 128)


def _budget_list(g, imgs):
    return g.encode_stream_budget_list_device(imgs, True, 16000, 2, 128)


def _sizes_list(g, imgs):
    return g.stream_sizes_list_device(imgs, True, (0, 37, 400))


# (row, shapes, the call, options, groups of four events per call, the steps behind them)
ROWS = (
    ("list_edges", EDGES, _list(EDGES), {}, 2, "one mixed chunk"),
    ("list_edges_chunks_of_3", EDGES, _list(EDGES), {"test_batch_chunk": 3}, 6, "mixed 3 + mixed 3 + single"),
    ("list_ragged_inside", RAGGED_INSIDE, _list(RAGGED_INSIDE), {}, 6, "mixed chunk of the two eligible items, then the two others as singles"),
    ("list_one_shape", SAME * 3, _list(SAME * 3, (20, 100, 400)), {}, 2, "one same-shape chunk at own factors"),
    ("list_one_shape_accurate", SAME * 3, _list(SAME * 3, (20, 100, 400), fast=False), {}, 6, "nothing eligible: three singles"),
    ("batch_ef_accurate_two_equal", SAME * 3, _batch_ef((20, 20, 400), fast=False), {}, 4, "sorted by factor: a shared-factor chunk of two, a single"),
    ("batch_ef_split_two_equal", SAME * 3, _batch_ef((20, 20, 400)), {"force_split": True}, 6, "sorted by factor, no launch pair: three singles"),
    ("batch_chunks_of_3", SAME * 4, _batch, {"test_batch_chunk": 3}, 4, "chunk of three, then a last chunk of one as a single"),
    ("budget_batch_chunks_of_2", SAME * 5, _budget_batch, {"test_batch_chunk": 2}, 9, "(probe grid + chunk) x 2, then the single budget call: probe grid + encode"),
    ("budget_list_edges", EDGES, _budget_list, {}, 3, "probe grid + one mixed chunk"),
    ("budget_list_edges_chunks_of_3", EDGES, _budget_list, {"test_batch_chunk": 3}, 9, "(probe grid + mixed chunk) x 2, then the single budget call"),
    ("sizes_list_edges", EDGES, _sizes_list, {}, 1, "one probe grid"),
    ("sizes_list_edges_chunks_of_3", EDGES, _sizes_list, {"test_batch_chunk": 3}, 3, "probe grid x 2, then the single sizes call: one probe grid"),
)


@pytest.mark.parametrize("row,shapes,call,options,groups,steps", ROWS, ids=[r[0] for r in ROWS])
def test_groups_per_call(gpu, images, row, shapes, call, options, groups, steps):
    import torch
    if any(k.startswith("test_") for k in options) and not L.has_hooks(gpu):
        return  # images per chunk: a test hook
    imgs = images(shapes)
    gpu.set_options(**options)
    try:
        call(gpu, imgs)  # (whatever the first call of a route grows or builds happens outside the timeline)
        torch.cuda.synchronize()
        gpu.profile_begin()
        for _ in range(CALLS):
            call(gpu, imgs)
        torch.cuda.synchronize()
        ms = gpu.profile_end(64)
    finally:
        gpu.set_options()
    print("%s: %d groups from %d calls (%s)" % (row, len(ms), CALLS, steps), ms.tolist())
    assert len(ms) == CALLS * groups, (row, len(ms), steps)
    assert np.all(np.isfinite(ms)) and np.all(ms >= 0), (row, ms)
    gpu.check()


L.product_twins(globals())
