"""limg_hip_stream_sizes(_device) and limg_hip_encode_stream_budget(_device): the stream's size probe (k_rate_probe, limg_hip_rate.hip) and the error-factor search on
top of it (limg_hip_rate_step.h), on the smallest shapes that cover the kernel's cases:

  8 x 8               one block: a strip of one block, 31 queue entries past the right edge
  256 x 8             exactly one strip
  264 x 24            two strips per block row, the second of one block; three block rows
  512 x 32 RGB        3 channels: no raw-escape fields
  128 x 256, pool 2   32 block rows of half a strip (the pool only moves the dither chains: sizes do not depend on it)
  203 x 61, 256 x 61  partial edge blocks: no probe kernel, every size is a whole stream encode driven by the same search

Sizes must equal the length of the container's CPU restatement (oracle/stream.py) of the oracle's encode AND of this library's own stream encode; the budget call's
choice, probe count and bytes must equal the algorithm of include/limg_hip.h restated in Python (tests/rate_search.py) over the oracle's sizes, and its stream must be
limg_hip_encode_stream's at the chosen error factor byte for byte."""
import ctypes as C

import numpy as np
import pytest

import lib_axis as L
from lib_axis import lib, lib_product  # noqa: F401  (fixtures: "test" / "product")
from oracle import stream as S
from rate_search import max_probes, oracle_size, restated_search

pytestmark = pytest.mark.gpu


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


# (name, width, height, alpha, pool threads)
SHAPES = (("8x8", 8, 8, True, 0), ("256x8", 256, 8, True, 0), ("264x24", 264, 24, True, 0), ("512x32_rgb", 512, 32, False, 0), ("128x256_pool2", 128, 256, True, 2),
          ("203x61", 203, 61, True, 0), ("256x61", 256, 61, True, 0))
ERROR_FACTORS = (0, 1, 2, 3, 34, 36, 100, 400, 2000, 4000000000)
SEEDS = (3, 7, 11, 13, 17, 19, 23)


@pytest.fixture(scope="module")
def images(oracle):
    """photo-noise and varying-alpha gradient alternate"""
    return {name: (oracle.photo_noise(w, h, SEEDS[k]) if k % 2 == 0 else oracle.random_gradient(w, h, SEEDS[k], False)) for k, (name, w, h, _, _) in enumerate(SHAPES)}


@pytest.fixture(scope="module")
def oracle_streams(oracle, images):
    """{(shape, error factor): the container's CPU restatement of the oracle's encode}, once for both libraries"""
    out = {}
    for name, w, h, alpha, pool in SHAPES:
        for ef in ERROR_FACTORS:
            enc = oracle.encode3d(images[name], alpha, extras=True, error_factor=ef, pool_threads=pool)
            out[name, ef] = S.pack(enc, w, h, 4 if alpha else 3, error_factor=ef)
    return out


def test_sizes_against_the_oracle(gpu, images, oracle_streams):
    saw_escape = False
    for name, w, h, alpha, pool in SHAPES:
        want = [oracle_streams[name, ef].size for ef in ERROR_FACTORS]
        got = gpu.stream_sizes(images[name], alpha, ERROR_FACTORS, pool_threads=pool)
        own = [gpu.encode_stream(images[name], alpha, error_factor=ef, pool_threads=pool).size for ef in ERROR_FACTORS]
        print(name, got)
        assert got == want == own, (name, got, want, own)
        assert want[0] == 64 + 56 * ((w + 7) // 8) * ((h + 7) // 8) * (1 + 0) + 8 * 24 * ((w + 7) // 8) * ((h + 7) // 8), name  # errorFactor 0: every field at 8 bits
        saw_escape |= any(bool((S.parse(oracle_streams[name, ef])[1]["shift"] >> 24).any()) for ef in ERROR_FACTORS)
    assert saw_escape, "no raw-escape field in any stream: the probe's alpha-lane rule was not exercised"
    assert gpu.stream_sizes(images["8x8"], True, []) == []


def _budget_case(gpu, img, alpha, pool, size, budget, lo_ef, hi_ef, ctx, **kw):
    """one budget call against the restated search over size(h); lo_ef / hi_ef as handed to the call (0: the defaults)"""
    h_lo, h_hi = (lo_ef or 2) // 2, (hi_ef or 1024) // 2
    want_h, within, asked, nbytes = restated_search(size, h_lo, h_hi, budget)
    st, res = gpu.encode_stream_budget(img, alpha, budget, lo_ef, hi_ef, pool_threads=pool, **kw)
    print(ctx, budget, (res.errorFactor, res.withinBudget, res.probes, res.bytes), (2 * want_h, within, asked, nbytes))
    assert (res.errorFactor, res.withinBudget, res.probes, res.bytes) == (2 * want_h, within, len(asked), nbytes), (ctx, budget)
    assert res.probes <= max_probes(h_lo, h_hi) and st.size == res.bytes, (ctx, budget)
    assert not within or res.bytes <= budget, (ctx, budget)
    assert np.array_equal(st, gpu.encode_stream(img, alpha, error_factor=res.errorFactor, pool_threads=pool, **kw)), (ctx, budget)
    return res


def test_budget_against_the_restated_search(gpu, oracle, images):
    outcomes = set()
    for name, w, h, alpha, pool in SHAPES:
        memo = {}

        def size(hh, name=name, alpha=alpha, memo=memo):
            if hh not in memo:
                memo[hh] = oracle_size(oracle, images[name], alpha, 2 * hh)
            return memo[hh]

        for lo_ef, hi_ef in ((2, 128), (0, 0)) if name == "264x24" else ((2, 128),):
            top, bottom = size((lo_ef or 2) // 2), size((hi_ef or 1024) // 2)
            assert bottom < top, name
            for budget in (bottom - 8, bottom, top, top + 8, top - 8, (top + bottom) // 2, size(((lo_ef or 2) + (hi_ef or 1024)) // 4)):
                res = _budget_case(gpu, images[name], alpha, pool, size, budget, lo_ef, hi_ef, (name, lo_ef, hi_ef))
                outcomes.add("refused" if not res.withinBudget else ("lo" if res.errorFactor == (lo_ef or 2) else "bisected"))
    assert outcomes == {"refused", "lo", "bisected"}


def test_budget_on_the_non_monotone_gradient(gpu, oracle):
    """256 x 32 opaque gradient as RGB: 10264 bytes at errorFactor 34, 10280 at 36, 10304 from 66 on -- 10270 is refused over [2, 256] and met over [2, 34]"""
    img = oracle.random_gradient(256, 32, 5, True)
    size = lambda hh: oracle_size(oracle, img, False, 2 * hh)  # noqa: E731
    assert gpu.stream_sizes(img, False, (34, 36, 66, 256)) == [10264, 10280, 10304, 10304]
    res = _budget_case(gpu, img, False, 0, size, 10270, 2, 256, "gradient [2, 256]")
    assert (res.errorFactor, res.withinBudget, res.probes) == (256, 0, 1)
    res = _budget_case(gpu, img, False, 0, size, 10270, 2, 34, "gradient [2, 34]")
    assert res.withinBudget == 1 and res.bytes <= 10270


def test_options(gpu, oracle, images):
    img = images["264x24"]
    efs = (0, 2, 34, 100, 400, 2000)

    def own_size(hh, **kw):
        return gpu.encode_stream(img, True, error_factor=2 * hh, **kw).size

    # FAST float mode: no bit-exact oracle -- the library's own FAST stream encode is the reference
    gpu.set_options(float_fast=True)
    try:
        want = [gpu.encode_stream(img, True, error_factor=ef).size for ef in efs]
        assert gpu.stream_sizes(img, True, efs) == want
        for budget in (want[3], (want[1] + want[5]) // 2):
            _budget_case(gpu, img, True, 0, own_size, budget, 2, 128, "float_fast")
    finally:
        gpu.set_options()
    # a forced shift triple: a flat curve -- the search returns the lower bound or refuses
    gpu.set_options(forced_shift=(7, 8, 1))
    try:
        flat = gpu.encode_stream(img, True, error_factor=100).size
        assert gpu.stream_sizes(img, True, efs) == [flat] * len(efs)
        res = _budget_case(gpu, img, True, 0, lambda hh: flat, flat, 2, 128, "forced, fits")
        assert (res.errorFactor, res.withinBudget, res.probes) == (2, 1, 2)
        res = _budget_case(gpu, img, True, 0, lambda hh: flat, flat - 8, 2, 128, "forced, refused")
        assert (res.errorFactor, res.withinBudget, res.probes) == (128, 0, 1)
    finally:
        gpu.set_options()
    plain = [oracle_size(oracle, img, True, ef) for ef in efs]
    # PCG dither: other streams, the same sizes
    gpu.set_options(dither_pcg=True)
    try:
        assert gpu.stream_sizes(img, True, efs) == plain
        _budget_case(gpu, img, True, 0, lambda hh: oracle_size(oracle, img, True, 2 * hh), (plain[1] + plain[5]) // 2, 2, 128, "pcg")
    finally:
        gpu.set_options()
    # the accurate search has no probe kernel: whole stream encodes, the same search
    accurate = [oracle_size(oracle, img, True, ef, fast=False) for ef in efs]
    assert gpu.stream_sizes(img, True, efs, fast=False) == accurate
    _budget_case(gpu, img, True, 0, lambda hh: oracle_size(oracle, img, True, 2 * hh, fast=False), (accurate[1] + accurate[5]) // 2, 2, 128, "accurate", fast=False)
    # ... nor has the split path
    gpu.set_options(force_split=True)
    try:
        assert gpu.stream_sizes(img, True, efs) == plain
    finally:
        gpu.set_options()
    # test build: the probe's generic 32-bit search (records beyond the packed trial's range) against the encode's, as tests/test_gpu_parity.py::test_generic_trial_path
    if L.has_hooks(gpu):
        for limit in (1, 120):
            gpu.set_options(test_record_limit=limit)
            try:
                assert gpu.stream_sizes(img, True, efs) == plain == [gpu.encode_stream(img, True, error_factor=ef).size for ef in efs], limit
            finally:
                gpu.set_options()


def test_device_forms_and_back_to_back(gpu, oracle, images):
    """torch tensors; two budget calls of different shapes on one stream, then a plain stream encode: the probe's state disturbs neither"""
    import torch
    a, b = images["264x24"], images["128x256_pool2"]
    sizes_a = [oracle_size(oracle, a, True, ef) for ef in (2, 100, 128)]
    want_b = gpu.encode_stream(b, True, error_factor=100)
    da, db = (torch.from_numpy(i.view(np.int32)).cuda() for i in (a, b))
    torch.cuda.synchronize()
    assert gpu.stream_sizes_device(da, True, (2, 100, 128)) == sizes_a
    budget = (sizes_a[0] + sizes_a[2]) // 2
    oa, ra = gpu.encode_stream_budget_device(da, True, budget, 2, 128)
    ob, rb = gpu.encode_stream_budget_device(db, True, want_b.size, 2, 128)
    plain, n = gpu.encode_stream_device(db, True, error_factor=100)
    torch.cuda.synchronize()
    gpu.check()
    want_h, within, asked, nbytes = restated_search(lambda hh: oracle_size(oracle, a, True, 2 * hh), 1, 64, budget)
    assert (ra.errorFactor, ra.withinBudget, ra.probes, ra.bytes) == (2 * want_h, within, len(asked), nbytes)
    assert np.array_equal(oa[:ra.bytes].cpu().numpy(), gpu.encode_stream(a, True, error_factor=ra.errorFactor))
    assert rb.withinBudget == 1 and rb.bytes <= want_b.size
    assert np.array_equal(ob[:rb.bytes].cpu().numpy(), gpu.encode_stream(b, True, error_factor=rb.errorFactor))
    assert n == want_b.size and np.array_equal(plain[:n].cpu().numpy(), want_b)


def test_probe_on_a_misaligned_image(gpu, images):
    """The probe's dword-load path.  Its domain is whole blocks, so the width is always a multiple of 4 and only an image that starts 4-byte but not 16-byte aligned
    takes it: the pixels of the 264 x 24 image at element 1 of a tensor one element longer.  Sizes, the search's result and the stream must be exactly those of the
    aligned tensor, which the tests above tie to the oracle."""
    import torch
    img = images["264x24"]
    aligned = torch.from_numpy(img.view(np.int32)).cuda()
    moved = torch.empty(img.size + 1, dtype=torch.int32, device="cuda")[1:].view(24, 264)
    moved.copy_(aligned)
    assert aligned.data_ptr() % 16 == 0 and moved.data_ptr() % 16 == 4 and moved.is_contiguous()
    efs = [2, 100, 1024]
    want = gpu.stream_sizes_device(aligned, True, efs)
    got = gpu.stream_sizes_device(moved, True, efs)
    print(want, got)
    assert got == want and want[2] < want[0]
    budget = (want[0] + want[2]) // 2
    oa, ra = gpu.encode_stream_budget_device(aligned, True, budget)
    ob, rb = gpu.encode_stream_budget_device(moved, True, budget)
    torch.cuda.synchronize()
    gpu.check()
    ta, tb = ((r.errorFactor, r.withinBudget, r.probes, r.bytes) for r in (ra, rb))
    print(budget, ta, tb)
    assert tb == ta and ra.withinBudget == 1 and ra.probes > 2 and 2 < ra.errorFactor <= 1024, "a bisected budget"
    assert torch.equal(ob[:rb.bytes], oa[:ra.bytes])


def test_errors(gpu):
    """the contract's refusals, in its order, each before anything touches the device: the output buffer keeps its pattern, the result its values"""
    import torch
    W, H = 64, 16
    bound = gpu.stream_bound(W, H)
    img = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    room = torch.full((bound + 256,), 0x5A, dtype=torch.uint8, device="cuda")
    assert room.data_ptr() % 16 == 0
    res = limg_result()
    dev, host = gpu.lib.limg_hip_encode_stream_budget_device, gpu.lib.limg_hip_encode_stream_budget
    NULL_, INVALID, BOUNDS = 102, 101, 103  # limg_hip_error_ArgumentNull, _InvalidParameter, _OutOfBounds

    def call(ctx=gpu.ctx, pin=img.data_ptr(), w=W, h=H, pout=room.data_ptr(), cap=bound, max_bytes=5000, lo=0, hi=0, pres=C.byref(res)):
        return dev(ctx, pin, w, h, 1, pout, cap, max_bytes, lo, hi, 0, 1, pres, None)

    assert call(ctx=None) == NULL_ and call(pin=None) == NULL_ and call(pout=None) == NULL_ and call(pres=None) == NULL_
    assert call(w=0) == INVALID and call(h=0) == INVALID and call(w=1 << 31) == INVALID
    assert call(cap=bound - 1) == BOUNDS
    assert call(pout=room.data_ptr() + 8) == INVALID
    for bad in ({"lo": 3}, {"hi": 101}, {"lo": 1}, {"hi": 1}, {"lo": 200, "hi": 100}, {"lo": 2000}, {"max_bytes": 0}):
        assert call(**bad) == INVALID, bad
    short = limg_result()
    short.struct_size = 16
    assert call(pres=C.byref(short)) == INVALID
    assert call(w=0, cap=0) == INVALID and call(cap=bound - 1, pout=room.data_ptr() + 8) == BOUNDS and call(cap=bound - 1, max_bytes=0) == BOUNDS  # the order
    host_img, host_out = np.zeros((H, W), dtype=np.uint32), np.full(bound, 0x5A, dtype=np.uint8)
    hp, ho = host_img.ctypes.data, host_out.ctypes.data
    assert host(None, hp, W, H, 1, ho, bound, 5000, 0, 0, 0, 1, C.byref(res)) == NULL_
    assert host(gpu.ctx, hp, W, H, 1, ho, bound, 5000, 0, 0, 0, 1, None) == NULL_
    assert host(gpu.ctx, hp, 0, H, 1, ho, bound, 5000, 0, 0, 0, 1, C.byref(res)) == INVALID
    assert host(gpu.ctx, hp, W, H, 1, ho, bound, 0, 0, 0, 0, 1, C.byref(res)) == INVALID
    assert host(gpu.ctx, hp, W, H, 1, ho, bound, 5000, 4, 2, 0, 1, C.byref(res)) == INVALID
    # the sizes entries
    efs, sizes = (C.c_uint32 * 2)(0, 100), (C.c_size_t * 2)(77, 77)
    sdev, shost = gpu.lib.limg_hip_stream_sizes_device, gpu.lib.limg_hip_stream_sizes
    assert sdev(None, img.data_ptr(), W, H, 1, efs, 2, sizes, 0, 1, None) == NULL_ and sdev(gpu.ctx, None, W, H, 1, efs, 2, sizes, 0, 1, None) == NULL_
    assert sdev(gpu.ctx, img.data_ptr(), W, H, 1, None, 2, sizes, 0, 1, None) == NULL_ and sdev(gpu.ctx, img.data_ptr(), W, H, 1, efs, 2, None, 0, 1, None) == NULL_
    assert sdev(gpu.ctx, img.data_ptr(), 0, H, 1, efs, 2, sizes, 0, 1, None) == INVALID and shost(gpu.ctx, hp, W, 0, 1, efs, 2, sizes, 0, 1) == INVALID
    assert shost(None, hp, W, H, 1, efs, 2, sizes, 0, 1) == NULL_
    assert sdev(gpu.ctx, img.data_ptr(), W, H, 1, efs, 0, sizes, 0, 1, None) == 0 and shost(gpu.ctx, hp, W, H, 1, efs, 0, sizes, 0, 1) == 0
    torch.cuda.synchronize()
    assert int((room != 0x5A).sum()) == 0 and int((host_out != 0x5A).sum()) == 0, "a refused call wrote to an output buffer"
    assert (res.errorFactor, res.probes, res.withinBudget, res.bytes) == (7, 7, 7, 7) and list(sizes) == [77, 77], "a refused call wrote a result"
    # the context is usable, and the same arguments are accepted: a flat image has one size from errorFactor 2 on, so the lower bound is the answer after two probes
    flat = [gpu.encode_stream(host_img, True, error_factor=ef).size for ef in (0, 100, 2)]
    assert call() == 0 and (res.errorFactor, res.withinBudget, res.probes, res.bytes) == (2, 1, 2, flat[2]) and flat[1] == flat[2] <= 5000
    assert sdev(gpu.ctx, img.data_ptr(), W, H, 1, efs, 2, sizes, 0, 1, None) == 0 and list(sizes) == flat[:2]
    gpu.check()


def limg_result():
    import limg_amd
    r = limg_amd.BudgetResult(C.sizeof(limg_amd.BudgetResult), 7, 7, 7, 7)
    return r


def test_context_device_bytes(lib):
    """the probe's state, its counter and a sizes list's 12 bytes per entry are context memory the context reports"""
    import limg_amd
    g = L.open_context(lib)
    try:
        img = g.synth_device("photo_noise", 264, 24, seed=5)
        g.encode_stream_device(img, True)
        before = g.device_bytes()
        g.encode_stream_budget_device(img, True, 20000, 2, 128)
        state = 48 + 24  # RateState, then RateDevice's list position and thresholds
        assert C.sizeof(limg_amd.BudgetResult) == 24 and state + 8 <= g.device_bytes() - before < state + 8 + 256, (before, g.device_bytes())
        before = g.device_bytes()
        g.stream_sizes_device(img, True, list(range(0, 200, 2)))
        assert g.device_bytes() - before == 12 * 100, (before, g.device_bytes())
        g.check()
    finally:
        g.close()


L.product_twins(globals())  # test_x_product: the same tests on the product library (tests/lib_axis.py)
