"""limg_hip_encode_stream_budget_batch(_device): a list of same-shape images, each to its own byte budget, in one call -- the records of the list from one float-stage
grid, one search state per image, the probes of all images in the same launches (k_rate_begin_batch / k_rate_probe_batch / k_rate_step_batch, limg_hip_rate.hip), one
wait, then one stream encode per distinct error factor.

Result i must be what the single budget call gives for image i: the choice, probe count and bytes must equal the algorithm of include/limg_hip.h restated in Python
(tests/rate_search.py) over the ORACLE's sizes, the stream must be limg_hip_encode_stream's at the chosen error factor byte for byte, and its header's totalBytes the
reported bytes.  The shapes are the smallest that reach each way the list kernels can go wrong:

  5 x 264 x 24 RGBA   two strips per block row, the second of one block, three block rows: six workgroups per image (no power of two); five contents whose searches
                      end three different ways with five different answers -- a probe that mixes up image index, record slice, state or counter cannot pass
  3 x 8 x 8           one workgroup per image, 31 empty queue entries
  66 x 8 x 8          more images than one k_rate_begin_batch launch (64) or one table launch (32) carries, and a second workgroup of k_rate_step_batch
  3 x 512 x 32 RGB    3 channels: no raw-escape fields
  2 x 128 x 256       pool_threads = 2 (the pool only moves the dither chains)
  the same image twice, two budgets, two buffers
  3 x 203 x 61        partial edge blocks: no probe kernel, the loop of single calls"""
import ctypes as C

import numpy as np
import pytest

import lib_axis as L
import limg_amd
from lib_axis import lib, lib_product  # noqa: F401  (fixtures: "test" / "product")
from rate_search import max_probes, oracle_size, restated_search

pytestmark = pytest.mark.gpu

W, H = 264, 24
STATE_BYTES = 72 + 8  # include/limg_hip.h: sizeof RateDevice + the counter, per image of the longest chunk


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


class Sizes:
    """size(h) of one image on the CPU oracle, every value computed once for the whole module"""

    def __init__(self, oracle, img, alpha):
        self.oracle, self.img, self.alpha, self.memo = oracle, img, alpha, {}

    def __call__(self, h):
        if h not in self.memo:
            self.memo[h] = oracle_size(self.oracle, self.img, self.alpha, 2 * h)
        return self.memo[h]


@pytest.fixture(scope="module")
def five(oracle):
    """the list of the issue: photo-noise 3, gradient 7 (varying alpha), photo-noise 11, opaque gradient 13, photo-noise 17 -- and the oracle's size function of each"""
    imgs = [oracle.photo_noise(W, H, 3), oracle.random_gradient(W, H, 7, False), oracle.photo_noise(W, H, 11), oracle.random_gradient(W, H, 13, True),
            oracle.photo_noise(W, H, 17)]
    return imgs, [Sizes(oracle, i, True) for i in imgs]


def _tuple(r):
    return (r.errorFactor, r.withinBudget, r.probes, r.bytes)


def _outcome(r, lo_ef):
    return "refused" if not r.withinBudget else ("lo" if r.errorFactor == (lo_ef or 2) else "bisected")


def _check(gpu, imgs, alpha, budgets, lo_ef, hi_ef, sizes, ctx, pool=0, singles=True, call=None, **kw):
    """one list call against the restated search over sizes[i](h); lo_ef / hi_ef as handed to the call (0: the defaults).  sizes[i] None: the single call is the
    reference of the search (what the issue sets for the fallbacks and FAST float mode).  -> the results"""
    h_lo, h_hi = (lo_ef or 2) // 2, (hi_ef or 1024) // 2
    n = len(imgs)
    budgets = [budgets] * n if np.isscalar(budgets) else list(budgets)
    streams, results = (call or gpu.encode_stream_budget_batch)(imgs, alpha, budgets if len(set(budgets)) > 1 else budgets[0], lo_ef, hi_ef, pool_threads=pool, **kw)
    assert len(streams) == len(results) == n, ctx
    for i in range(n):
        res, st = results[i], streams[i]
        if sizes[i] is not None:
            want_h, within, asked, nbytes = restated_search(sizes[i], h_lo, h_hi, budgets[i])
            print(ctx, i, budgets[i], _tuple(res), (2 * want_h, within, len(asked), nbytes))
            assert _tuple(res) == (2 * want_h, within, len(asked), nbytes), (ctx, i, budgets[i])
        assert res.probes <= max_probes(h_lo, h_hi) and (not res.withinBudget or res.bytes <= budgets[i]), (ctx, i)
        assert st.size == res.bytes == limg_amd.stream_info(st, gpu.lib)[3], (ctx, i, st.size, res.bytes)
        want = gpu.encode_stream(imgs[i], alpha, error_factor=res.errorFactor, pool_threads=pool, **kw)
        assert st.size == want.size and np.array_equal(st, want), (ctx, i, "the stream is not encode_stream's at the chosen error factor")
        if singles:
            one_st, one = gpu.encode_stream_budget(imgs[i], alpha, budgets[i], lo_ef, hi_ef, pool_threads=pool, **kw)
            assert _tuple(res) == _tuple(one) and np.array_equal(st, one_st), (ctx, i, _tuple(res), _tuple(one))
    return results


def test_one_budget_three_outcomes(gpu, five):
    """a common budget of 11500 over [2, 128]: bisected, refused, bisected, met at the lower bound, bisected -- in ONE call, five different answers"""
    imgs, sizes = five
    results = _check(gpu, imgs, True, 11500, 2, 128, sizes, "five")
    assert {_outcome(r, 2) for r in results} == {"refused", "lo", "bisected"}, [_tuple(r) for r in results]
    assert len({_tuple(r) for r in results}) == 5, [_tuple(r) for r in results]


@pytest.mark.parametrize("bounds", [(2, 128), (0, 0)], ids=["2_128", "defaults"])
def test_per_image_budgets(gpu, five, bounds):
    """bottom - 8, top, the middle, top + 8, bottom -- one per image; the default bounds [2, 1024] reach the largest launch count"""
    imgs, sizes = five
    lo_ef, hi_ef = bounds
    budgets = []
    for i, size in enumerate(sizes):
        top, bottom = size((lo_ef or 2) // 2), size((hi_ef or 1024) // 2)
        assert bottom < top
        budgets.append((bottom - 8, top, (top + bottom) // 2, top + 8, bottom)[i])
    results = _check(gpu, imgs, True, budgets, lo_ef, hi_ef, sizes, ("per image", bounds))
    assert {_outcome(r, lo_ef) for r in results} == {"refused", "lo", "bisected"}


@pytest.mark.parametrize("shape", ["8x8", "66x8x8", "512x32_rgb", "128x256_pool2", "twice"])
def test_other_shapes(gpu, oracle, five, shape):
    if shape == "twice":  # the same image twice in one list: two budgets, two output buffers
        imgs, sizes = [five[0][0], five[0][0]], [five[1][0], five[1][0]]
        top, bottom = sizes[0](1), sizes[0](64)
        results = _check(gpu, imgs, True, [(top + bottom) // 2, (top + 3 * bottom) // 4], 2, 128, sizes, shape)
        assert results[0].errorFactor != results[1].errorFactor
        return
    w, h, n, alpha, pool = {"8x8": (8, 8, 3, True, 0), "66x8x8": (8, 8, 66, True, 0), "512x32_rgb": (512, 32, 3, False, 0), "128x256_pool2": (128, 256, 2, True, 2)}[shape]
    imgs = [oracle.photo_noise(w, h, 3 + 4 * i) if i % 2 == 0 else oracle.random_gradient(w, h, 3 + 4 * i, False) for i in range(n)]
    sizes = [Sizes(oracle, i, alpha) for i in imgs]
    budgets = [((s(1) + s(64)) // 2, s(64) - 8, s(1))[i % 3] for i, s in enumerate(sizes)]
    _check(gpu, imgs, alpha, budgets, 2, 128, sizes, shape, pool=pool, singles=n < 10)


def test_chunks(gpu, five):
    """test hook: 2 images per chunk => 2 + 2 + 1, the last through the single call; the results are those of the one-chunk call"""
    if not L.has_hooks(gpu):
        return
    imgs, sizes = five
    gpu.set_options(test_batch_chunk=2)
    try:
        results = _check(gpu, imgs, True, 11500, 2, 128, sizes, "chunks of 2", singles=False)
    finally:
        gpu.set_options()
    assert len({_tuple(r) for r in results}) == 5


def test_fallbacks(gpu, oracle, five):
    """no probe kernel: partial edge blocks, the accurate search, the split path -- each alone on the whole-block list too -- the loop of single calls, the same results"""
    ragged = [oracle.photo_noise(203, 61, 3), oracle.random_gradient(203, 61, 7, False), oracle.photo_noise(203, 61, 11)]
    sizes = [Sizes(oracle, i, True) for i in ragged]
    budgets = [(s(1) + s(64)) // 2 for s in sizes]
    whole, whole_sizes = five[0][:3], five[1][:3]
    _check(gpu, ragged, True, budgets, 2, 128, sizes, "203x61")
    _check(gpu, ragged, True, budgets, 2, 128, [None] * 3, "203x61 accurate", fast=False)
    _check(gpu, whole, True, 11500, 2, 128, [None] * 3, "264x24 accurate", fast=False)
    gpu.set_options(force_split=True)
    try:
        _check(gpu, ragged, True, budgets, 2, 128, sizes, "203x61 split")
        _check(gpu, whole, True, 11500, 2, 128, whole_sizes, "264x24 split")
    finally:
        gpu.set_options()


def test_one_image_and_none(gpu, five):
    imgs, sizes = five
    _check(gpu, imgs[:1], True, 11500, 2, 128, sizes[:1], "count 1")
    assert gpu.encode_stream_budget_batch([], True, 11500) == ([], [])
    assert gpu.encode_stream_budget_batch_device([], True, 11500) == ([], [])


@pytest.mark.parametrize("opt", ["float_fast", "forced", "pcg", "record_limit_1", "record_limit_120"])
def test_options(gpu, five, opt):
    imgs, sizes = five
    if opt.startswith("record_limit"):
        if not L.has_hooks(gpu):
            return
        gpu.set_options(test_record_limit=int(opt.rsplit("_", 1)[1]))  # the probe's generic 32-bit search: the sizes are the oracle's
        try:
            _check(gpu, imgs, True, 11500, 2, 128, sizes, opt)
        finally:
            gpu.set_options()
        return
    if opt == "float_fast":  # no bit-exact oracle: the library's own FAST stream encode is the reference of the sizes
        gpu.set_options(float_fast=True)
        try:
            own = [lambda h, img=img: gpu.encode_stream(img, True, error_factor=2 * h).size for img in imgs]
            _check(gpu, imgs, True, 11500, 2, 128, own, opt)
        finally:
            gpu.set_options()
    elif opt == "forced":  # a flat curve: every image is refused, or met at the lower bound after two probes
        gpu.set_options(forced_shift=(7, 8, 1))
        try:
            flat = [gpu.encode_stream(img, True, error_factor=100).size for img in imgs]
            budgets = [f - 8 if i % 2 else f for i, f in enumerate(flat)]
            results = _check(gpu, imgs, True, budgets, 2, 128, [lambda h, f=f: f for f in flat], opt)
            assert [(r.errorFactor, r.withinBudget, r.probes) for r in results] == [(128, 0, 1) if i % 2 else (2, 1, 2) for i in range(5)]
        finally:
            gpu.set_options()
    else:  # PCG dither: other streams, the same sizes
        gpu.set_options(dither_pcg=True)
        try:
            _check(gpu, imgs, True, 11500, 2, 128, sizes, opt)
        finally:
            gpu.set_options()


def test_device_form_back_to_back(gpu, oracle, five):
    """torch tensors; two list calls of different shapes, then a plain batched stream encode, on one stream with no synchronisation of the test's own in between"""
    import torch
    imgs, sizes = five
    small = [oracle.photo_noise(128, 16, s) for s in (5, 9, 21)]
    small_sizes = [Sizes(oracle, i, True) for i in small]
    small_budgets = [(s(1) + s(64)) // 2 for s in small_sizes]
    da = [torch.from_numpy(i.view(np.int32)).cuda() for i in imgs]
    db = [torch.from_numpy(i.view(np.int32)).cuda() for i in small]
    torch.cuda.synchronize()
    oa, ra = gpu.encode_stream_budget_batch_device(da, True, 11500, 2, 128)
    ob, rb = gpu.encode_stream_budget_batch_device(db, True, small_budgets, 2, 128)
    plain, n = gpu.encode_stream_batch_device(da, True, error_factor=100)
    torch.cuda.synchronize()
    gpu.check()
    for what, ims, ss, budgets, outs, results in (("a", imgs, sizes, [11500] * 5, oa, ra), ("b", small, small_sizes, small_budgets, ob, rb)):
        for i, (img, size, out, res) in enumerate(zip(ims, ss, outs, results)):
            want_h, within, asked, nbytes = restated_search(size, 1, 64, budgets[i])
            assert _tuple(res) == (2 * want_h, within, len(asked), nbytes), (what, i)
            assert np.array_equal(out[:res.bytes].cpu().numpy(), gpu.encode_stream(img, True, error_factor=res.errorFactor)), (what, i)
    for i, img in enumerate(imgs):
        assert np.array_equal(plain[i][:n[i]].cpu().numpy(), gpu.encode_stream(img, True, error_factor=100)), i


def test_one_misaligned_image_in_the_list(gpu, five):
    """The probe's dword-load path.  The probe's domain is whole blocks, so the width is always a multiple of 4 and only an image that starts 4-byte but not 16-byte
    aligned takes it -- and with it every image of its chunk.  Three images, the middle one at element 1 of a tensor one element longer: results and streams must be
    exactly those of the call on the aligned tensors, which the tests above tie to the oracle."""
    import torch
    aligned = [torch.from_numpy(i.view(np.int32)).cuda() for i in five[0][:3]]
    moved = torch.empty(W * H + 1, dtype=torch.int32, device="cuda")[1:].view(H, W)
    moved.copy_(aligned[1])
    assert all(t.data_ptr() % 16 == 0 for t in aligned) and moved.data_ptr() % 16 == 4 and moved.is_contiguous()
    oa, ra = gpu.encode_stream_budget_batch_device(aligned, True, 11500, 2, 128)
    ob, rb = gpu.encode_stream_budget_batch_device([aligned[0], moved, aligned[2]], True, 11500, 2, 128)
    torch.cuda.synchronize()
    gpu.check()
    print([_tuple(r) for r in ra], [_tuple(r) for r in rb])
    assert [_tuple(r) for r in rb] == [_tuple(r) for r in ra] and {_outcome(r, 2) for r in ra} == {"refused", "bisected"}
    for i in range(3):
        assert torch.equal(ob[i][:rb[i].bytes], oa[i][:ra[i].bytes]), i


def _results(n, struct_size=None):
    rs = (limg_amd.BudgetResult * n)()
    for r in rs:
        r.struct_size, r.errorFactor, r.probes, r.withinBudget, r.bytes = struct_size or C.sizeof(limg_amd.BudgetResult), 7, 7, 7, 7
    return rs


def test_errors(gpu):
    """the contract's refusals, in its order, each before anything touches the device: the output buffers keep their pattern, the results their values"""
    import torch
    w, h, n = 64, 16, 3
    bound = gpu.stream_bound(w, h)
    imgs = [torch.zeros((h, w), dtype=torch.int32, device="cuda") for _ in range(n)]
    rooms = [torch.full((bound + 256,), 0x5A, dtype=torch.uint8, device="cuda") for _ in range(n)]
    assert all(r.data_ptr() % 16 == 0 for r in rooms)
    res = _results(n)
    dev, host = gpu.lib.limg_hip_encode_stream_budget_batch_device, gpu.lib.limg_hip_encode_stream_budget_batch
    NULL_, INVALID, BOUNDS = 102, 101, 103  # limg_hip_error_ArgumentNull, _InvalidParameter, _OutOfBounds
    ins, outs = (C.c_void_p * n)(*[i.data_ptr() for i in imgs]), (C.c_void_p * n)(*[r.data_ptr() for r in rooms])
    budgets = (C.c_size_t * n)(5000, 5000, 5000)

    def ptrs(base, at, value):
        a = (C.c_void_p * n)(*base)
        a[at] = value
        return a

    def call(ctx=gpu.ctx, count=n, pin=ins, ww=w, hh=h, pout=outs, cap=bound, pmax=budgets, lo=0, hi=0, pres=res):
        return dev(ctx, count, pin, ww, hh, 1, pout, cap, pmax, lo, hi, 0, 1, pres, None)

    # 1. the batched stream encode's errors in its order, pMaxBytes and pResults among the pointers
    assert call(ctx=None) == NULL_ and call(pin=None) == NULL_ and call(pout=None) == NULL_ and call(pmax=None) == NULL_ and call(pres=None) == NULL_
    assert call(pin=ptrs(ins, 2, None)) == NULL_ and call(pout=ptrs(outs, 1, None)) == NULL_
    assert call(ww=0) == INVALID and call(hh=0) == INVALID and call(ww=1 << 31) == INVALID
    assert call(cap=bound - 1) == BOUNDS
    misaligned = ptrs(outs, 2, rooms[2].data_ptr() + 8)
    assert call(pout=misaligned) == INVALID
    # 2. the bound rules, 3. a zero budget or a short struct_size, whichever image
    for bad in ({"lo": 3}, {"hi": 101}, {"lo": 1}, {"hi": 1}, {"lo": 200, "hi": 100}, {"lo": 2000}):
        assert call(**bad) == INVALID, bad
    assert call(pmax=(C.c_size_t * n)(5000, 5000, 0)) == INVALID and call(pmax=(C.c_size_t * n)(0, 5000, 5000)) == INVALID
    short = _results(n)
    short[1].struct_size = 16
    assert call(pres=short) == INVALID
    # the order
    assert call(pin=ptrs(ins, 0, None), ww=0) == NULL_ and call(ww=0, cap=0) == INVALID and call(cap=bound - 1, pout=misaligned) == BOUNDS
    assert call(cap=bound - 1, lo=3) == BOUNDS and call(pout=misaligned, pmax=(C.c_size_t * n)(0, 0, 0)) == INVALID
    # 4. an empty list: the checks that do not need an element still hold, then success with nothing done
    assert call(count=0, lo=3) == INVALID and call(count=0, cap=bound - 1) == BOUNDS and call(count=0, pres=None) == NULL_ and call(count=0) == 0
    # the host form: capacityEach below the bound is no error of its own there
    host_imgs = [np.zeros((h, w), dtype=np.uint32) for _ in range(n)]
    host_outs = [np.full(bound, 0x5A, dtype=np.uint8) for _ in range(n)]
    hin, hout = (C.c_void_p * n)(*[i.ctypes.data for i in host_imgs]), (C.c_void_p * n)(*[o.ctypes.data for o in host_outs])

    def hcall(ctx=gpu.ctx, count=n, pin=hin, ww=w, pout=hout, cap=bound, pmax=budgets, lo=0, hi=0, pres=res):
        return host(ctx, count, pin, ww, h, 1, pout, cap, pmax, lo, hi, 0, 1, pres)

    assert hcall(ctx=None) == NULL_ and hcall(pres=None) == NULL_ and hcall(pmax=None) == NULL_ and hcall(pin=ptrs(hin, 1, None)) == NULL_
    assert hcall(ww=0) == INVALID and hcall(lo=4, hi=2) == INVALID and hcall(pmax=(C.c_size_t * n)(5000, 0, 5000)) == INVALID and hcall(pres=short) == INVALID
    assert hcall(count=0, hi=7) == INVALID and hcall(count=0) == 0
    torch.cuda.synchronize()
    assert all(int((r != 0x5A).sum()) == 0 for r in rooms) and all(int((o != 0x5A).sum()) == 0 for o in host_outs), "a refused call wrote to an output buffer"
    assert all(_tuple(r) == (7, 7, 7, 7) for r in res) and all(_tuple(r) == (7, 7, 7, 7) for r in short), "a refused call wrote a result"
    # the context is usable and the same arguments are accepted: a flat image has one size from errorFactor 2 on, so the lower bound is the answer after two probes
    flat = gpu.encode_stream(host_imgs[0], True, error_factor=2).size
    assert flat <= 5000 and call() == 0 and all(_tuple(r) == (2, 1, 2, flat) for r in res)
    # the host form's capacity rule: all results filled, no stream written, limg_hip_error_OutOfBounds
    res2 = _results(n)
    assert hcall(cap=flat - 1, pres=res2) == BOUNDS and all(_tuple(r) == (2, 1, 2, flat) for r in res2)
    assert all(int((o != 0x5A).sum()) == 0 for o in host_outs)
    assert hcall(cap=flat, pres=res2) == 0 and all(np.array_equal(o[:flat], gpu.encode_stream(host_imgs[0], True, error_factor=2)) and int((o[flat:] != 0x5A).sum()) == 0 for o in host_outs)
    gpu.check()


def test_context_device_bytes(lib):
    """behind a single and a batched stream encode of the same list, the budgeted list adds 72 + 8 bytes per image -- state and counter -- and nothing else: it reads
    the images through the batched encode's own table"""
    g = L.open_context(lib)
    try:
        imgs = [g.synth_device("photo_noise", W, H, seed=5 + i) for i in range(5)]
        g.encode_stream_device(imgs[0], True)
        g.encode_stream_batch_device(imgs, True)
        before = g.device_bytes()
        _, results = g.encode_stream_budget_batch_device(imgs, True, 16000, 2, 128)
        assert g.device_bytes() - before == STATE_BYTES * 5, (before, g.device_bytes())
        before = g.device_bytes()
        _, again = g.encode_stream_budget_batch_device(imgs[:3], True, 16000, 2, 128)
        assert g.device_bytes() == before and [_tuple(r) for r in again] == [_tuple(r) for r in results[:3]]
        g.check()
    finally:
        g.close()


L.product_twins(globals())  # test_x_product: the same tests on the product library (tests/lib_axis.py)
