"""limg_hip_encode_stream_budget_list(_device): a list of images of MIXED shapes, each to its own byte budget, in one call -- per chunk the records from one
k_fit_tpb_list grid, one search state per image, the probes of all images in the same launches (k_rate_probe_list: one workgroup per work strip of the chunk, the
strip's image by a binary search over the strip prefix, its geometry and slices from its table entry; k_rate_begin_batch / k_rate_step_batch with the chunk's image
table, limg_hip_rate.hip), one wait, then the chunk through the mixed-list encode at the error factors the searches chose.

Result i must be what the single budget call gives for item i: the choice, probe count and bytes must equal the algorithm of include/limg_hip.h restated in Python
(tests/rate_search.py) over the ORACLE's sizes of that image, the stream must be limg_hip_encode_stream's at the chosen error factor byte for byte, and its header's
totalBytes the reported bytes.  The shapes are the smallest that reach each way the list probe can go wrong:

  edges           (264,24) (8,8) (256,8) (520,16) (8,512) (24,40) (512,32): a last strip of one block; an image of one workgroup; 65 blocks across, so a record slice
                  and an invN slice (4 floats per block) that start off any round number; 64 block rows of one block; strip counts 6, 1, 1, 6, 64, 5, 8, so the binary
                  search ends at every position; fixed bytes that differ per image
  one_strip_each  every workgroup belongs to another image than its neighbour
  rgb             3 channels: no raw-escape fields
  sixty_six       more images than one k_rate_begin_batch launch (64) and one table launch carry, and a second workgroup of the step kernel
  ragged_inside   two ineligible items (13 x 9, 256 x 20) take the single call inside the same call
  pool            pool_threads = 2 (the pool only moves the dither chains: the sizes are unchanged)"""
import ctypes as C

import numpy as np
import pytest

import lib_axis as L
import limg_amd
from lib_axis import lib, lib_product  # noqa: F401  (fixtures: "test" / "product")
from budget_list_cases import LISTS, image as _image
from limg_amd import StreamListItem
from rate_search import max_probes, oracle_size, restated_search

pytestmark = pytest.mark.gpu

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

    def __init__(self, oracle, img, alpha, kw):
        self.oracle, self.img, self.alpha, self.kw, self.memo = oracle, img, alpha, kw, {}

    def __call__(self, h):
        if h not in self.memo:
            self.memo[h] = oracle_size(self.oracle, self.img, self.alpha, 2 * h, **self.kw)
        return self.memo[h]


@pytest.fixture(scope="module")
def lists(oracle):
    """every list of LISTS once: (images, alpha, encode arguments, the oracle's size function of each image); sixty_six repeats five images (and their functions)"""
    out = {}
    for name, (alpha, shapes, kw) in LISTS.items():
        imgs, sizes, memo = [], [], {}
        for i, (w, h) in enumerate(shapes):
            key = i % 5 if name == "sixty_six" else i
            if key not in memo:
                img = _image(oracle, w, h, key)
                memo[key] = (img, Sizes(oracle, img, alpha, kw))
            imgs.append(memo[key][0]); sizes.append(memo[key][1])
        out[name] = (imgs, alpha, kw, sizes)
    return out


def _tuple(r):
    return (r.errorFactor, r.withinBudget, r.probes, r.bytes)


def _outcome(r, lo_ef):
    return "refused" if not r.withinBudget else ("lo" if r.errorFactor == (lo_ef or 2) else "bisected")


def _mid_budgets(sizes):
    """bisected, refused, met at the lower bound -- in turn"""
    return [((s(1) + s(64)) // 2, s(64) - 8, s(1))[i % 3] for i, s in enumerate(sizes)]


def _check(gpu, imgs, alpha, budgets, lo_ef, hi_ef, sizes, ctx, singles=True, fast=True, **kw):
    """one list call against the restated search over sizes[i](h); lo_ef / hi_ef as handed to the call (0: the defaults).  sizes[i] None: the single call is the
    reference of the search (the fallbacks).  -> (streams, results)"""
    h_lo, h_hi = (lo_ef or 2) // 2, (hi_ef or 1024) // 2
    n = len(imgs)
    budgets = [budgets] * n if np.isscalar(budgets) else list(budgets)
    streams, results = gpu.encode_stream_budget_list(imgs, alpha, budgets if len(set(budgets)) > 1 else budgets[0], lo_ef, hi_ef, fast=fast, **kw)
    assert len(streams) == len(results) == n, ctx
    for i in range(n):
        res, st = results[i], streams[i]
        if sizes[i] is not None:
            want_h, within, asked, nbytes = restated_search(sizes[i], h_lo, h_hi, budgets[i])
            print(ctx, i, budgets[i], _tuple(res), (2 * want_h, within, len(asked), nbytes))
            assert _tuple(res) == (2 * want_h, within, len(asked), nbytes), (ctx, i, budgets[i])
        assert res.probes <= max_probes(h_lo, h_hi) and (not res.withinBudget or res.bytes <= budgets[i]), (ctx, i)
        info = limg_amd.stream_info(st, gpu.lib)
        assert st.size == res.bytes == info[3] and (info[0], info[1]) == (imgs[i].shape[1], imgs[i].shape[0]), (ctx, i, st.size, res.bytes)
        want = gpu.encode_stream(imgs[i], alpha, error_factor=res.errorFactor, fast=fast, **kw)
        assert st.size == want.size and np.array_equal(st, want), (ctx, i, "the stream is not encode_stream's at the chosen error factor")
        if singles:
            one_st, one = gpu.encode_stream_budget(imgs[i], alpha, budgets[i], lo_ef, hi_ef, fast=fast, **kw)
            assert _tuple(res) == _tuple(one) and np.array_equal(st, one_st), (ctx, i, _tuple(res), _tuple(one))
    return streams, results


def test_edges_one_budget_three_outcomes(gpu, lists):
    """16000 bytes over [2, 128]: on the oracle errorFactor 12, 2, 2, 6, 2, 2 and refused at 128 -- all three outcomes in ONE call, fixed bytes that differ per image"""
    imgs, alpha, kw, sizes = lists["edges"]
    _, results = _check(gpu, imgs, alpha, 16000, 2, 128, sizes, "edges")
    assert [(r.errorFactor, r.withinBudget) for r in results] == [(12, 1), (2, 1), (2, 1), (6, 1), (2, 1), (2, 1), (128, 0)], [_tuple(r) for r in results]
    assert {_outcome(r, 2) for r in results} == {"refused", "lo", "bisected"}
    assert len({_tuple(results[i]) for i in (0, 3, 6)}) == 3, [_tuple(r) for r in results]


def test_edges_default_bounds(gpu, lists):
    """[2, 1024]: the largest launch count"""
    imgs, alpha, kw, sizes = lists["edges"]
    _, results = _check(gpu, imgs, alpha, 16000, 0, 0, sizes, "edges, default bounds")
    assert [(r.errorFactor, r.withinBudget, r.probes) for r in results] == [(12, 1, 11), (2, 1, 2), (2, 1, 2), (6, 1, 11), (2, 1, 2), (2, 1, 2), (1024, 0, 1)]
    assert results[6].bytes == 20568


@pytest.mark.parametrize("bounds", [(2, 128), (0, 0)], ids=["2_128", "defaults"])
def test_per_image_budgets(gpu, lists, bounds):
    """bottom - 8, top, the middle, top + 8, bottom, ... -- one per image, from the oracle"""
    imgs, alpha, kw, sizes = lists["edges"]
    lo_ef, hi_ef = bounds
    budgets = []
    for i, size in enumerate(sizes):
        top, bottom = size((lo_ef or 2) // 2), size((hi_ef or 1024) // 2)
        assert bottom < top
        budgets.append((bottom - 8, top, (top + bottom) // 2, top + 8, bottom)[i % 5])
    _, results = _check(gpu, imgs, alpha, budgets, lo_ef, hi_ef, sizes, ("per image", bounds))
    assert {_outcome(r, lo_ef) for r in results} == {"refused", "lo", "bisected"}


@pytest.mark.parametrize("name", ["one_strip_each", "rgb", "sixty_six", "ragged_inside", "pool"])
def test_other_lists(gpu, lists, name):
    imgs, alpha, kw, sizes = lists[name]
    if name == "one_strip_each":
        _, results = _check(gpu, imgs, alpha, 5000, 2, 128, sizes, name, **kw)
        assert [(r.errorFactor, r.bytes) for r in results] == [(14, 4968), (2, 216), (14, 4864), (2, 336), (14, 4912)], [_tuple(r) for r in results]
    elif name == "rgb":
        _, results = _check(gpu, imgs, alpha, 6000, 2, 128, sizes, name, **kw)
        assert [(r.errorFactor, r.withinBudget) for r in results] == [(128, 0), (2, 1), (8, 1)], [_tuple(r) for r in results]
    else:  # (the single-call comparison is left out above 10 items, as in tests/test_gpu_stream_budget_batch.py)
        _, results = _check(gpu, imgs, alpha, _mid_budgets(sizes), 2, 128, sizes, name, singles=len(imgs) < 10, **kw)
        assert {_outcome(r, 2) for r in results} == {"refused", "lo", "bisected"}


def _same(got, want, what):
    (gs, gr), (ws, wr) = got, want
    assert [_tuple(r) for r in gr] == [_tuple(r) for r in wr], what
    for i, (a, b) in enumerate(zip(gs, ws)):
        assert a.size == b.size and np.array_equal(a, b), (what, i)


def test_order_does_not_matter(gpu, lists):
    """the reversed list, and the list rotated by one, give the same result and stream per image"""
    imgs, alpha, kw, sizes = lists["edges"]
    n = len(imgs)
    budgets = _mid_budgets(sizes)
    streams, results = _check(gpu, imgs, alpha, budgets, 2, 128, sizes, "edges, per image", singles=False)
    for perm in (list(range(n))[::-1], [(i + 1) % n for i in range(n)]):
        got = gpu.encode_stream_budget_list([imgs[i] for i in perm], alpha, [budgets[i] for i in perm], 2, 128)
        _same(got, ([streams[i] for i in perm], [results[i] for i in perm]), perm)


def test_chunks(gpu, lists):
    """test hook batch_chunk = 3: edges as 3 + 3 + 1 (the last through the single call), sixty_six as 22 chunks, twice in a row: the results of the one-chunk call"""
    if not L.has_hooks(gpu):
        return
    for name in ("edges", "sixty_six"):
        imgs, alpha, kw, sizes = lists[name]
        budgets = _mid_budgets(sizes)
        whole = gpu.encode_stream_budget_list(imgs, alpha, budgets, 2, 128)
        gpu.set_options(test_batch_chunk=3)
        try:
            for rep in range(2):
                _same(gpu.encode_stream_budget_list(imgs, alpha, budgets, 2, 128), whole, (name, rep))
        finally:
            gpu.set_options()
        for i, (res, size) in enumerate(zip(whole[1], sizes)):
            want_h, within, asked, nbytes = restated_search(size, 1, 64, budgets[i])
            assert _tuple(res) == (2 * want_h, within, len(asked), nbytes), (name, i)


def test_same_shape_one_and_none(gpu, oracle):
    """five images of 264 x 24 take the same-shape list's route: encode_stream_budget_batch's results and streams; a list of one; an empty list"""
    imgs = [_image(oracle, 264, 24, i) for i in range(5)]
    budgets = [11500, 9000, 11500, 30000, 7000]
    _same(gpu.encode_stream_budget_list(imgs, True, budgets, 2, 128), gpu.encode_stream_budget_batch(imgs, True, budgets, 2, 128), "same shape")
    one_st, one = gpu.encode_stream_budget(imgs[0], True, 11500, 2, 128)
    _same(gpu.encode_stream_budget_list(imgs[:1], True, 11500, 2, 128), ([one_st], [one]), "a list of one")
    assert gpu.encode_stream_budget_list([], True, 11500) == ([], [])
    assert gpu.encode_stream_budget_list_device([], True, 11500) == ([], [])


@pytest.mark.parametrize("opt", ["float_fast", "forced", "pcg", "record_limit_1", "record_limit_120"])
def test_options(gpu, lists, opt):
    imgs, alpha, kw, sizes = lists["edges"]
    if opt.startswith("record_limit"):
        if not L.has_hooks(gpu):
            return
        gpu.set_options(test_record_limit=int(opt.rsplit("_", 1)[1]))  # the probe's generic 32-bit search: the sizes are the oracle's
        try:
            _check(gpu, imgs, alpha, 16000, 2, 128, sizes, opt)
        finally:
            gpu.set_options()
        return
    if opt == "float_fast":  # no bit-exact oracle: the library's own FAST stream encode is the reference of the sizes
        gpu.set_options(float_fast=True)
        try:
            own = [lambda h, img=img: gpu.encode_stream(img, alpha, error_factor=2 * h).size for img in imgs]
            _check(gpu, imgs, alpha, 16000, 2, 128, own, opt)
        finally:
            gpu.set_options()
    elif opt == "forced":  # a flat curve: every item is refused after one probe, or met at the lower bound after two
        gpu.set_options(forced_shift=(7, 8, 1))
        try:
            flat = [gpu.encode_stream(img, alpha, error_factor=100).size for img in imgs]
            budgets = [f - 8 if i % 2 else f for i, f in enumerate(flat)]
            _, results = _check(gpu, imgs, alpha, budgets, 2, 128, [lambda h, f=f: f for f in flat], opt)
            assert [(r.errorFactor, r.withinBudget, r.probes) for r in results] == [(128, 0, 1) if i % 2 else (2, 1, 2) for i in range(len(imgs))]
        finally:
            gpu.set_options()
    else:  # PCG dither: other streams, the same sizes
        gpu.set_options(dither_pcg=True)
        try:
            _check(gpu, imgs, alpha, 16000, 2, 128, sizes, opt)
        finally:
            gpu.set_options()


@pytest.mark.parametrize("how", ["force_split", "legacy_float_stage", "accurate"])
def test_fallbacks(gpu, lists, how):
    """force_split_kernels, legacy_float_stage and fastBitCrushing == 0: no item is eligible, every one takes the single call -- the single calls' results"""
    imgs, alpha, kw, sizes = lists["one_strip_each"]
    gpu.set_options(force_split=how == "force_split", legacy_float_stage=how == "legacy_float_stage")
    try:
        _check(gpu, imgs, alpha, 5000, 2, 128, [None] * len(imgs), how, fast=how != "accurate")
    finally:
        gpu.set_options()


def _to_device(imgs):
    import torch
    return [torch.from_numpy(i.view(np.int32)).cuda() for i in imgs]


def test_one_misaligned_image_in_the_list(gpu, lists):
    """The probe's dword-load path, for ONE image of the chunk: the middle item of three starts 4-byte but not 16-byte aligned.  Results and streams must be exactly
    those of the call on aligned tensors, which the tests above tie to the oracle."""
    import torch
    imgs = lists["edges"][0]
    aligned = _to_device([imgs[0], imgs[3], imgs[6]])
    h, w = imgs[3].shape
    moved = torch.empty(w * h + 1, dtype=torch.int32, device="cuda")[1:].view(h, w)
    moved.copy_(aligned[1])
    assert all(t.data_ptr() % 16 == 0 for t in aligned) and moved.data_ptr() % 16 == 4 and moved.is_contiguous()
    oa, ra = gpu.encode_stream_budget_list_device(aligned, True, 16000, 2, 128)
    ob, rb = gpu.encode_stream_budget_list_device([aligned[0], moved, aligned[2]], True, 16000, 2, 128)
    torch.cuda.synchronize()
    gpu.check()
    assert [_tuple(r) for r in rb] == [_tuple(r) for r in ra] and {_outcome(r, 2) for r in ra} == {"refused", "bisected"}
    for i in range(3):
        assert torch.equal(ob[i][:rb[i].bytes], oa[i][:ra[i].bytes]), i


def test_device_form_back_to_back(gpu, lists):
    """torch tensors; two list calls of different lists, then a plain mixed-list encode, on one stream with no synchronisation of the test's own in between"""
    import torch
    (ia, alpha, _, sa), (ib, _, _, sb) = lists["edges"], lists["one_strip_each"]
    ba, bb = _mid_budgets(sa), [5000] * len(ib)
    da, db = _to_device(ia), _to_device(ib)
    torch.cuda.synchronize()
    oa, ra = gpu.encode_stream_budget_list_device(da, alpha, ba, 2, 128)
    ob, rb = gpu.encode_stream_budget_list_device(db, alpha, bb, 2, 128)
    plain, n = gpu.encode_stream_list_device(da, alpha, 100)
    torch.cuda.synchronize()
    gpu.check()
    for what, ims, ss, budgets, outs, results in (("a", ia, sa, ba, oa, ra), ("b", ib, sb, bb, ob, rb)):
        for i, (img, size, out, res) in enumerate(zip(ims, ss, outs, results)):
            want_h, within, asked, nbytes = restated_search(size, 1, 64, budgets[i])
            assert _tuple(res) == (2 * want_h, within, len(asked), nbytes), (what, i)
            assert np.array_equal(out[:res.bytes].cpu().numpy(), gpu.encode_stream(img, alpha, error_factor=res.errorFactor)), (what, i)
    for i, img in enumerate(ia):
        assert np.array_equal(plain[i][:n[i]].cpu().numpy(), gpu.encode_stream(img, alpha, error_factor=100)), i


def _results(n, struct_size=None):
    rs = (limg_amd.BudgetResult * n)()
    for r in rs:
        r.struct_size, r.errorFactor, r.probes, r.withinBudget, r.bytes = struct_size or C.sizeof(limg_amd.BudgetResult), 7, 7, 7, 7
    return rs


def test_errors(gpu):
    """the contract's refusals, one case per rule in its order, each before anything touches the device: canary-filled stream buffers and preset results stay untouched"""
    import torch
    shapes = ((64, 16), (8, 8), (264, 24))
    n = len(shapes)
    imgs = [torch.zeros((h, w), dtype=torch.int32, device="cuda") for w, h in shapes]
    bounds = [gpu.stream_bound(w, h) for w, h in shapes]
    room = [torch.full((b + 256,), 0x5A, dtype=torch.uint8, device="cuda") for b in bounds]
    assert all(r.data_ptr() % 16 == 0 for r in room)
    res = _results(n)
    dev, host = gpu.lib.limg_hip_encode_stream_budget_list_device, gpu.lib.limg_hip_encode_stream_budget_list
    NULL_, INVALID, BOUNDS = 102, 101, 103  # limg_hip_error_ArgumentNull, _InvalidParameter, _OutOfBounds
    SIZE = C.sizeof(StreamListItem)
    budgets = (C.c_size_t * n)(8000, 8000, 8000)

    def items(**change):
        """the good list with item 1 (and, `also2`, item 2) changed"""
        it = (StreamListItem * n)()
        for k in range(n):
            it[k] = StreamListItem(imgs[k].data_ptr(), room[k].data_ptr(), bounds[k], shapes[k][0], shapes[k][1], 12345, 0)  # (errorFactor is ignored)
        also2 = change.pop("also2", {})
        for name, v in change.items():
            setattr(it[1], name, v)
        for name, v in also2.items():
            setattr(it[2], name, v)
        return it

    def call(ctx=gpu.ctx, count=n, it=None, size=SIZE, pmax=budgets, lo=0, hi=0, pres=res):
        return dev(ctx, count, items() if it is None else it, size, 1, pmax, lo, hi, 0, 1, pres, None)

    # 1. NULL context or pointers, pMaxBytes and pResults among them -- before the item size and before the empty list
    assert call(ctx=None) == NULL_ and call(pmax=None) == NULL_ and call(pres=None) == NULL_
    assert dev(gpu.ctx, n, None, SIZE, 1, budgets, 0, 0, 0, 1, res, None) == NULL_ and dev(gpu.ctx, 0, None, 0, 1, budgets, 0, 0, 0, 1, res, None) == NULL_
    # 2. itemSize -- before any item
    assert call(size=SIZE - 1, it=items(sizeX=0)) == INVALID and call(size=0, it=items(pIn=None)) == INVALID
    # 3. per item, the first offending item in list order: a NULL pointer, a zero size, the size bound, alignment, capacity below the bound, reserved
    assert call(it=items(pIn=None)) == NULL_ and call(it=items(pStream=None)) == NULL_
    assert call(it=items(sizeX=0)) == INVALID and call(it=items(sizeY=0)) == INVALID
    assert call(it=items(sizeX=0xFFFFFFF8, sizeY=0xFFFFFFF8)) == INVALID
    assert call(it=items(pStream=room[1].data_ptr() + 8)) == INVALID
    assert call(it=items(capacity=bounds[1] - 1)) == BOUNDS
    assert call(it=items(reserved=1)) == INVALID
    assert call(it=items(capacity=0, also2={"pIn": None})) == BOUNDS and call(it=items(reserved=1, also2={"capacity": 0})) == INVALID
    # 4. the bound rules, a zero budget, struct_size -- behind every item rule
    for bad in ({"lo": 3}, {"hi": 101}, {"lo": 1}, {"hi": 1}, {"lo": 200, "hi": 100}, {"lo": 2000}):
        assert call(**bad) == INVALID, bad
    assert call(pmax=(C.c_size_t * n)(5000, 5000, 0)) == INVALID and call(pmax=(C.c_size_t * n)(0, 5000, 5000)) == INVALID
    short = _results(n)
    short[1].struct_size = 16
    assert call(pres=short) == INVALID
    assert call(it=items(capacity=bounds[1] - 1), lo=3) == BOUNDS and call(it=items(pIn=None), pmax=(C.c_size_t * n)(0, 0, 0)) == NULL_
    # 5. an empty list: the checks that do not need an element still hold, then success with nothing done
    assert call(count=0, lo=3) == INVALID and call(count=0, size=SIZE - 1) == INVALID and call(count=0, pres=None) == NULL_ and call(count=0) == 0
    # the host form: the same order; a capacity below the bound is no error of its own there
    host_imgs = [np.zeros((h, w), dtype=np.uint32) for w, h in shapes]
    host_outs = [np.full(b, 0x5A, dtype=np.uint8) for b in bounds]

    def hitems(caps=bounds):
        it = (StreamListItem * n)()
        for k in range(n):
            it[k] = StreamListItem(host_imgs[k].ctypes.data, host_outs[k].ctypes.data, caps[k], shapes[k][0], shapes[k][1], 0, 0)
        return it

    def hcall(ctx=gpu.ctx, count=n, it=None, size=SIZE, pmax=budgets, lo=0, hi=0, pres=res):
        return host(ctx, count, hitems() if it is None else it, size, 1, pmax, lo, hi, 0, 1, pres)

    bad_item = hitems()
    bad_item[2].reserved = 9
    assert hcall(ctx=None) == NULL_ and hcall(pres=None) == NULL_ and hcall(pmax=None) == NULL_ and hcall(size=8) == INVALID and hcall(it=bad_item) == INVALID
    assert hcall(lo=4, hi=2) == INVALID and hcall(pmax=(C.c_size_t * n)(5000, 0, 5000)) == INVALID and hcall(pres=short) == INVALID
    assert hcall(count=0, hi=7) == INVALID and hcall(count=0) == 0
    torch.cuda.synchronize()
    assert all(int((r != 0x5A).sum()) == 0 for r in room) and all(int((o != 0x5A).sum()) == 0 for o in host_outs), "a refused call wrote to an output buffer"
    assert all(_tuple(r) == (7, 7, 7, 7) for r in res) and all(_tuple(r) == (7, 7, 7, 7) for r in short), "a refused call wrote a result"
    # the context is usable and the same arguments are accepted: a flat image has one size from errorFactor 2 on, so the lower bound is the answer after two probes
    flat = [gpu.encode_stream(i, True, error_factor=2).size for i in host_imgs]
    assert max(flat) <= 8000 and call() == 0 and [_tuple(r) for r in res] == [(2, 1, 2, f) for f in flat]
    # the host form's capacity rule: all results filled, no stream written, limg_hip_error_OutOfBounds
    res2 = _results(n)
    assert hcall(it=hitems([flat[0], flat[1] - 1, flat[2]]), pres=res2) == BOUNDS and [_tuple(r) for r in res2] == [(2, 1, 2, f) for f in flat]
    assert all(int((o != 0x5A).sum()) == 0 for o in host_outs)
    assert hcall(it=hitems(flat), pres=res2) == 0
    assert all(np.array_equal(o[:f], gpu.encode_stream(i, True, error_factor=2)) and int((o[f:] != 0x5A).sum()) == 0 for o, f, i in zip(host_outs, flat, host_imgs))
    gpu.check()


def test_context_memory(lib, lists):
    """behind a mixed-list encode of the same list, the budgeted list adds sizeof(RateDevice) + 8 bytes per image -- state and counter -- and nothing else; a second call
    grows nothing; a closed context gave back everything"""
    import torch
    imgs, alpha, kw, sizes = lists["edges"]
    live = (lambda: np.array(limg_amd.live_resources(limg_amd.load_library(L.TEST)), dtype=np.int64)) if lib == "test" else None
    base = live() if live else None
    dimgs = _to_device(imgs)
    g = L.open_context(lib)
    try:
        g.encode_stream_list_device(dimgs, alpha, 100)
        before = g.device_bytes()
        _, results = g.encode_stream_budget_list_device(dimgs, alpha, 16000, 2, 128)
        assert g.device_bytes() - before == STATE_BYTES * len(imgs), (before, g.device_bytes())
        before = g.device_bytes()
        _, again = g.encode_stream_budget_list_device(dimgs, alpha, 16000, 2, 128)
        torch.cuda.synchronize()
        assert g.device_bytes() == before and [_tuple(r) for r in again] == [_tuple(r) for r in results]
        g.check()
    finally:
        g.close()
    if live:
        assert np.array_equal(live(), base), (live() - base).tolist()


L.product_twins(globals())  # test_x_product: the same tests on the product library (tests/lib_axis.py)
