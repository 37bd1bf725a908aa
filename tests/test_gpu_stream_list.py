"""limg_hip_encode_stream_list(_device): a list of images of MIXED shapes to version 1 streams in one call, image i at its own error factor.  The items that can
share launches go through one float-stage grid (k_fit_tpb_list), one persistent launch (k_encode_list_mixed: per strip its image's view from a device table), one
scan and one pack per chunk; the others take the single call inside the same call.  Stream i must be byte for byte the single call's: against the CPU restatement
of the container (oracle/stream.py), against limg_hip_encode_stream(_device) under every option the list honours, whatever the order of the list, in chunks,
through the fallbacks, back to back, from two threads; and the contract's refusals, in its order, write nothing."""
import ctypes as C
import threading

import numpy as np
import pytest

import lib_axis as L
from lib_axis import lib, lib_product  # noqa: F401  (fixtures: "test" / "product")
import limg_amd
from limg_amd import StreamListItem
from oracle import stream as S

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


FACTORS = (0, 1, 2, 37, 101, 400, 1000)
SMALL = ((264, 24), (8, 8), (256, 8), (24, 40), (512, 32))  # the five shapes `sixty_six` cycles through
# (name, alpha, shapes (w, h), encode arguments)
LISTS = (
    # a last strip of one block; one block; one strip; 65 blocks across (a second float-stage unit of one block, three strips per row); one block wide and 64 rows;
    # widths that are and are not multiples of 16 side by side: the access flags must be per image
    ("edges", True, ((264, 24), (8, 8), (256, 8), (520, 16), (8, 512), (24, 40), (512, 32)), {}),
    # every workgroup's F step belongs to an image of another shape than its E step
    ("one_strip_each", True, ((256, 8), (8, 8), (248, 8), (16, 8), (256, 8)), {}),
    # strips per image 4, 4, 3, 4, 1, 8: slices start on and off a multiple of 4, with lengths that are and are not multiples of 4
    ("scan_slices", True, ((256, 32), (512, 16), (256, 24), (1024, 8), (8, 8), (512, 32)), {}),
    ("rgb", False, ((512, 32), (40, 24), (264, 8)), {}),
    # chainRows differs per image, and one image has fewer block rows than chains
    ("pool", True, ((128, 256), (64, 24), (8, 8), (256, 40)), {"pool_threads": 2}),
    # the two ineligible items take the single call inside the same call
    ("ragged_inside", True, ((264, 24), (13, 9), (256, 20), (8, 8)), {}),
    # more than one table launch holds
    ("sixty_six", True, tuple(SMALL[i % 5] for i in range(66)), {}),
)


def _image(oracle, w, h, i):
    """photo-noise and random-gradient images alternate"""
    return oracle.photo_noise(w, h, 3 + 2 * (i % 8)) if i % 2 == 0 else oracle.random_gradient(w, h, 3 + 2 * (i % 8), False)


@pytest.fixture(scope="module")
def lists(oracle):
    """every list of LISTS once: its images and factors, the stream the container's CPU restatement makes of the oracle's encode of image i at factor i, and that
    encode's pDecoded (a repeated (image, factor) pair is encoded once)"""
    out = {}
    for k, (name, alpha, shapes, kw) in enumerate(LISTS):
        rng = np.random.default_rng(100 + k)
        efs = [int(FACTORS[j]) for j in rng.integers(0, len(FACTORS), len(shapes))] if name != "sixty_six" else [FACTORS[i % 7] for i in range(len(shapes))]
        imgs, streams, decoded, memo = [], [], [], {}
        for i, ((w, h), ef) in enumerate(zip(shapes, efs)):
            key = (w, h, (i % 5) if name == "sixty_six" else i, ef)
            if key not in memo:
                img = _image(oracle, w, h, key[2])
                e = oracle.encode3d(img, alpha, extras=True, error_factor=ef, **kw)
                memo[key] = (img, S.pack(e, w, h, 4 if alpha else 3, error_factor=ef), e["pDecoded"])
            imgs.append(memo[key][0]); streams.append(memo[key][1]); decoded.append(memo[key][2])
        out[name] = (imgs, alpha, efs, kw, streams, decoded)
    return out


def _same(got, want, what):
    assert len(got) == len(want), what
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.size == b.size, (what, i, a.size, b.size)
        assert np.array_equal(a, b), (what, i, np.argwhere(a != b)[:8].ravel())


def _singles(gpu, imgs, alpha, efs, **kw):
    return [gpu.encode_stream(i, alpha, error_factor=ef, **kw) for i, ef in zip(imgs, efs)]


def _to_device(imgs):
    import torch
    return [torch.from_numpy(i.view(np.int32)).cuda() for i in imgs]


def test_bytes_against_the_oracle(gpu, lists):
    for name, (imgs, alpha, efs, kw, streams, decoded) in lists.items():
        got = gpu.encode_stream_list(imgs, alpha, efs, **kw)
        _same(got, streams, name)
        seen = set()
        for img, st, dec, ef in zip(imgs, got, decoded, efs):
            head = S.parse(st)[0]
            assert (int(head["errorFactor"]), int(head["sizeX"]), int(head["sizeY"])) == (ef, img.shape[1], img.shape[0]), (name, ef)
            if (img.shape, ef, id(dec)) not in seen:
                seen.add((img.shape, ef, id(dec)))
                assert np.array_equal(gpu.decode_stream(st), dec), name


def test_equals_single_calls(gpu, lists):
    """the host form and the device form; pBytes is each stream's totalBytes"""
    import torch
    for name, (imgs, alpha, efs, kw, streams, _) in lists.items():
        if name == "sixty_six":
            want = streams  # (the single calls' equality with the oracle's container: tests/test_gpu_stream.py; 66 more of them here would show nothing new)
        else:
            want = _singles(gpu, imgs, alpha, efs, **kw)
        _same(gpu.encode_stream_list(imgs, alpha, efs, **kw), want, name)
        outs, sizes = gpu.encode_stream_list_device(_to_device(imgs), alpha, efs, **kw)
        torch.cuda.synchronize()
        assert sizes == [w.size for w in want], name
        assert sizes == [int(S.parse(w)[0]["totalBytes"]) for w in want], name
        _same([o[:n].cpu().numpy() for o, n in zip(outs, sizes)], want, (name, "device"))
    gpu.check()


def test_order_does_not_matter(gpu, lists):
    """the reversed list, and the list rotated by one, give the same stream per image"""
    for name in ("edges", "one_strip_each", "scan_slices", "pool", "ragged_inside"):
        imgs, alpha, efs, kw, streams, _ = lists[name]
        n = len(imgs)
        for perm in (list(range(n))[::-1], [(i + 1) % n for i in range(n)]):
            got = gpu.encode_stream_list([imgs[i] for i in perm], alpha, [efs[i] for i in perm], **kw)
            _same(got, [streams[i] for i in perm], (name, perm))


def test_same_shape_list_equals_batch_ef(gpu, oracle):
    imgs = [_image(oracle, 264, 24, i) for i in range(5)]
    efs = (400, 2, 100, 0, 37)
    _same(gpu.encode_stream_list(imgs, True, efs), gpu.encode_stream_batch_ef(imgs, True, efs), "same shape")
    _same(gpu.encode_stream_list(imgs[:1], True, efs[:1]), gpu.encode_stream_batch_ef(imgs[:1], True, efs[:1]), "a list of one")


def test_chunks_and_sub_batches(gpu, lists):
    """test hook batch_chunk = 3: chunks of different strip totals (sixty_six: 22 of them; edges: 3 + 3 + 1, the last through the single call), twice in a row;
    batch_sub_images does not apply to the mixed route: the same bytes"""
    for name in ("edges", "sixty_six"):
        imgs, alpha, efs, kw, streams, _ = lists[name]
        if L.has_hooks(gpu):
            gpu.set_options(test_batch_chunk=3)
            try:
                for rep in range(2):
                    _same(gpu.encode_stream_list(imgs, alpha, efs, **kw), streams, (name, "chunk", rep))
            finally:
                gpu.set_options()
        gpu.set_options(batch_sub_images=2)
        try:
            _same(gpu.encode_stream_list(imgs, alpha, efs, **kw), streams, (name, "sub_images"))
        finally:
            gpu.set_options()


@pytest.mark.parametrize("opts", [{"float_fast": True}, {"dither_pcg": True}, {"forced_shift": (7, 8, 1)}], ids=["float_fast", "pcg", "shift781"])
def test_options(gpu, lists, opts):
    """float_mode = 1 (the FAST instances), dither_pcg and forced_shift reach the list as they reach the single call"""
    imgs, alpha, efs, kw, streams, _ = lists["edges"]
    gpu.set_options(**opts)
    try:
        want = _singles(gpu, imgs, alpha, efs, **kw)
        _same(gpu.encode_stream_list(imgs, alpha, efs, **kw), want, opts)
    finally:
        gpu.set_options()
    if "float_fast" not in opts:  # (FAST may or may not change a byte of these images; the other two must)
        assert any(not np.array_equal(a, b) for a, b in zip(want, streams)), "the option changed nothing: the comparison above shows nothing"


@pytest.mark.parametrize("how", ["force_split", "legacy_float_stage", "accurate"])
def test_fallbacks(gpu, lists, how):
    """force_split_kernels, legacy_float_stage and fastBitCrushing == 0: no item is eligible, every one takes the single call -- the same bytes"""
    imgs, alpha, efs, kw, _, _ = lists["scan_slices"]
    fast = how != "accurate"
    gpu.set_options(force_split=how == "force_split", legacy_float_stage=how == "legacy_float_stage")
    try:
        _same(gpu.encode_stream_list(imgs, alpha, efs, fast=fast, **kw), _singles(gpu, imgs, alpha, efs, fast=fast, **kw), how)
    finally:
        gpu.set_options()


def _items(imgs, outs, efs):
    items = (StreamListItem * len(imgs))()
    for k, (i, o, ef) in enumerate(zip(imgs, outs, efs)):
        items[k] = StreamListItem(i.data_ptr(), o.data_ptr(), o.numel(), i.shape[1], i.shape[0], ef, 0)
    return items


def test_back_to_back(gpu, lists):
    """two calls on one stream with no wait between them, the host item array overwritten with garbage right after each call returns"""
    import torch
    (ia, alpha, ea, _, wa, _), (ib, _, eb, _, wb, _) = lists["edges"], lists["scan_slices"]
    da, db = _to_device(ia), _to_device(ib)
    oa = [torch.zeros(gpu.stream_bound(i.shape[1], i.shape[0]), dtype=torch.uint8, device="cuda") for i in da]
    ob = [torch.zeros(gpu.stream_bound(i.shape[1], i.shape[0]), dtype=torch.uint8, device="cuda") for i in db]
    torch.cuda.synchronize()
    for d, o, e in ((da, oa, ea), (db, ob, eb)):
        items = _items(d, o, e)
        r = gpu.lib.limg_hip_encode_stream_list_device(gpu.ctx, len(d), items, C.sizeof(StreamListItem), int(alpha), None, 0, 1, gpu._stream())
        C.memset(items, 0xA5, C.sizeof(items))
        assert r == 0
    torch.cuda.synchronize()
    gpu.check()
    for outs, ref in ((oa, wa), (ob, wb)):
        _same([o[:r.size].cpu().numpy() for o, r in zip(outs, ref)], ref, "back to back")


def test_two_contexts_two_threads(lib, lists):
    """two contexts on two threads encode `edges` and `scan_slices` at once, three times each: all bytes right, check() clean in both"""
    ctxs = [L.open_context(lib), L.open_context(lib)]
    names = ("edges", "scan_slices")
    failures = []

    def work(k):
        try:
            imgs, alpha, efs, kw, streams, _ = lists[names[k]]
            for rep in range(3):
                _same(ctxs[k].encode_stream_list(imgs, alpha, efs, **kw), streams, (names[k], rep))
            ctxs[k].check()
        except BaseException as e:  # noqa: BLE001  (reported on the main thread)
            failures.append((k, repr(e)))

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for g in ctxs:
        g.close()
    assert not failures, failures


def test_errors(gpu):
    """the contract's refusals, one case per rule in its order, each before anything touches the device: canary-filled stream buffers and pBytes stay untouched"""
    import torch
    shapes = ((64, 16), (8, 8), (264, 24))
    n = len(shapes)
    imgs = [torch.zeros((h, w), dtype=torch.int32, device="cuda") for w, h in shapes]
    bounds = [gpu.stream_bound(w, h) for w, h in shapes]
    room = [torch.full((b + 256,), 0x5A, dtype=torch.uint8, device="cuda") for b in bounds]
    assert all(r.data_ptr() % 16 == 0 for r in room)
    sizes = (C.c_size_t * n)(*([0x5A5A] * n))
    dev, host = gpu.lib.limg_hip_encode_stream_list_device, gpu.lib.limg_hip_encode_stream_list
    NULL_, INVALID, BOUNDS = 102, 101, 103  # limg_hip_error_ArgumentNull, _InvalidParameter, _OutOfBounds
    SIZE = C.sizeof(StreamListItem)
    assert SIZE == 40

    def items(**change):
        """the good list with item 1 (and, `also2`, item 2) changed"""
        it = (StreamListItem * n)()
        for k in range(n):
            it[k] = StreamListItem(imgs[k].data_ptr(), room[k].data_ptr(), bounds[k], shapes[k][0], shapes[k][1], (0, 100, 401)[k], 0)
        also2 = change.pop("also2", {})
        for name, v in change.items():
            setattr(it[1], name, v)
        for name, v in also2.items():
            setattr(it[2], name, v)
        return it

    def call(ctx=gpu.ctx, count=n, it=None, size=SIZE, pb=sizes):
        return dev(ctx, count, items() if it is None else it, size, 1, pb, 0, 1, None)

    # 1. NULL context or pointers -- before the item size and before the empty list
    assert call(ctx=None) == NULL_
    assert dev(gpu.ctx, n, None, SIZE, 1, sizes, 0, 1, None) == NULL_ and dev(gpu.ctx, 0, None, 0, 1, sizes, 0, 1, None) == NULL_
    assert host(gpu.ctx, n, items(), SIZE, 1, None, 0, 1) == NULL_ and host(None, n, items(), SIZE, 1, sizes, 0, 1) == NULL_
    # 2. itemSize -- before any item
    assert call(size=SIZE - 1, it=items(sizeX=0)) == INVALID and call(size=0, it=items(pIn=None)) == INVALID
    # 3. per item, the first offending item in list order: a NULL pointer, a zero size, the size bound, alignment, capacity below the bound, reserved
    assert call(it=items(pIn=None)) == NULL_ and call(it=items(pStream=None)) == NULL_
    assert call(it=items(sizeX=0)) == INVALID and call(it=items(sizeY=0)) == INVALID
    assert call(it=items(sizeX=0xFFFFFFF8, sizeY=0xFFFFFFF8)) == INVALID  # the single call's size bound
    assert call(it=items(pStream=room[1].data_ptr() + 8)) == INVALID
    assert call(it=items(capacity=bounds[1] - 1)) == BOUNDS
    assert call(it=items(reserved=1)) == INVALID
    # ... the order inside an item, and the first offending item decides
    assert call(it=items(pStream=room[1].data_ptr() + 8, capacity=0, reserved=1)) == INVALID and call(it=items(capacity=0, reserved=1)) == BOUNDS
    assert call(it=items(capacity=0, also2={"pIn": None})) == BOUNDS and call(it=items(reserved=1, also2={"capacity": 0})) == INVALID
    assert call(it=items(sizeX=0), count=1) == 0  # (item 1 is not part of a list of one)
    # 4. count == 0: success with nothing done
    assert call(count=0) == 0 and host(gpu.ctx, 0, items(), SIZE, 1, sizes, 0, 1) == 0
    torch.cuda.synchronize()
    assert all(int((r[bounds[0] if k == 0 else 0:] != 0x5A).sum()) == 0 for k, r in enumerate(room)), "a refused call wrote to an output buffer"
    assert list(sizes)[1:] == [0x5A5A] * (n - 1), "a refused call wrote to pBytes"
    # the context is usable, the same arguments are accepted, and a larger itemSize is a newer caller's struct
    good, wide = items(), (C.c_uint8 * (48 * n))()  # (`good` stays alive while it is copied from)
    for k in range(n):
        C.memmove(C.addressof(wide) + 48 * k, C.addressof(good) + 40 * k, 40)
    assert dev(gpu.ctx, n, wide, 48, 1, sizes, 0, 1, None) == 0
    first = list(sizes)
    assert call() == 0 and list(sizes) == first and all(64 + (w // 8) * (h // 8) * 56 <= s <= b for s, b, (w, h) in zip(sizes, bounds, shapes))
    assert [int(r[:64].cpu().numpy().view(S.HEADER)[0]["errorFactor"]) for r in room] == [0, 100, 401]
    gpu.check()


def test_host_form_capacity_rule(gpu, lists):
    """a capacity below that stream's bytes: all sizes are reported, no stream is written, OutOfBounds"""
    imgs, alpha, efs, _, streams, _ = lists["scan_slices"]
    imgs = [np.ascontiguousarray(i) for i in imgs]
    outs = [np.full(s.size + 64, 0x5A, dtype=np.uint8) for s in streams]
    it = (StreamListItem * len(imgs))()
    for k, (i, o, ef) in enumerate(zip(imgs, outs, efs)):
        it[k] = StreamListItem(i.ctypes.data, o.ctypes.data, streams[k].size - (1 if k == 2 else 0), i.shape[1], i.shape[0], ef, 0)
    sizes = (C.c_size_t * len(imgs))()
    assert gpu.lib.limg_hip_encode_stream_list(gpu.ctx, len(imgs), it, C.sizeof(StreamListItem), int(alpha), sizes, 0, 1) == 103
    assert list(sizes) == [s.size for s in streams]
    assert all(int((o != 0x5A).sum()) == 0 for o in outs)
    it[2].capacity = streams[2].size
    assert gpu.lib.limg_hip_encode_stream_list(gpu.ctx, len(imgs), it, C.sizeof(StreamListItem), int(alpha), sizes, 0, 1) == 0
    _same([o[:s.size] for o, s in zip(outs, streams)], streams, "exact capacities")
    assert all(int((o[s.size:] != 0x5A).sum()) == 0 for o, s in zip(outs, streams))


def test_context_memory(lib, lists):
    """limg_hip_context_device_bytes: what the header states for the chunk -- the per-image factor planes, 4 bytes per strip, the per-block scratch, the look-back, the
    tables -- on top of what a single encode of the list's most demanding image holds; a second call grows nothing; a closed context gave back everything"""
    imgs, alpha, efs, kw, streams, _ = lists["edges"]
    live = (lambda: np.array(limg_amd.live_resources(limg_amd.load_library(L.TEST)), dtype=np.int64)) if lib == "test" else None
    base = live() if live else None
    up = lambda v, a: (v + a - 1) // a * a  # noqa: E731
    n = len(imgs)
    blocks = sum((i.shape[0] // 8) * (i.shape[1] // 8) for i in imgs)
    strips = sum((i.shape[0] // 8) * ((i.shape[1] // 8 + 31) // 32) for i in imgs)
    tables = 0
    for entry in (160, 64, 96, 32, 32, 4, 4):  # view, ListImage, ImageIO, RatedImage, StreamImage, two prefix words
        tables = up(tables + n * entry, 16)
    stated = sum(3 * up(i.size, 256) for i in imgs) + 4 * strips + blocks * (64 + 4 + 16) + 32 + 8 * strips + tables + 32 * n + 8 * n
    import torch
    dimgs = _to_device(imgs)  # (the device form: no staging of a host form in the count)
    one = L.open_context(lib)
    for i in dimgs:
        one.encode_stream_device(i, alpha, error_factor=100)
    single = one.device_bytes()
    one.close()
    g = L.open_context(lib)
    outs, sizes = g.encode_stream_list_device(dimgs, alpha, efs, **kw)
    torch.cuda.synchronize()
    _same([o[:k].cpu().numpy() for o, k in zip(outs, sizes)], streams, "edges")
    held = g.device_bytes()
    print("device bytes: the list", held, "stated for the chunk", stated, "the single calls' context", single)
    assert stated <= held <= stated + single, (held, stated, single)
    g.encode_stream_list_device(dimgs, alpha, efs, **kw)
    assert g.device_bytes() == held
    if live:
        assert (live() - base)[1] == held
    g.check()
    g.close()
    if live:
        assert np.array_equal(live(), base), (live() - base).tolist()


def test_collect_stats(gpu, oracle, lists):
    """limg_hip_last_stats after the call: all images together = the sum of the single encodes' counters at their factors, whichever way each item went (three
    through the shared launches, one with partial edge blocks through the single call)"""
    imgs, alpha, efs, kw, _, _ = lists["edges"]
    imgs, efs = imgs[:3] + [_image(oracle, 13, 9, 1)], efs[:3] + [101]
    gpu.set_options(collect_stats=True)
    try:
        total, pixels = np.zeros(30, dtype=np.uint64), 0
        for i, ef in zip(imgs, efs):
            gpu.encode_stream(i, alpha, error_factor=ef)
            c, p = gpu.last_stats()
            total += c
            pixels += p
        gpu.encode_stream_list(imgs, alpha, efs, **kw)
        c, p = gpu.last_stats()
    finally:
        gpu.set_options()
    assert p == pixels == sum(i.size for i in imgs) and np.array_equal(c, total), (c, total)


def test_list_ends_a_pending_chain_phase(gpu):
    """the mixed chunk reuses the context's per-block scratch as any outer encode does: a chain encode's phase 1 that was pending is gone, and its phase 2 is
    refused (InvalidParameter) instead of running the F step on the list's records"""
    import torch
    strip = torch.zeros((16, 256), dtype=torch.int32, device="cuda")
    planes = gpu.alloc_planes_device(256, 16)
    calls, base = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
    gpu.encode3d_chain_device(strip, True, planes, 1, calls=calls)
    gpu.encode3d_chain_device(strip, True, planes, 2, base=base)  # (with nothing in between, the same arguments are accepted)
    gpu.encode3d_chain_device(strip, True, planes, 1, calls=calls)
    imgs = [torch.zeros((h, w), dtype=torch.int32, device="cuda") for w, h in ((256, 8), (8, 8))]  # two eligible shapes: one chunk through the shared launches
    gpu.encode_stream_list_device(imgs, True, [100, 37])
    with pytest.raises(limg_amd.LimgHipError, match="limg_hip_result 101"):
        gpu.encode3d_chain_device(strip, True, planes, 2, base=base)
    torch.cuda.synchronize()
    gpu.check()


L.product_twins(globals())  # test_x_product: the same tests on the product library (tests/lib_axis.py)
