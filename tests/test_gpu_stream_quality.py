"""limg_hip_encode_stream_quality(_device) and its list form: the stream encode to a quality target -- one ordinary stream encode, one error launch over the whole
image (k_stream_windows_error) and one download per probe, stepped by limg_hip_quality_step.h -- on the shapes of the error tests and one of whole strips:

  8 x 8 photo-noise            one block
  536 x 24 gradient, alpha     two units per block row, the second of 3 blocks
  520 x 16 RGB photo-noise     3 channels: no alpha term; the documented non-monotone curve
  75 x 21 gradient             partial edge blocks on both axes: the ragged encode
  128 x 64 photo-noise         the list form's shape

E(h) comes from the ORACLE (mse x pixels of compare(image, pDecoded) at error factor 2 h, memoised); the call's choice, verdict, probe count and error sum must equal
the search of include/limg_hip.h restated in Python (tests/stream_error_ref.py) over it, bytes the stream's length, and the stream limg_hip_encode_stream's at the chosen
error factor byte for byte."""
import ctypes as C

import numpy as np
import pytest

import lib_axis as L
import limg_amd
from rate_search import max_probes
from stream_error_ref import oracle_error_sum, restated_quality_search

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


# (name, width, height, alpha, generator, seed)
SHAPES = (("8x8", 8, 8, True, "photo_noise", 3), ("536x24", 536, 24, True, "gradient_alpha", 7), ("520x16_rgb", 520, 16, False, "photo_noise", 11),
          ("75x21", 75, 21, True, "gradient_alpha", 13), ("128x64", 128, 64, True, "photo_noise", 17))
_REF = {}


def _image(oracle, name):
    """(img, alpha, E) of a shape; E(h, **kw) is the oracle's error sum at error factor 2 h, memoised: computed once, shared, never changed"""
    if name not in _REF:
        _, w, h, alpha, kind, seed = next(s for s in SHAPES if s[0] == name)
        img = oracle.photo_noise(w, h, seed) if kind == "photo_noise" else oracle.random_gradient(w, h, seed, False)
        memo = {}

        def E(hh, **kw):
            key = (hh, tuple(sorted(kw.items())))
            if key not in memo:
                memo[key] = oracle_error_sum(oracle, img, alpha, 2 * hh, **kw)
            return memo[key]

        _REF[name] = (img, alpha, E)
    return _REF[name]


def _limits(E, h_lo=1, h_hi=64):
    return [E(h_lo) - 1, E(h_lo), E(h_hi), E(h_hi) + 1, E(h_hi) - 1, (E(h_lo) + E(h_hi)) // 2, E((h_lo + h_hi) // 2)]


def _outcome(res, hi_ef):
    return "refused" if not res.withinTarget else ("upper bound" if res.errorFactor == hi_ef else "bisected")


def _quality_case(gpu, img, alpha, E, limit, lo_ef, hi_ef, ctx, **kw):
    """one quality call against the restated search over E(h); lo_ef / hi_ef as handed to the call (0: the defaults)"""
    h_lo, h_hi = (lo_ef or 2) // 2, (hi_ef or 1024) // 2
    want_h, within, asked, esum = restated_quality_search(lambda hh: E(hh, **kw), h_lo, h_hi, limit)
    st, res = gpu.encode_stream_quality(img, alpha, limit, lo_ef, hi_ef, **kw)
    print(ctx, limit, (res.errorFactor, res.withinTarget, res.probes, res.errorSum, res.bytes), (2 * want_h, within, asked, esum))
    assert (res.errorFactor, res.withinTarget, res.probes, res.errorSum) == (2 * want_h, within, len(asked), esum), (ctx, limit)
    assert res.probes <= max_probes(h_lo, h_hi) and st.size == res.bytes, (ctx, limit)
    assert bool(within) == (res.errorSum <= limit), (ctx, limit)
    assert np.array_equal(st, gpu.encode_stream(img, alpha, error_factor=res.errorFactor, **kw)), (ctx, limit)
    return res


@pytest.mark.parametrize("name", [s[0] for s in SHAPES])
def test_quality_against_the_restated_search(gpu, oracle, name):
    img, alpha, E = _image(oracle, name)
    assert E(1) > 0 and E(1) < E(64), name
    outcomes = {_outcome(_quality_case(gpu, img, alpha, E, limit, 2, 128, name), 128) for limit in _limits(E)}
    assert outcomes == {"refused", "upper bound", "bisected"}, name  # (every shape alone yields all three with these limits)


def test_the_documented_non_monotone_case(gpu, oracle):
    """520 x 16 RGB photo-noise seed 11: E(36) = 654054, E(37) = 672780, E(38) = 670651.  A limit of 670651 over [2, 128] returns errorFactor 72 after 8 probes
    (h = 1, 64, 33, 49, 41, 37, 35, 36), although 76 would also meet it: the result is the search's, not the largest value that meets the limit."""
    img, alpha, E = _image(oracle, "520x16_rgb")
    assert (E(36), E(37), E(38)) == (654054, 672780, 670651)
    assert restated_quality_search(E, 1, 64, 670651)[2] == [1, 64, 33, 49, 41, 37, 35, 36]
    res = _quality_case(gpu, img, alpha, E, 670651, 2, 128, "non-monotone")
    assert (res.errorFactor, res.withinTarget, res.probes, res.errorSum) == (72, 1, 8, 654054)


def test_bounds_and_options(gpu, oracle):
    img, alpha, E = _image(oracle, "128x64")
    # both bounds at 0: the defaults 2 and 1024
    for limit in (E(1), (E(1) + E(512)) // 2, E(512)):
        _quality_case(gpu, img, alpha, E, limit, 0, 0, "defaults")
    # hLo == hHi asks once, whatever the limit
    for limit in (E(20) - 1, E(20)):
        res = _quality_case(gpu, img, alpha, E, limit, 40, 40, "one value")
        assert (res.errorFactor, res.probes, res.withinTarget) == (40, 1, int(limit >= E(20)))
    # maxErrorSum == 0 is allowed: it asks for a lossless image, which no error factor gives here
    res = _quality_case(gpu, img, alpha, E, 0, 2, 128, "lossless")
    assert (res.errorFactor, res.withinTarget, res.probes) == (2, 0, 1)
    # the accurate search, and a thread pool of 2 (it moves the dither chains, and with them the error), against the oracle in the same configuration
    _quality_case(gpu, img, alpha, E, (E(1, fast=False) + E(64, fast=False)) // 2, 2, 128, "accurate", fast=False)
    img2, alpha2, E2 = _image(oracle, "536x24")
    _quality_case(gpu, img2, alpha2, E2, (E2(1, pool_threads=2) + E2(64, pool_threads=2)) // 2, 2, 128, "pool 2", pool_threads=2)
    # a PSNR target through the helper: the comparison the search makes is errorSum <= limit
    limit = gpu.error_sum_for_psnr(128, 64, alpha, 38.0)
    res = _quality_case(gpu, img, alpha, E, limit, 2, 128, "38 dB")
    psnr = gpu.stream_compare(gpu.encode_stream(img, alpha, error_factor=res.errorFactor), img)[0]
    assert (psnr >= 38.0) == bool(res.withinTarget), (psnr, limit, res.errorSum)


def _five(oracle):
    """five 128 x 64 photo-noise images and their memoised E(h)"""
    imgs = [oracle.photo_noise(128, 64, 17 + k) for k in range(5)]

    def curve(img):
        memo = {}

        def E(hh):
            if hh not in memo:
                memo[hh] = oracle_error_sum(oracle, img, True, 2 * hh)
            return memo[hh]
        return E

    return imgs, [curve(img) for img in imgs]


def test_list_form(gpu, oracle):
    """five 128 x 64 images whose limits land on all three outcomes in ONE call: results and streams are the five single calls'; a list of one; count == 0"""
    import torch
    imgs, Es = _five(oracle)
    limits = [Es[0](1) - 1, Es[1](64), (Es[2](1) + Es[2](64)) // 2, Es[3](32), Es[4](64) + 1]
    want = [restated_quality_search(E, 1, 64, lim) for E, lim in zip(Es, limits)]
    streams, results = gpu.encode_stream_quality_batch(imgs, True, limits, 2, 128)
    got = [(r.errorFactor, r.withinTarget, r.probes, r.errorSum) for r in results]
    print(got, want)
    assert got == [(2 * h, within, len(asked), esum) for h, within, asked, esum in want]
    assert {_outcome(r, 128) for r in results} == {"refused", "upper bound", "bisected"}
    for img, lim, st, r in zip(imgs, limits, streams, results):
        one, res = gpu.encode_stream_quality(img, True, lim, 2, 128)
        assert (res.errorFactor, res.withinTarget, res.probes, res.errorSum, res.bytes) == (r.errorFactor, r.withinTarget, r.probes, r.errorSum, r.bytes)
        assert st.size == r.bytes and np.array_equal(st, one) and np.array_equal(st, gpu.encode_stream(img, True, error_factor=r.errorFactor))
    # the device form, into the caller's buffers; one shared limit
    dimgs = [torch.from_numpy(i.view(np.int32)).cuda() for i in imgs]
    outs, dres = gpu.encode_stream_quality_batch_device(dimgs, True, limits, 2, 128)
    torch.cuda.synchronize()
    assert all(np.array_equal(o[:r.bytes].cpu().numpy(), st) for o, r, st in zip(outs, dres, streams))
    # a list of one is the single call; an empty list succeeds
    st1, r1 = gpu.encode_stream_quality_batch(imgs[2:3], True, limits[2], 2, 128)
    assert np.array_equal(st1[0], streams[2]) and (r1[0].errorFactor, r1[0].probes, r1[0].errorSum) == (results[2].errorFactor, results[2].probes, results[2].errorSum)
    assert gpu.encode_stream_quality_batch([], True, 5, 2, 128) == ([], [])
    assert gpu.encode_stream_quality_batch_device([], True, 5, 2, 128)[1] == []
    gpu.check()


def _result():
    return limg_amd.QualityResult(C.sizeof(limg_amd.QualityResult), 7, 7, 7, 7, 7)


def test_errors(gpu, oracle):
    """the contract's refusals, in its order, each before anything touches the device: the output buffers keep their pattern, the results their values"""
    import torch
    W, H = 64, 16
    bound = gpu.stream_bound(W, H)
    img = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    room = torch.full((bound + 256,), 0x5A, dtype=torch.uint8, device="cuda")
    res = _result()
    dev, host = gpu.lib.limg_hip_encode_stream_quality_device, gpu.lib.limg_hip_encode_stream_quality
    NULL_, INVALID, BOUNDS = 102, 101, 103

    def call(ctx=gpu.ctx, pin=img.data_ptr(), w=W, h=H, pout=room.data_ptr(), cap=bound, limit=5000, lo=0, hi=0, pres=C.byref(res)):
        return dev(ctx, pin, w, h, 1, pout, cap, limit, lo, hi, 0, 1, pres, None)

    assert call(ctx=None) == NULL_ and call(pin=None) == NULL_ and call(pout=None) == NULL_ and call(pres=None) == NULL_
    assert call(w=0) == INVALID and call(h=0) == INVALID and call(w=1 << 31) == INVALID
    assert call(cap=bound - 1) == BOUNDS
    assert call(pout=room.data_ptr() + 8) == INVALID
    for bad in ({"lo": 3}, {"hi": 101}, {"lo": 1}, {"hi": 1}, {"lo": 200, "hi": 100}, {"lo": 2000}):
        assert call(**bad) == INVALID, bad
    short = _result()
    short.struct_size = 24
    assert call(pres=C.byref(short)) == INVALID
    assert call(w=0, cap=0) == INVALID and call(cap=bound - 1, pout=room.data_ptr() + 8) == BOUNDS and call(cap=bound - 1, lo=3) == BOUNDS  # the order
    host_img, host_out = np.zeros((H, W), dtype=np.uint32), np.full(bound, 0x5A, dtype=np.uint8)
    hp, ho = host_img.ctypes.data, host_out.ctypes.data
    assert host(None, hp, W, H, 1, ho, bound, 5000, 0, 0, 0, 1, C.byref(res)) == NULL_
    assert host(gpu.ctx, hp, W, H, 1, ho, bound, 5000, 0, 0, 0, 1, None) == NULL_
    assert host(gpu.ctx, hp, 0, H, 1, ho, bound, 5000, 0, 0, 0, 1, C.byref(res)) == INVALID
    assert host(gpu.ctx, hp, W, H, 1, ho, bound, 5000, 4, 2, 0, 1, C.byref(res)) == INVALID
    # the list forms: pointers (the arrays, then the elements), the shape, the capacity, the alignment, the bounds, a struct_size -- whichever element it is
    bdev, bhost = gpu.lib.limg_hip_encode_stream_quality_batch_device, gpu.lib.limg_hip_encode_stream_quality_batch
    ins, outs = (C.c_void_p * 2)(img.data_ptr(), img.data_ptr()), (C.c_void_p * 2)(room.data_ptr(), room.data_ptr() + 128)
    limits = (C.c_uint64 * 2)(5000, 0)
    results = (limg_amd.QualityResult * 2)(_result(), _result())

    def bcall(ctx=gpu.ctx, n=2, pins=ins, w=W, pouts=outs, cap=bound, plim=limits, lo=0, hi=0, pres=results):
        return bdev(ctx, n, pins, w, H, 1, pouts, cap, plim, lo, hi, 0, 1, pres, None)

    assert bcall(ctx=None) == NULL_ and bcall(pins=None) == NULL_ and bcall(pouts=None) == NULL_ and bcall(plim=None) == NULL_ and bcall(pres=None) == NULL_
    assert bcall(pins=(C.c_void_p * 2)(img.data_ptr(), None)) == NULL_ and bcall(pouts=(C.c_void_p * 2)(room.data_ptr(), None)) == NULL_
    assert bcall(w=0) == INVALID and bcall(cap=bound - 1) == BOUNDS and bcall(pouts=(C.c_void_p * 2)(room.data_ptr(), room.data_ptr() + 8)) == INVALID
    assert bcall(lo=3) == INVALID and bcall(lo=4, hi=2) == INVALID and bcall(n=0, lo=3) == INVALID
    results[1].struct_size = 24
    assert bcall() == INVALID
    results[1].struct_size = C.sizeof(limg_amd.QualityResult)
    assert bcall(cap=bound - 1, lo=3) == BOUNDS and bcall(w=0, cap=0) == INVALID  # the order
    assert bcall(n=0) == 0
    hins, houts = (C.c_void_p * 2)(hp, hp), (C.c_void_p * 2)(ho, ho)
    assert bhost(None, 2, hins, W, H, 1, houts, bound, limits, 0, 0, 0, 1, results) == NULL_ and bhost(gpu.ctx, 2, hins, W, H, 1, houts, bound, None, 0, 0, 0, 1, results) == NULL_
    assert bhost(gpu.ctx, 2, hins, W, H, 1, houts, bound, limits, 3, 0, 0, 1, results) == INVALID and bhost(gpu.ctx, 0, hins, W, H, 1, houts, bound, limits, 0, 0, 0, 1, results) == 0
    torch.cuda.synchronize()
    assert int((room != 0x5A).sum()) == 0 and int((host_out != 0x5A).sum()) == 0, "a refused call wrote to an output buffer"
    for r in (res, results[0], results[1]):
        assert (r.errorFactor, r.probes, r.withinTarget, r.bytes, r.errorSum) == (7, 7, 7, 7, 7), "a refused call wrote a result"
    # the context is usable, and the same arguments are accepted: the flat image's search is the restated one over the oracle's E -- the upper bound after two probes
    want_h, within, asked, esum = restated_quality_search(lambda hh: oracle_error_sum(oracle, host_img, True, 2 * hh), 1, 512, 5000)
    assert call() == 0 and (res.errorFactor, res.withinTarget, res.probes, res.errorSum) == (2 * want_h, within, len(asked), esum) == (1024, 1, 2, esum)
    assert res.bytes == gpu.encode_stream(host_img, True, error_factor=1024).size
    # the host form's capacity rule: the result is filled, limg_hip_error_OutOfBounds comes back and nothing is written
    res2 = _result()
    assert host(gpu.ctx, hp, W, H, 1, ho, 64, 5000, 0, 0, 0, 1, C.byref(res2)) == BOUNDS
    assert (res2.errorFactor, res2.bytes) == (1024, res.bytes) and int((host_out != 0x5A).sum()) == 0
    gpu.check()


L.product_twins(globals())
