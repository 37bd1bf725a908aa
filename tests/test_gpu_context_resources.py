"""A context owns its GPU resources through its members (limg_amd/csrc/limg_hip_owned.h) and limg_hip_shutdown is `delete`: whatever a context took -- device
buffers and their bytes, pinned buffers, streams, events -- is back when it is closed, whichever entry families ran on it.  Asserted exactly, on the counts the test build
keeps (limg_hip_test_live_resources): the tests are about that hook, so they run on the test build only (tests/lib_axis.py HOOK_ONLY).  Every test measures against the
numbers it finds when it starts: contexts of other modules' fixtures may be alive."""
import gc

import numpy as np
import pytest

import lib_axis as L
import limg_amd
from oracle.bind import PLANES, BLOCKED_WRITTEN

pytestmark = pytest.mark.gpu

NAMES = ("device buffers", "device bytes", "pinned buffers", "streams", "events")


def _live():
    return np.array(limg_amd.live_resources(limg_amd.load_library(L.TEST)), dtype=np.int64)


def _baseline():
    gc.collect()  # (a context an earlier test dropped without closing it goes now, not in the middle of this test)
    return _live()


def _small_encodes(g, oracle, img64, want64, img96, want96):
    got = g.encode3d(img64, True)
    for k in PLANES:
        assert np.array_equal(want64[k], got[k]), k
    gotb = g.blocked_encode3d(img96, True)
    for k in BLOCKED_WRITTEN:
        assert np.array_equal(want96[k], gotb[k]), k


@pytest.fixture(scope="module")
def small(oracle):
    """a 64 x 64 image and a 96 x 72 one with what the oracle makes of them (8x8 encode / merged-block encode)"""
    img64, img96 = oracle.photo_noise(64, 64, 3), oracle.random_gradient(96, 72, 5, False)
    return img64, oracle.encode3d(img64, True), img96, oracle.blocked_encode3d(img96, True)


def test_every_family_then_close(oracle, small):
    import torch
    img64, want64, img96, want96 = small
    base = _baseline()
    g = L.open_context("test")
    try:
        # the 8x8 encode with statistics and profiling: the counters' buffer, the profiling events
        g.set_options(collect_stats=True)
        g.profile_begin()
        got = g.encode3d(img64, True)
        assert g.profile_end().shape[0] == 1
        assert g.last_stats()[1] == 64 * 64
        for k in PLANES:
            assert np.array_equal(want64[k], got[k]), k
        g.set_options()
        # the accurate search: its table
        want = oracle.encode3d(img64, True, fast=False)
        got = g.encode3d(img64, True, fast=False)
        for k in PLANES:
            assert np.array_equal(want[k], got[k]), ("accurate", k)
        # a list in sub-batches: the float stage's stream and the events that fork / join it
        g.set_options(batch_sub_images=2)
        imgs = [oracle.photo_noise(64, 64, 10 + i) for i in range(4)]
        dimgs = [torch.from_numpy(i.view(np.int32)).cuda() for i in imgs]
        planes = [g.alloc_planes_device(64, 64) for _ in imgs]
        g.encode3d_batch_device(dimgs, True, planes)
        torch.cuda.synchronize()
        for i in (0, 3):
            want = oracle.encode3d(imgs[i], True)
            for k in PLANES:
                assert np.array_equal(want[k].view(np.uint8), planes[i][k].cpu().numpy().view(np.uint8)), ("batch", i, k)
        # partial edge blocks, in bands and in independent chains: pinned staging and its event, the bands' events, per-call noise
        g.set_options(ragged_bands=2)
        rag = oracle.photo_noise(67, 45, 4)
        for threads in (0, 2):
            want = oracle.encode3d(rag, True, pool_threads=threads)
            got = g.encode3d(rag, True, pool_threads=threads)
            for k in PLANES:
                assert np.array_equal(want[k], got[k]), ("ragged", threads, k)
        g.set_options()
        # the host-pointer entry in row bands (from 2048 x 2048 on): its two streams, the bands' events and words.  Against the device entry on the same image.
        dbig = g.synth_device("random_gradient", 2048, 2048, seed=7)
        big = dbig.cpu().numpy().view(np.uint32)
        got = g.encode3d(big, True)
        dplanes = g.alloc_planes_device(2048, 2048)
        g.encode3d_device(dbig, True, dplanes)
        torch.cuda.synchronize()
        for k in PLANES:
            assert np.array_equal(got[k].view(np.uint8), dplanes[k].cpu().numpy().view(np.uint8)), ("host bands", k)
        psnr, mse = g.compare_device(dbig, dplanes["pDecoded"], True)
        assert mse >= 0 and not np.isnan(psnr)
        del got, dplanes, big
        # the merged-block encoder: three streams, its events and timers, device and pinned buffers; then its stream packer
        gotb = g.blocked_encode3d(img96, True)
        for k in BLOCKED_WRITTEN:
            assert np.array_equal(want96[k], gotb[k]), k
        st2 = g.blocked_encode_stream(img96, True)
        assert np.array_equal(st2, g.blocked_last_stream(96, 72))
        assert np.array_equal(g.blocked_decode_stream(st2), want96["pDecoded"])
        # version 1 streams, single and as a list
        st1 = g.encode_stream(img64, True)
        assert np.array_equal(g.decode_stream(st1), want64["pDecoded"])
        batch = g.encode_stream_batch(imgs[:3], True)
        assert np.array_equal(batch[0], g.encode_stream(imgs[0], True)) and len(batch) == 3
        # batched window decode, 5 calls back to back per version: every slot of the ring, the first one twice
        for version, stream, (W, H), whole in ((1, st1, (64, 64), want64["pDecoded"]), (2, st2, (96, 72), want96["pDecoded"])):
            dst = torch.from_numpy(np.concatenate([stream, np.zeros(-stream.size % 16 + 16, dtype=np.uint8)])).cuda()
            decode = g.decode_stream_windows_device if version == 1 else g.blocked_decode_stream_windows_device
            outs = [decode([(dst, stream.size, W, H, 3 + c, 5, 40, 33, None, None), (dst, stream.size, W, H, 0, 0, W, H, None, None)]) for c in range(5)]
            torch.cuda.synchronize()
            for c, (win, full) in enumerate(outs):
                assert np.array_equal(full.cpu().numpy().view(np.uint32), whole), (version, c)
                assert np.array_equal(win.cpu().numpy().view(np.uint32), whole[5:38, 3 + c:43 + c]), (version, c)
        g.check()
        held = _live() - base
        print("held by one context after every family:", dict(zip(NAMES, held.tolist())), "device_bytes()", g.device_bytes())
        assert held[3] >= 6, held     # the sub-batch pipeline's, the host entry's two, the merged-block encoder's three
        assert held[4] > 0 and held[2] > 0 and held[0] > 0, held
        assert held[1] == g.device_bytes(), (held, g.device_bytes())
    finally:
        g.close()
    assert np.array_equal(_live(), base), dict(zip(NAMES, (_live() - base).tolist()))


def test_two_contexts(oracle, small):
    base = _baseline()
    a, b = L.open_context("test"), L.open_context("test")
    try:
        _small_encodes(a, oracle, *small)
        only_a = _live() - base
        assert only_a[1] == a.device_bytes() and b.device_bytes() == 0, (only_a, a.device_bytes(), b.device_bytes())
        _small_encodes(b, oracle, *small)
        both = _live() - base
        assert both[1] == a.device_bytes() + b.device_bytes(), (both, a.device_bytes(), b.device_bytes())
        assert np.array_equal(both, 2 * only_a), (both, only_a)  # the same calls, the same resources
        a_bytes = a.device_bytes()
        a.close()
        assert np.array_equal(_live() - base, both - only_a), (_live() - base, both, only_a)  # exactly A's share is gone
        assert both[1] - (_live() - base)[1] == a_bytes > 0
        assert (_live() - base)[1] == b.device_bytes()
        _small_encodes(b, oracle, *small)  # B is untouched by A's going
        b.check()
    finally:
        a.close()
        b.close()
    assert np.array_equal(_live(), base), dict(zip(NAMES, (_live() - base).tolist()))


def test_unused_context():
    base = _baseline()
    g = L.open_context("test")
    try:
        assert g.device_bytes() == 0
        assert np.array_equal(_live(), base)  # everything is made on first use
    finally:
        g.close()
    assert np.array_equal(_live(), base), dict(zip(NAMES, (_live() - base).tolist()))


def test_open_encode_close_cycles(oracle, small):
    base = _baseline()
    for round_ in range(6):
        g = L.open_context("test")
        try:
            _small_encodes(g, oracle, *small)
            assert (_live() - base)[1] == g.device_bytes() > 0
            g.check()
        finally:
            g.close()
        assert np.array_equal(_live(), base), (round_, dict(zip(NAMES, (_live() - base).tolist())))
