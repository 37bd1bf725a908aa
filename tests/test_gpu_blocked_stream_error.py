"""Error windows of the version 2 stream (limg_hip_blocked_decode_stream_windows_error*, k_bstream_windows_map + k_bstream_windows_error) and limg_hip_stream_compare on
version 2 streams: tests/test_gpu_stream_error.py for the merged-block encoder's streams, against the oracle's limg_blocked_encode3d_test pDecoded.  A malformed
rectangle refuses every job of its stream and no job of another (tests/stream_error_cases.py)."""
import numpy as np
import pytest

import lib_axis as L
import limg_amd
from oracle import blocked_stream as B
from stream_error_cases import SHAPES, SUM_SENTINEL, Layout, Version, host_form_refusals, host_refusals, images, jobs_of, random_original, run, sums_tensor, windows
from stream_error_ref import error_sum
from window_batch import device_stream

pytestmark = pytest.mark.gpu
V = Version(blocked=True)


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


@pytest.mark.parametrize("name", [s[0] for s in SHAPES])
def test_sums_against_the_restatement(gpu, oracle, name):
    layout = Layout()
    jobs, want = jobs_of(V, gpu, oracle, name, layout)
    assert len(jobs) == 4 * len(windows(*images(oracle, V)[name][0].shape[::-1]))
    got = run(V, gpu, jobs, want, layout, name)
    assert got[0] != got[2], "the random original must differ from the image's own error"
    # the host form: the same windows of the one stream, the originals as strided views of the full images
    img, alpha, channels, dec = images(oracle, V)[name]
    h, w = img.shape
    rnd = random_original(w, h, 5)
    wins = windows(w, h)
    st = gpu.blocked_encode_stream(img, alpha)
    for original in (img, rnd):
        before = original.copy()
        sums = gpu.blocked_decode_stream_windows_error(st, wins, [original[y:y + hh, x:x + ww] for x, y, ww, hh in wins])
        assert sums == [error_sum(dec, original, channels, win) for win in wins], name
        assert np.array_equal(original, before)


def test_one_call_of_many_jobs_over_three_streams(gpu, oracle):
    """more than 70 jobs over three streams of different shapes, in an order that mixes the streams: the sums of the single-job calls"""
    import torch
    layout = Layout()
    jobs, want = [], []
    for k, name in enumerate(("536x24", "520x16_rgb", "75x21")):
        j, w = jobs_of(V, gpu, oracle, name, layout, first_seed=200 + 10 * k)
        jobs += j + j[:8]
        want += w + w[:8]
    order = np.random.RandomState(3).permutation(len(jobs))
    jobs, want = [jobs[i] for i in order], [want[i] for i in order]
    assert len(jobs) >= 70 and len({j[0].data_ptr() for j in jobs}) == 3
    got = run(V, gpu, jobs, want, layout, "three streams")
    single = [int(gpu.blocked_decode_stream_windows_error_device([j])[0]) for j in jobs]
    torch.cuda.synchronize()
    assert single == got


def test_a_refused_job_changes_no_other_sum(gpu, oracle):
    import torch
    img, alpha, channels, dec = images(oracle, V)["536x24"]
    img2, alpha2, channels2, dec2 = images(oracle, V)["75x21"]
    st, st2 = gpu.blocked_encode_stream(img, alpha), gpu.blocked_encode_stream(img2, alpha2)
    evil = st.copy()
    n = len(B.parse(st)[1])
    evil[64:64 + 64 * n].view(B.RECT)["payloadWord"][n // 2] = 0x7FFFFFF0  # a rectangle whose payload lies past the stream's end: its whole stream is refused
    layout = Layout()
    o1, s1 = layout.add(img, False)
    o2, s2 = layout.add(img2, True)
    jobs = [(device_stream(st), st.size, 536, 24, 0, 0, 536, 24, o1, s1), (device_stream(evil), st.size, 536, 24, 0, 0, 536, 24, o1, s1),
            (device_stream(st2), st2.size, 75, 21, 0, 0, 75, 21, o2, s2)]
    big, sums = sums_tensor(3)
    status = torch.full((3,), 77, dtype=torch.int32, device="cuda")
    gpu.blocked_decode_stream_windows_error_device(jobs, sums=sums, status=status)
    torch.cuda.synchronize()
    with pytest.raises(limg_amd.LimgHipError):
        gpu.check()
    gpu.check()  # reported once
    got, s = sums.cpu().tolist(), status.cpu().tolist()
    assert s[0] == 0 and s[2] == 0 and s[1] != 0, s
    assert got[0] == error_sum(dec, img, channels) and got[2] == error_sum(dec2, img2, channels2), got
    assert big[:2].cpu().tolist() == [SUM_SENTINEL] * 2 and big[-2:].cpu().tolist() == [SUM_SENTINEL] * 2 and layout.untouched()
    # the host form hands no sum back for a stream that is refused for any window
    with pytest.raises(limg_amd.LimgHipError):
        gpu.blocked_decode_stream_windows_error(evil, [(0, 0, 8, 8), (0, 0, 536, 24)], [img[:8, :8], img])
    gpu.check()


def test_host_refusals(gpu, oracle):
    img, alpha, _, _ = images(oracle, V)["536x24"]
    st = gpu.blocked_encode_stream(img, alpha)
    host_refusals(V, gpu, device_stream(st), st.size, 536, 24)
    host_form_refusals(V, gpu, st, 536, 24)


def test_stream_compare(gpu, oracle):
    """the value and mse of compare(original, decode_stream(stream)) -- the oracle's, and this library's own two-step path"""
    for name, (img, alpha, channels, dec) in images(oracle, V).items():
        h, w = img.shape
        st = gpu.blocked_encode_stream(img, alpha)
        for original in (img, random_original(w, h, 9)):
            psnr, mse = gpu.stream_compare(st, original)
            want = oracle.compare(original, dec, alpha)
            own = gpu.compare(original, gpu.blocked_decode_stream(st), alpha)
            assert mse == want[1] == own[1] and round(mse * w * h) == error_sum(dec, original, channels), (name, mse, want, own)
            assert psnr == pytest.approx(want[0], abs=1e-9) and psnr == own[0], (name, psnr, want, own)
    # refusals are NaN: pixels that do not match the header, a header that is no stream's, a NULL pointer
    assert np.isnan(gpu.stream_compare(st, img[:, :-1])[0])
    bad = st.copy()
    bad[0] ^= 0xFF
    assert np.isnan(gpu.stream_compare(bad, img)[0]) and np.isnan(gpu.stream_compare(st[:32], img)[0])
    assert np.isnan(gpu.lib.limg_hip_stream_compare(gpu.ctx, None, st.size, img.ctypes.data, img.size, None, None))
    gpu.check()


L.product_twins(globals())
