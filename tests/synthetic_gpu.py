"""What the GPU tests of the hand-built streams of both versions share (tests/test_gpu_synthetic_streams.py, tests/test_gpu_synthetic_blocked_streams.py): the corpus of
tests/synthetic_streams.py on the device in the form the shared bodies take -- (device stream, nbytes, W, H, the ORACLE's decode of the same bytes) -- and the calls
into those bodies (window_cases, window_batch, window_tensor, window_scaled, window_resized, stream_error_cases).  No comparison is written here.  Not a test module."""
import numpy as np

import stream_error_cases as E
import synthetic_streams as Y
import window_batch as WB
import window_resized as WR
import window_scaled as WS
import window_tensor as WT
from stream_error_ref import error_sum
from window_cases import device_window, host_window, windows

NAMES = {1: [s[0] for s in Y.V1], 2: [s[0] for s in Y.V2]}
TENSOR_FORMATS = [("float32", 3, "A"), ("float16", 3, "B"), ("float32", 4, "B"), ("float16", 4, "A")]
SCALED_MODES = ["rgba", ("float32", 3, "A"), ("float16", 4, "B")]
_DEVICE, _PYRAMIDS = {}, {}


def fmt_id(m):
    return WS.mode_id(m)


def by_name(version, name):
    return Y.corpus(version)[NAMES[version].index(name)]


def prefix(version):
    return "blocked_" if version == 2 else ""


def device(gpu, oracle, version):
    """[(device stream, nbytes, W, H, the oracle's decode)] of the version's corpus: uploaded once per library"""
    key = (gpu.library, version)
    if key not in _DEVICE:
        _DEVICE[key] = [(WB.device_stream(st.bytes), st.bytes.size, st.W, st.H, Y.decoded(st, oracle)) for st in Y.corpus(version)]
    return _DEVICE[key]


def with_pyramids(gpu, oracle, version):
    """the same with the pyramid of the oracle's decode in place of the decode (tests/window_scaled.py)"""
    out = []
    for st, (d, nbytes, W, H, want) in zip(Y.corpus(version), device(gpu, oracle, version)):
        if st.name not in _PYRAMIDS:
            _PYRAMIDS[st.name] = WS.pyramid(want)
        out.append((d, nbytes, W, H, _PYRAMIDS[st.name]))
    return out


def whole_decode(gpu, oracle, version, name):
    """the host and the device entry of the version's full decoder; a mismatch names the first blocks with their class, shift word and group kind"""
    import torch
    st = by_name(version, name)
    want = Y.decoded(st, oracle)
    got = getattr(gpu, prefix(version) + "decode_stream")(st.bytes)
    assert np.array_equal(got, want), Y.describe_mismatch(st, want, got)
    d, nbytes, W, H, _ = device(gpu, oracle, version)[NAMES[version].index(name)]
    out = getattr(gpu, prefix(version) + "decode_stream_device")(d, nbytes, W, H)
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint32)
    assert np.array_equal(got, want), Y.describe_mismatch(st, want, got)
    gpu.check()


def single_windows(gpu, oracle, version, name):
    st = by_name(version, name)
    d, nbytes, W, H, want = device(gpu, oracle, version)[NAMES[version].index(name)]
    for win in windows(W, H):
        host_window(getattr(gpu, prefix(version) + "decode_stream_window"), st.bytes, want, win)
        for unaligned in (False, True):
            device_window(getattr(gpu, prefix(version) + "decode_stream_window_device"), d, nbytes, W, H, want, win, unaligned)
    gpu.check()


def batched_windows(gpu, oracle, version):
    batch = WB.Batch()
    for d, nbytes, W, H, want in device(gpu, oracle, version):
        for win in windows(W, H):
            batch.add(d, nbytes, W, H, want, win, unaligned=bool(len(batch.jobs) & 1))
    WB.run_and_compare(gpu, getattr(gpu, prefix(version) + "decode_stream_windows_device"), getattr(gpu, prefix(version) + "decode_stream_window_device"), batch)


def tensor_windows(gpu, oracle, version, fmt):
    WT.mixed_batch(gpu, getattr(gpu, prefix(version) + "decode_stream_windows_tensor_device"), device(gpu, oracle, version), *fmt)


def scaled_windows(gpu, oracle, version, mode):
    WS.mixed_batch(gpu, version == 2, with_pyramids(gpu, oracle, version), mode)


def resized_windows(gpu, oracle, version, mode):
    WR.mixed_batch(gpu, version == 2, with_pyramids(gpu, oracle, version), mode)


def error_sums(gpu, oracle, version):
    """every stream's windows against a random original, densely and strided: the sums of the numpy restatement on the oracle's decode"""
    V = E.Version(blocked=version == 2)
    layout = E.Layout()
    jobs, want = [], []
    for k, (st, (d, nbytes, W, H, dec)) in enumerate(zip(Y.corpus(version), device(gpu, oracle, version))):
        original = E.random_original(W, H, 300 + k)
        for n, win in enumerate(E.windows(W, H) + [(5, 3, W - 9, H - 4)]):
            x, y, w, h = win
            t, stride = layout.add(original[y:y + h, x:x + w], strided=bool(n & 1))
            jobs.append((d, nbytes, W, H, x, y, w, h, t, stride))
            want.append(error_sum(dec, original, st.channels, win))
    E.run(V, gpu, jobs, want, layout, "hand-built streams, version %d" % version)
