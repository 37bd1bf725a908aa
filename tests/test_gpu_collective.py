"""Multi-GPU entries of the C ABI (include/limg_hip.h "multi-GPU") on ONE GPU: everything but the wire.
  * the cross-GPU single dither chain (== the reference with pThreadPool == nullptr, src/limg.cpp:1893,2110) through its two exchange-free halves
    `limg_hip_encode3d_chain_device`: four contexts play four ranks, the per-strip call totals are prefix-summed on the host exactly as the all-gather +
    k_chain_base would, and the assembled planes must equal the single-chain encode of the whole image;
  * a world-size-1 RCCL communicator (the real library, resolved at run time): `limg_hip_gather_stream` as a self-gather and
    `limg_hip_encode3d_single_chain_device` == the plain encode.
RCCL with more than one rank needs more than one GPU: unmeasured here (the driver's 8-GPU node runs bench.py --config 5 --single-chain)."""
import numpy as np
import pytest

import lib_axis as L
from lib_axis import lib, lib_product  # noqa: F401  (fixtures: "test" / "product")
from oracle.bind import PLANES

pytestmark = pytest.mark.gpu


def _np(planes):
    import torch
    return {k: v.cpu().numpy().view(np.uint32 if v.dtype == torch.int32 else np.uint8) for k, v in planes.items()}


@pytest.mark.parametrize("kind,alpha,ranks", [("pn", True, 4), ("rg", True, 2), ("pn", False, 8)])
def test_single_chain_across_emulated_ranks(oracle, kind, alpha, ranks, lib):
    import torch
    import limg_amd
    from limg_amd import shard
    W, H = 512, 256
    img = oracle.photo_noise(W, H, 21) if kind == "pn" else oracle.random_gradient(W, H, 21, True)
    want = oracle.encode3d(img, alpha)  # pool_threads = 0: ONE chain over the whole image
    d_img = torch.from_numpy(img.view(np.int32)).cuda()
    rows = shard.strip_rows(H, ranks)
    ctxs = [L.open_context(lib) for _ in range(ranks)]
    try:
        planes = [c.alloc_planes_device(W, y1 - y0) for c, (y0, y1) in zip(ctxs, rows)]
        calls = torch.zeros(ranks, dtype=torch.int64, device="cuda")
        before = [(y0 // 8) * (W // 8) for (y0, _) in rows]
        for r, (c, (y0, y1)) in enumerate(zip(ctxs, rows)):  # E step + scan on every "rank"
            c.encode3d_chain_device(d_img[y0:y1], alpha, planes[r], 1, calls=calls[r:r + 1], blocks_before=before[r])
        torch.cuda.synchronize()
        bases = limg_amd.host_chain_bases(calls.cpu().numpy().astype(np.uint64))  # what all-gather + k_chain_base compute on the device
        assert int(bases[0]) == 0 and all(int(bases[r + 1]) - int(bases[r]) == int(calls[r]) for r in range(ranks - 1))
        d_bases = torch.from_numpy(bases.astype(np.int64)).cuda()
        for r, (c, (y0, y1)) in enumerate(zip(ctxs, rows)):  # F step from the exchanged chain position
            c.encode3d_chain_device(d_img[y0:y1], alpha, planes[r], 2, base=d_bases[r:r + 1], blocks_before=before[r])
        torch.cuda.synchronize()
        for r, (y0, y1) in enumerate(rows):
            got = _np(planes[r])
            for k in PLANES:
                assert np.array_equal(got[k], want[k][y0:y1]), (r, k)
        # and the contexts are still good for ordinary encodes afterwards
        g = ctxs[0].encode3d(img, alpha)
        for k in PLANES:
            assert np.array_equal(g[k], want[k]), k
    finally:
        for c in ctxs:
            c.check()
            c.close()


def test_chain_entry_refuses_what_it_cannot_chain(oracle, lib):
    import torch
    import limg_amd
    g = L.open_context(lib)
    try:
        img = torch.zeros((20, 30), dtype=torch.int32, device="cuda")  # partial edge blocks: the chain position is not a table index
        planes = g.alloc_planes_device(30, 20)
        calls = torch.zeros(1, dtype=torch.int64, device="cuda")
        with pytest.raises(limg_amd.LimgHipError):
            g.encode3d_chain_device(img, True, planes, 1, calls=calls)
        with pytest.raises(limg_amd.LimgHipError):
            g.encode3d_single_chain_device(torch.zeros((64, 64), dtype=torch.int32, device="cuda"), True, g.alloc_planes_device(64, 64), 0)  # no communicator yet
        # phase 2 without a pending phase 1 of the same strip: refused (the context holds the strip's intermediate results between the two)
        strip = torch.zeros((64, 64), dtype=torch.int32, device="cuda")
        planes = g.alloc_planes_device(64, 64)
        base = torch.zeros(1, dtype=torch.int64, device="cuda")
        with pytest.raises(limg_amd.LimgHipError):
            g.encode3d_chain_device(strip, True, planes, 2, base=base)
        g.encode3d_chain_device(strip, True, planes, 1, calls=calls)
        g.encode3d_device(strip, True, planes)  # any other encode reuses the scratch ...
        with pytest.raises(limg_amd.LimgHipError):
            g.encode3d_chain_device(strip, True, planes, 2, base=base)  # ... so the pending phase 1 is gone
    finally:
        g.close()


def test_rccl_world_of_one(oracle, lib):
    """The real RCCL through the C ABI with a communicator of one rank: id, init, the gather (degenerates to the local copy after the size all-gather),
    the single-chain encode (its all-gather is a copy), destroy.  Checks the dlopen path, the argument plumbing and the stream ordering."""
    import torch
    import limg_amd
    g = L.open_context(lib)
    try:
        g.comm_init(g.comm_unique_id(), 0, 1)
        W, H = 512, 128
        img = oracle.photo_noise(W, H, 31)
        want = oracle.encode3d(img, True)
        d_img = torch.from_numpy(img.view(np.int32)).cuda()
        st, n = g.encode_stream_device(d_img, True)
        out = torch.zeros(g.stream_bound(W, H) + 64, dtype=torch.uint8, device="cuda")
        got, offs = g.gather_stream(st, n, root=0, out=out)
        torch.cuda.synchronize()
        assert int(offs[0]) == 0 and int(offs[1]) == (n + 15) // 16 * 16
        assert torch.equal(got[:n], st[:n])
        dec = g.decode_stream_device(got, n, W, H)
        torch.cuda.synchronize()
        assert np.array_equal(dec.cpu().numpy().view(np.uint32), want["pDecoded"])
        # an output buffer that is too small: refused (the decision is taken from all-gathered numbers, so every rank of a larger job refuses alike)
        small = torch.zeros((n // 2 + 15) // 16 * 16, dtype=torch.uint8, device="cuda")
        with pytest.raises(limg_amd.LimgHipError):
            g.gather_stream(st, n, root=0, out=small)
        torch.cuda.synchronize()
        planes = g.alloc_planes_device(W, H)
        g.encode3d_single_chain_device(d_img, True, planes, 0)
        torch.cuda.synchronize()
        got = _np(planes)
        for k in PLANES:
            assert np.array_equal(got[k], want[k]), k
        g.check()
        if L.has_hooks(g):
            # abort rule: a rank whose E step failed (test hook) still joins the all-gather -- with a poison value -- and returns its error; the call comes back
            # (no rank is left waiting), no plane is written, and the context reports the aborted chain once
            for v in planes.values():
                v.zero_()
            g.set_options(test_fail_chain_phase1=True)
            try:
                with pytest.raises(limg_amd.LimgHipError):
                    g.encode3d_single_chain_device(d_img, True, planes, 0)
            finally:
                g.set_options()
            torch.cuda.synchronize()
            assert all(int(v.count_nonzero().item()) == 0 for v in planes.values())
            with pytest.raises(limg_amd.LimgHipError):
                g.check()  # "a rank of the communicator aborted a single-chain encode"
            g.check()      # sticky until reported once
            g.encode3d_single_chain_device(d_img, True, planes, 0)  # and the context goes on working
            torch.cuda.synchronize()
            got = _np(planes)
            for k in PLANES:
                assert np.array_equal(got[k], want[k]), k
        g.comm_destroy()
        g.check()
    finally:
        g.close()


RANK_SCRIPT = r"""
import os, sys
import numpy as np
sys.path.insert(0, os.environ["LIMG_ROOT"])
import torch
import torch.distributed as dist
import limg_amd
from limg_amd import shard
from oracle.bind import Oracle, PLANES
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
torch.cuda.set_device(rank)
dist.init_process_group("nccl", device_id=torch.device("cuda", rank))
orc = Oracle()
W, H = 512, 256
img = orc.photo_noise(W, H, 21)
want = orc.encode3d(img, True)                      # ONE chain over the whole image
rows = shard.strip_rows(H, world)
y0, y1 = rows[rank]
g = limg_amd.LimgHip(rank)
g.comm_init_from_torch(dist)
torch.cuda.synchronize()
dist.barrier()
print("LIMG_COMM_UP rank %d" % rank, flush=True)   # rendezvous and communicator are done: a hang from here on is a failure of the code under test, not of the node
strip = torch.from_numpy(img[y0:y1].view(np.int32)).cuda()
planes = g.alloc_planes_device(W, y1 - y0)
g.encode3d_single_chain_device(strip, True, planes, (y0 // 8) * (W // 8))
torch.cuda.synchronize()
for k in PLANES:
    got = planes[k].cpu().numpy()
    got = got.view(np.uint32) if got.dtype == np.int32 else got
    assert np.array_equal(got, want[k][y0:y1]), (rank, k)
# the compact streams of the strips, gathered on rank 0 over RCCL and decoded there
st, n = g.encode_stream_device(strip, True)
out = torch.zeros(sum(g.stream_bound(W, b - a) + 16 for a, b in rows), dtype=torch.uint8, device="cuda") if rank == 0 else None
res = g.gather_stream(st, n, root=0, out=out)
torch.cuda.synchronize()
if rank == 0:
    buf, offs = res
    for r, (a, b) in enumerate(rows):
        o0 = int(offs[r]); nb = int(offs[r + 1]) - o0
        dec = g.decode_stream_device(buf[o0:o0 + nb], nb, W, b - a)
        torch.cuda.synchronize()
        # strip-restart streams: each strip's chain starts at the seed, so compare with the strip's own encode
        assert np.array_equal(dec.cpu().numpy().view(np.uint32), orc.encode3d(img[a:b], True)["pDecoded"]), r
# an undersized buffer on the root: EVERY rank must return OutOfBounds (no rank may be left with an unmatched send)
small = torch.zeros(64, dtype=torch.uint8, device="cuda") if rank == 0 else None
try:
    g.gather_stream(st, n, root=0, out=small)
    raise SystemExit("rank %d: undersized gather was accepted" % rank)
except limg_amd.LimgHipError as e:
    assert "103" in str(e), str(e)
torch.cuda.synchronize()
dist.barrier()
# abort rule: rank 1's E step "fails" (test hook).  It must still join the all-gather (rank 0 would wait in it forever otherwise) and return its error;
# rank 0's call returns, writes no plane and its context reports the aborted chain.
for v in planes.values():
    v.zero_()
if rank == 1:
    g.set_options(test_fail_chain_phase1=True)
try:
    g.encode3d_single_chain_device(strip, True, planes, (y0 // 8) * (W // 8))
    failed = False
except limg_amd.LimgHipError:
    failed = True
torch.cuda.synchronize()
assert failed == (rank == 1), (rank, failed)
assert all(int(v.count_nonzero().item()) == 0 for v in planes.values()), rank
try:
    g.check()
    reported = False
except limg_amd.LimgHipError:
    reported = True
assert reported, rank
g.set_options()
dist.barrier()
g.comm_destroy(); g.check(); g.close()
dist.destroy_process_group()
print("rank %d ok" % rank)
"""


def test_rccl_two_ranks(tmp_path):
    """RCCL with MORE than one rank (needs two GPUs: skipped on the one-GPU boxes this repo is developed on, so this path stays unmeasured until a multi-GPU node
    runs the suite): the single dither chain through two strips against the one-chain oracle, the stream gather + decode on rank 0, and an undersized gather
    buffer refused by both ranks."""
    import os
    import socket
    import subprocess
    import sys
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "rank.py"
    script.write_text(RANK_SCRIPT)
    sock = socket.socket(); sock.bind(("127.0.0.1", 0)); port = sock.getsockname()[1]; sock.close()
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), LIMG_ROOT=root, LIMG_HIP_LIB="test",  # (the abort-rule leg needs the test build's fail_chain_phase1 hook)
                   HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        procs.append(subprocess.Popen([sys.executable, str(script)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = []
    timed_out = False
    for pr in procs:
        try:
            outs.append(pr.communicate(timeout=240)[0])
        except subprocess.TimeoutExpired:
            timed_out = True
            pr.kill()
            outs.append(pr.communicate()[0])
    # Only a job that never got its communicator up may skip (rendezvous / fabric problem of the node).  Once both ranks have printed LIMG_COMM_UP a timeout is a
    # hang of the code under test -- a deadlock is the likeliest failure of new collective code -- and fails the suite.
    up = sum("LIMG_COMM_UP" in o for o in outs)
    if timed_out and up < 2 and not any("AssertionError" in o or "SystemExit" in o for o in outs):
        pytest.skip("the two-rank RCCL job did not get its communicator up in 240 s on this node (rendezvous / fabric problem, not a result): " + " | ".join(o[-300:] for o in outs))
    assert not timed_out, ("two-rank RCCL job hung AFTER the communicator was up", [o[-600:] for o in outs])
    assert all(p.returncode == 0 for p in procs), outs


L.product_twins(globals())  # test_x_product: the same tests on the product library (tests/lib_axis.py)
