"""FAST float mode (limg_hip_options.float_mode = 1; north_star: "within a stated PSNR tolerance on the float factor stage").  Its contract, from
SURVEY.md 8(c):
  Stage F (a4-a8)  : int16 extrema within +-2 LSB of the EXACT mode's on >= 99.9 % of blocks; end-to-end perceptual PSNR within 0.10 dB of EXACT.
                     One stated exception, measured not assumed: the THIRD direction of 4-channel synthetic gradients.  With opaque alpha a gradient block spans
                     two colour directions, so pass 3 fits a direction to the rounding residue of passes 1-2; any change of the arithmetic moves it -- the
                     reference's own -ffast-math build differs from its strict build there on 0.3 % of the blocks by up to 21 LSB (profiles/archive/r02_fast_float.md) at
                     identical PSNR.  For those images the C extrema get >= 95 % of blocks instead of 99.9 % (measured: 96.2 %); A and B keep 99.9 % everywhere;
  Stage I (a9-a16) : bit-exact GIVEN the records and factor bytes the float stage produced -- checked here by feeding the GPU's own FAST-mode records and
                     pre-dither factor bytes to the oracle's integer stage (search, dither chain, plane packing, decode) block by block.
  Both float stages: k_fit_tpb (one lane per block) and the E step's lane == pixel stage do the same operations in FAST mode too, so they give the same bits.
EXACT stays the default and the headline; this file is the whole of FAST's parity claim.  Its references are the same build's EXACT mode (pinned bit for bit to the
oracle and the reference by the rest of the suite) and the oracle's integer stage.

Fixture modes (every test runs in each; `set_options` keeps the mode unless a test names the option itself):
  fused        k_fit_tpb + k_encode_persistent<PREFIT> on images of whole blocks; height-ragged images: the rows above the last through those, the last block row
               through the split kernels (encode_height_ragged: both float stages in one image)
  split        force_split: k_fit_tpb + k_fit_search<PREFIT>, scan, k_dither_store
  legacy       legacy_float_stage: the persistent kernel's own lane == pixel float stage (k_encode_persistent<PREFIT = false>)
  split_legacy both: k_fit_search<PREFIT = false>
Images with partial edge blocks take k_fit_search<PREFIT = false> (lane == pixel) in every mode but the height-ragged case of `fused`.

What each test reaches, FAST instances only:
  test_float_stage_tolerance          EXACT vs FAST, fast search, whole blocks: every mode's default kernels, CH 3 and 4
  test_float_stage_tolerance_more     EXACT vs FAST on the accurate search (ACC = true: k_encode_persistent / k_fit_search, PREFIT true and false by mode) and on
                                      ragged images of >= 8 000 blocks (lane == pixel; `fused` 1024 x 618: both stages), partial blocks counted
  test_float_stages_identical_whole_blocks
                                      lane == pixel (legacy_float_stage) vs k_fit_tpb, both in the mode's split setting: pn / rg / rga, alpha on and off, fast and
                                      accurate search; records, shift words and all 11 planes
  test_float_stages_identical_at_size the same at 16384^2 RGB and 8192^2 RGBA, compared on the device
  test_float_stages_identical_unaligned_input
                                      a 4-byte-aligned input: k_fit_tpb<DIRECT = false> (fused, split) or the dword staging of the E step (legacy modes) vs the
                                      aligned k_fit_tpb<DIRECT = true> encode
  test_float_stages_identical_height_ragged
                                      the mode's path (whole-image ragged hook in `fused`) vs the default fused path (encode_height_ragged)
  test_float_stages_identical_width_ragged
                                      records of every whole-block column vs the image cropped to whole blocks through k_fit_tpb
  test_integer_stage_exact_given_fast_records(_more)
                                      block-by-block replay through the oracle's integer stage: whole and ragged shapes (a corner block of < 4 pixels), alpha on and
                                      off, accurate search, errorFactor 0 / 25 / 400, strip partitions (pool 1 / 2), PCG dither
  test_batch_entry / test_host_entry / test_compact_outputs / test_stream_entry
                                      the list, host-pointer (banded at 4096 x 2048), compact and stream entries against FAST single device encodes
  test_blocked_encoder_stays_exact    the merged-block encoder ignores float_mode: the oracle's (EXACT) planes with it set
  test_fast_mode_at_bench_size        8192^2 photo-noise: PSNR and shift words against EXACT"""
import numpy as np
import pytest

import lib_axis as L
from oracle.bind import PLANES, REC_DTYPE, BLOCKED_WRITTEN

pytestmark = pytest.mark.gpu

REC_I16 = ("dirA_min", "dirA_max", "dirB_offset", "dirB_mag", "dirC_offset", "dirC_mag")
TOL_LSB = 2          # extrema tolerance (int16 LSB)
TOL_BLOCK_FRAC = 1e-3  # blocks allowed outside it
TOL_PSNR_DB = 0.10
SEED = 0xCA7F00D15BADF00D  # every dither chain starts here (src/limg.cpp:1893)


def _gpu(mode, lib):
    g = L.open_context(lib)
    g.mode = mode
    plain = g.set_options

    def set_options(**kw):  # every options change inside a test keeps the fixture's mode, unless the test names the option itself
        kw.setdefault("force_split", mode in ("split", "split_legacy"))
        kw.setdefault("legacy_float_stage", mode in ("legacy", "split_legacy"))
        plain(**kw)
    g.set_options = set_options
    g.set_options()
    yield g
    g.set_options()
    g.check()
    g.close()


@pytest.fixture(scope="module", params=["fused", "split", "legacy", "split_legacy"])
def gpu(request):
    yield from _gpu(request.param, "test")


@pytest.fixture(scope="module", params=["fused", "split", "legacy", "split_legacy"])
def gpu_product(request):
    yield from _gpu(request.param, "product")


def _gen(oracle, kind, w, h, seed):
    return {"pn": lambda: oracle.photo_noise(w, h, seed), "rg": lambda: oracle.random_gradient(w, h, seed, True), "rga": lambda: oracle.random_gradient(w, h, seed, False)}[kind]()


def _dev(img):
    import torch
    return torch.from_numpy(np.ascontiguousarray(img).view(np.int32)).cuda()


def _encode(gpu, d_img, alpha, fast_float, forced=None, error_factor=100, fast=True, pool_threads=0, compact=False, **opts):
    """One device encode; opts go to set_options (the fixture's mode unless named).  -> numpy planes + records (by, bx) + shift words (by, bx)"""
    import torch
    h, w = d_img.shape
    gpu.set_options(float_fast=fast_float, forced_shift=forced, **opts)
    planes = gpu.alloc_planes_device(w, h)
    if compact:  # only the factor planes: the compact mode of limg_hip_encode3d_device
        planes = {k: v for k, v in planes.items() if k.startswith("pFactors")}
    by, bx = (h + 7) // 8, (w + 7) // 8
    rec = torch.zeros((by * bx, 16), dtype=torch.int32, device="cuda")
    sh = torch.zeros(by * bx, dtype=torch.int32, device="cuda")
    try:
        gpu.encode3d_device(d_img, alpha, planes, records=rec, shifts=sh, error_factor=error_factor, fast=fast, pool_threads=pool_threads)
        torch.cuda.synchronize()
    finally:
        gpu.set_options()
    out = {k: v.cpu().numpy().view(np.uint32 if v.dtype == torch.int32 else np.uint8) for k, v in planes.items()}
    out["records"] = rec.cpu().numpy().view(REC_DTYPE).reshape(by, bx)
    out["shifts"] = sh.cpu().numpy().astype(np.uint32).reshape(by, bx)
    return out


def _assert_same(got, want, ctx, keys=PLANES + ("records", "shifts")):
    bad = []
    for k in keys:
        if k == "records":
            bad += [(k, f, int((got[k][f] != want[k][f]).sum())) for f in REC_DTYPE.names if not np.array_equal(got[k][f], want[k][f])]
        elif not np.array_equal(got[k], want[k]):
            bad.append((k, int((got[k] != want[k]).sum())))
    assert not bad, (ctx, bad)


def _check_tolerance(gpu, img, exact, fast, alpha, residue_fit_c, ctx):
    """FAST against EXACT: extrema within TOL_LSB on all but TOL_BLOCK_FRAC of the blocks (partial blocks included), PSNR within TOL_PSNR_DB."""
    nblocks = exact["records"].size
    for group, fields in (("AB", REC_I16[:4]), ("C", REC_I16[4:])):
        off = np.zeros(exact["records"].shape, dtype=bool)
        worst = 0
        for f in fields:
            d = np.abs(exact["records"][f].astype(np.int32) - fast["records"][f].astype(np.int32)).max(axis=-1)
            off |= d > TOL_LSB
            worst = max(worst, int(d.max()))
        allowed = 0.05 if (group == "C" and residue_fit_c) else TOL_BLOCK_FRAC
        assert off.sum() / nblocks <= allowed, (ctx, group, "blocks beyond +-%d LSB: %d of %d (worst %d)" % (TOL_LSB, off.sum(), nblocks, worst))
    p_exact = gpu.compare(img, exact["pDecoded"], alpha)[0]
    p_fast = gpu.compare(img, fast["pDecoded"], alpha)[0]
    assert abs(p_exact - p_fast) <= TOL_PSNR_DB, (ctx, p_exact, p_fast)


@pytest.mark.parametrize("kind,alpha,size", [("pn", True, 1024), ("rg", True, 1024), ("pn", False, 1024), ("rga", True, 512)])
def test_float_stage_tolerance(gpu, oracle, kind, alpha, size):
    img = _gen(oracle, kind, size, size, 1)
    d_img = _dev(img)
    exact = _encode(gpu, d_img, alpha, False)
    fast = _encode(gpu, d_img, alpha, True)
    want = oracle.encode3d(img, alpha)
    for k in PLANES:  # EXACT is untouched by the new template parameter
        assert np.array_equal(exact[k], want[k]), k
    _check_tolerance(gpu, img, exact, fast, alpha, alpha and kind in ("rg", "rga"), (kind, alpha))  # see the module docstring for the C exception


# the accurate search under FAST (ACC = true), and ragged images whose 8 320 / 9 984 blocks make 0.1 % a count of 8 / 9
@pytest.mark.parametrize("kind,alpha,w,h,fast", [("pn", True, 1024, 1024, False), ("rg", True, 1024, 1024, False), ("pn", False, 1024, 1024, False),
                                                 ("pn", True, 1022, 517, True), ("pn", False, 1022, 517, True), ("rg", True, 1024, 618, True), ("pn", False, 1024, 618, True)])
def test_float_stage_tolerance_more(gpu, oracle, kind, alpha, w, h, fast):
    img = _gen(oracle, kind, w, h, 2)
    d_img = _dev(img)
    exact = _encode(gpu, d_img, alpha, False, fast=fast)
    got = _encode(gpu, d_img, alpha, True, fast=fast)
    _check_tolerance(gpu, img, exact, got, alpha, alpha and kind in ("rg", "rga"), (kind, alpha, w, h, fast))


@pytest.mark.parametrize("kind", ["pn", "rg", "rga"])
@pytest.mark.parametrize("alpha", [True, False])
@pytest.mark.parametrize("fast", [True, False])
def test_float_stages_identical_whole_blocks(gpu, oracle, kind, alpha, fast):
    """limg_hip_options.legacy_float_stage: "same bits either way" holds in FAST mode too -- the E step's lane == pixel float stage against k_fit_tpb.  A slip of
    one ulp in the float stage reaches the int16 records only where a value sits next to a rounding boundary, so the images are large (32 768 blocks)."""
    img = _gen(oracle, kind, 2048, 1024, 7)
    d_img = _dev(img)
    tpb = _encode(gpu, d_img, alpha, True, fast=fast, legacy_float_stage=False)
    lane = _encode(gpu, d_img, alpha, True, fast=fast, legacy_float_stage=True)
    _assert_same(lane, tpb, (kind, alpha, fast))


@pytest.mark.parametrize("alpha,W", [(False, 16384), (True, 8192)])
def test_float_stages_identical_at_size(gpu, alpha, W):
    """The same at full size, compared on the device: a one-ulp slip in the 3-channel third direction moves a C record value of a few LSB by about 1e-6, so it
    shows on one value in about a million -- here 1.6 M (16384^2, RGB) and 0.4 M (8192^2, RGBA) blocks."""
    import torch
    d_img = gpu.synth_device("photo_noise", W, W, seed=5)
    out = {}
    for legacy in (False, True):
        gpu.set_options(float_fast=True, legacy_float_stage=legacy)
        planes = gpu.alloc_planes_device(W, W)
        rec = torch.empty(((W // 8) ** 2, 16), dtype=torch.int32, device="cuda")
        sh = torch.empty((W // 8) ** 2, dtype=torch.int32, device="cuda")
        try:
            gpu.encode3d_device(d_img, alpha, planes, records=rec, shifts=sh, pool_threads=2)
            torch.cuda.synchronize()
        finally:
            gpu.set_options()
        out[legacy] = (planes, rec, sh)
    gpu.check()
    (pa, ra, sa), (pb, rb, sb) = out[False], out[True]
    assert torch.equal(ra, rb), ("records", int((ra != rb).any(dim=1).sum()))
    assert torch.equal(sa, sb), ("shifts", int((sa != sb).sum()))
    for k in PLANES:
        assert torch.equal(pa[k], pb[k]), k
    del out, pa, pb, ra, rb, sa, sb, d_img
    torch.cuda.empty_cache()


@pytest.mark.parametrize("alpha", [True, False])
def test_float_stages_identical_unaligned_input(gpu, oracle, alpha):
    """An input pointer that is only 4-byte aligned (a slice of a larger allocation, as in test_gpu_parity.test_unaligned_device_pointers) takes k_fit_tpb's
    dword-input variant (DIRECT = false) or the E step's dword staging: the same bits as the aligned input through k_fit_tpb<DIRECT = true>."""
    import torch
    W, H = 2048, 512
    img = oracle.random_gradient(W, H, 77, False) if alpha else oracle.photo_noise(W, H, 77)
    buf = torch.zeros(W * H + 8, dtype=torch.int32, device="cuda")
    d_img = buf[1:1 + W * H].view(H, W)
    d_img.copy_(torch.from_numpy(img.view(np.int32)))
    assert d_img.data_ptr() % 16 == 4
    got = _encode(gpu, d_img, alpha, True)
    want = _encode(gpu, _dev(img), alpha, True, legacy_float_stage=False)
    _assert_same(got, want, ("unaligned", alpha))


@pytest.mark.parametrize("w,h", [(8, 9), (512, 100), (1024, 301), (40, 1001), (2048, 1021)])
@pytest.mark.parametrize("alpha", [True, False])
def test_float_stages_identical_height_ragged(gpu, oracle, w, h, alpha):
    """Width in whole blocks, last block row partial.  The default fused path runs the rows above through k_fit_tpb and the last row through the lane == pixel stage
    (encode_height_ragged); the whole-image ragged path (test hook in `fused`; the other modes take it anyway) runs every block through the lane == pixel stage."""
    img = oracle.photo_noise(w, h, 31) if w != 512 else oracle.random_gradient(w, h, 31, True)
    d_img = _dev(img)
    want = _encode(gpu, d_img, alpha, True, force_split=False, legacy_float_stage=False)
    if L.has_hooks(gpu):
        got = _encode(gpu, d_img, alpha, True, test_whole_image_ragged=True)
    elif gpu.mode == "fused":  # no whole-image ragged hook on the product: its fused leg is `want` itself, so the lane == pixel stage comes from the split path
        got = _encode(gpu, d_img, alpha, True, force_split=True)
    else:
        got = _encode(gpu, d_img, alpha, True)
    _assert_same(got, want, (w, h, alpha))


@pytest.mark.parametrize("w,h,alpha", [(203, 61, True), (509, 515, False), (1022, 517, True), (2046, 1029, False), (2045, 1027, True)])
def test_float_stages_identical_width_ragged(gpu, oracle, w, h, alpha):
    """A partial last block column puts every block on the lane == pixel stage.  A block's record depends on its own pixels only (the under-4-pixel corner quirk
    touches partial blocks alone), so the whole-block columns must carry the records of the image cropped to whole blocks, encoded through k_fit_tpb."""
    img = oracle.photo_noise(w, h, 41) if alpha else oracle.random_gradient(w, h, 41, True)
    wc = w // 8 * 8
    got = _encode(gpu, _dev(img), alpha, True)
    want = _encode(gpu, _dev(img[:, :wc]), alpha, True, force_split=False, legacy_float_stage=False)
    for f in REC_DTYPE.names:
        assert np.array_equal(got["records"][:, :wc // 8][f], want["records"][f]), (w, h, alpha, f)


def _chain_starts(h, pool):
    """Block rows at which a dither chain starts, the oracle's strip partition (oracle/limg_oracle.c limg_oracle_encode3d, src/limg.cpp:2114-2134): without a pool
    one chain; otherwise 4 * pool strips of (block rows / (4 * pool)) block rows -- or pool strips if that is 0 -- the last strip taking the remainder; if even
    pool strips get no whole block row, all but the last strip are empty and one chain covers the image."""
    if pool <= 0:
        return {0}
    count = pool * 4
    rows = (h // 8) // count
    if rows == 0:
        count = pool
        rows = (h // 8) // count
    if rows == 0:
        return {0}
    return {i * rows for i in range(count)}


def _replay(gpu, oracle, img, alpha, ef=100, fast=True, pool=0, pcg=False):
    """Records and pre-dither factor bytes from the GPU's FAST float stage (forced shift 0 => the factor planes hold the raw factor bytes) go through the
    ORACLE's integer stage, block by block (rx x ry pixels) in raster order, the dither chain restarting at every strip: its search must pick the GPU's shifts
    and its dither chain + decode must reproduce the GPU's factor planes and pDecoded."""
    from oracle.bind import DITHER_AES, DITHER_PCG
    h, w = img.shape
    assert ((w + 7) // 8) * ((h + 7) // 8) <= 2000
    ch = 4 if alpha else 3
    mode = DITHER_PCG if pcg else DITHER_AES
    d_img = _dev(img)
    kw = dict(error_factor=ef, fast=fast, pool_threads=pool, dither_pcg=pcg)
    raw = _encode(gpu, d_img, alpha, True, forced=(0, 0, 0), **kw)
    got = _encode(gpu, d_img, alpha, True, **kw)
    for f in REC_DTYPE.names:
        assert np.array_equal(raw["records"][f], got["records"][f]), f  # the float stage does not depend on the shifts
    starts = _chain_starts(h, pool)
    chain = SEED
    for by in range((h + 7) // 8):
        if by in starts:
            chain = SEED
        for bx in range((w + 7) // 8):
            ry, rx = min(8, h - by * 8), min(8, w - bx * 8)
            sl = (slice(by * 8, by * 8 + ry), slice(bx * 8, bx * 8 + rx))
            px = np.ascontiguousarray(img[sl]).ravel()
            rec = np.ascontiguousarray(got["records"][by, bx:bx + 1])
            fa, fb, fc = (np.ascontiguousarray(raw[k][sl]).ravel() for k in ("pFactorsA", "pFactorsB", "pFactorsC"))
            shift, _ = oracle.block_search(px, ch, rec, fa, fb, fc, ef, fast)
            sw = int(got["shifts"][by, bx])
            assert [int(s) for s in shift] == [sw & 0xFF, (sw >> 8) & 0xFF, (sw >> 16) & 0xFF], (by, bx)
            fs = []
            for s, f in zip(shift, (fa, fb, fc)):
                if int(s) not in (0, 8):
                    chain, f = oracle.dither(int(s), chain, f, mode)
                fs.append(f)
            dec = oracle.block_decode(rx, ry, ch, rec, fs[0], fs[1], fs[2], shift)
            assert np.array_equal(dec, got["pDecoded"][sl]), (by, bx)
            for k, f, s in zip(("pFactorsA", "pFactorsB", "pFactorsC"), fs, shift):
                assert np.array_equal(((f.astype(np.uint32) << int(s)) & 0xFF).astype(np.uint8).reshape(ry, rx), got[k][sl]), (by, bx, k)


@pytest.mark.parametrize("kind,alpha", [("pn", True), ("rg", True), ("pn", False)])
def test_integer_stage_exact_given_fast_records(gpu, oracle, kind, alpha):
    """_replay on 256 x 32 (whole blocks, one chain, fast search, errorFactor 100)."""
    _replay(gpu, oracle, _gen(oracle, kind, 256, 32, 9), alpha)


# (kind, w, h, alpha, errorFactor, fast search, pool threads, PCG dither); 3 x 1 is a corner block of fewer than 4 pixels
REPLAY = [("pn", 61, 27, True, 100, True, 0, False), ("rga", 203, 61, True, 100, True, 0, False), ("pn", 203, 61, False, 100, True, 0, False),
          ("pn", 17, 10, False, 100, True, 0, False), ("rg", 9, 9, True, 100, True, 0, False), ("pn", 265, 9, True, 100, True, 0, False),
          ("pn", 3, 1, True, 100, True, 0, False), ("pn", 3, 1, False, 100, True, 0, False),
          ("pn", 203, 61, True, 100, False, 0, False), ("rg", 61, 27, False, 100, False, 0, False), ("pn", 256, 32, True, 100, False, 0, False),
          ("pn", 61, 27, True, 0, True, 0, False), ("pn", 203, 61, True, 25, True, 0, False), ("rga", 203, 61, False, 400, True, 0, False),
          ("pn", 203, 61, True, 100, True, 1, False), ("pn", 256, 64, True, 100, True, 2, False), ("pn", 61, 27, False, 100, True, 2, False),
          ("pn", 61, 27, True, 100, True, 0, True)]


@pytest.mark.parametrize("kind,w,h,alpha,ef,fast,pool,pcg", REPLAY)
def test_integer_stage_exact_given_fast_records_more(gpu, oracle, kind, w, h, alpha, ef, fast, pool, pcg):
    """_replay on ragged shapes, the accurate search, other error factors, strip partitions and the PCG dither."""
    _replay(gpu, oracle, _gen(oracle, kind, w, h, 9), alpha, ef, fast, pool, pcg)


@pytest.mark.parametrize("alpha,fast,sub,n", [(True, True, 0, 5), (False, True, 0, 5), (True, False, 0, 5), (True, True, 1, 5), (False, True, 3, 5), (True, True, 0, 17)])
def test_batch_entry(gpu, oracle, alpha, fast, sub, n):
    """limg_hip_encode3d_batch_device in FAST mode: every image gets the planes of its own FAST single encode -- one launch pair, sub-batch pipelines of 1 / 3 images,
    and 17 images (the default pipelining rule: sub-batches of 4)."""
    import torch
    W, H = 512, 72
    host = [oracle.photo_noise(W, H, 40 + i) if i % 2 == 0 else oracle.random_gradient(W, H, 40 + i, i % 4 != 3) for i in range(n)]
    imgs = [_dev(h) for h in host]
    outs = [gpu.alloc_planes_device(W, H) for _ in imgs]
    gpu.set_options(float_fast=True, batch_sub_images=sub)
    try:
        gpu.encode3d_batch_device(imgs, alpha, outs, fast=fast)
        torch.cuda.synchronize()
    finally:
        gpu.set_options()
    gpu.check()
    for i, (d_img, pl) in enumerate(zip(imgs, outs)):
        want = _encode(gpu, d_img, alpha, True, fast=fast)
        got = {k: v.cpu().numpy().view(np.uint32 if v.dtype == torch.int32 else np.uint8) for k, v in pl.items()}
        _assert_same(got, want, (i, alpha, fast, sub, n), keys=PLANES)


@pytest.mark.parametrize("w,h,pool", [(203, 61, 0), (4096, 2048, 2)])
def test_host_entry(gpu, oracle, w, h, pool):
    """limg_hip_encode3d (host pointers; from 4 Mpixels on in row bands, a band per restarted chain with a pool) in FAST mode == the FAST device entry."""
    import torch
    d_img = gpu.synth_device("photo_noise", w, h, seed=9)
    img = d_img.cpu().numpy().view(np.uint32)
    gpu.set_options(float_fast=True)
    try:
        got = gpu.encode3d(img, True, pool_threads=pool)
    finally:
        gpu.set_options()
    want = _encode(gpu, d_img, True, True, pool_threads=pool)
    _assert_same(got, want, (w, h, pool), keys=PLANES)
    del d_img
    torch.cuda.empty_cache()


@pytest.mark.parametrize("w,h,alpha", [(512, 64, True), (256, 61, False), (203, 61, True)])
def test_compact_outputs(gpu, oracle, w, h, alpha):
    """Compact mode (factor planes + records + shift words, no uint32 planes) in FAST mode: the same values as the full run."""
    img = oracle.photo_noise(w, h, 61)
    d_img = _dev(img)
    full = _encode(gpu, d_img, alpha, True)
    got = _encode(gpu, d_img, alpha, True, compact=True)
    _assert_same(got, full, (w, h, alpha), keys=("pFactorsA", "pFactorsB", "pFactorsC", "records", "shifts"))


def test_stream_entry(gpu, oracle):
    """limg_hip_encode_stream in FAST mode: the bytes oracle/stream.py packs from the FAST run's records, shift words and factor planes (the forced-0 run's raw
    factor bytes for the raw escapes), and decode(stream) == the FAST pDecoded.  Whole-block, height-ragged and width-ragged shapes."""
    from oracle import stream as S
    saw_escape = False
    for kind, w, h, alpha in (("pn", 256, 64, True), ("rga", 256, 64, True), ("pn", 256, 61, True), ("rga", 203, 61, True), ("pn", 131, 77, False)):
        img = _gen(oracle, kind, w, h, 3)
        d_img = _dev(img)
        got = _encode(gpu, d_img, alpha, True)
        raw = _encode(gpu, d_img, alpha, True, forced=(0, 0, 0))
        sh = got["shifts"]
        enc = dict(records=got["records"], shifts=np.stack([sh & 0xFF, (sh >> 8) & 0xFF, (sh >> 16) & 0xFF], axis=-1).astype(np.uint8),
                   pFactorsA=got["pFactorsA"], pFactorsB=got["pFactorsB"], pFactorsC=got["pFactorsC"], preA=raw["pFactorsA"], preB=raw["pFactorsB"], preC=raw["pFactorsC"])
        want = S.pack(enc, w, h, 4 if alpha else 3)
        gpu.set_options(float_fast=True)
        try:
            st = gpu.encode_stream(img, alpha)
        finally:
            gpu.set_options()
        assert st.size == want.size and np.array_equal(st, want), (kind, w, h, alpha, st.size, want.size)
        saw_escape |= bool((S.parse(st)[1]["shift"] >> 24).any())
        assert np.array_equal(gpu.decode_stream(st), got["pDecoded"]), (kind, w, h, alpha)
    assert saw_escape


def test_blocked_encoder_stays_exact(gpu, oracle):
    """"The merged-block encoder always runs EXACT": with float_mode = 1 set, its planes are still the oracle's."""
    for kind, alpha, (w, h) in (("pn", True, (256, 128)), ("rga", True, (203, 61)), ("pn", False, (131, 77)), ("rg", True, (265, 9))):
        img = _gen(oracle, kind, w, h, 5)
        want = oracle.blocked_encode3d(img, alpha)
        gpu.set_options(float_fast=True)
        try:
            got = gpu.blocked_encode3d(img, alpha)
        finally:
            gpu.set_options()
        bad = [(k, int((got[k] != want[k]).sum())) for k in BLOCKED_WRITTEN if not np.array_equal(got[k], want[k])]
        assert not bad, (kind, alpha, w, h, bad)


def test_fast_mode_at_bench_size(gpu):
    """8192^2 photo-noise (the bench workload): PSNR of FAST within 0.10 dB of EXACT, shifts identical on >= 99 % of blocks."""
    import torch
    W = 8192
    d_img = gpu.synth_device("photo_noise", W, W, seed=1)
    res = {}
    for ff in (False, True):
        gpu.set_options(float_fast=ff)
        planes = gpu.alloc_planes_device(W, W)
        sh = torch.zeros((W // 8) ** 2, dtype=torch.int32, device="cuda")
        gpu.encode3d_device(d_img, True, planes, shifts=sh)
        torch.cuda.synchronize()
        res[ff] = (gpu.compare_device(d_img, planes["pDecoded"], True)[0], sh & 0xFFFFFF)
        del planes
    assert abs(res[False][0] - res[True][0]) <= TOL_PSNR_DB, (res[False][0], res[True][0])
    same = float((res[False][1] == res[True][1]).float().mean())
    assert same >= 0.99, same
    gpu.set_options()
    torch.cuda.empty_cache()


L.product_twins(globals())  # test_x_product: the same tests on the product library (tests/lib_axis.py)
