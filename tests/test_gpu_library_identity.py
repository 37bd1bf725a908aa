"""The product library (limg_amd/liblimg_hip.so) against the test build (liblimg_hip_test.so) BIT FOR BIT, in one process, on the same device inputs.  Every kernel that
takes EncodeParams is a separate code object in each (tests/test_product_library.py test_kernel_inventory_of_the_two_builds), so the product's instantiations are run here
over the matrix they come in: 3 / 4 channels, fast / accurate search, the four fixture modes of tests/test_gpu_fast_float.py (fused, split, legacy, split_legacy),
EXACT / FAST float mode, whole-block, height-ragged, width-ragged and corner-block shapes and a 4-byte-aligned input (k_fit_tpb<DIRECT = false>), strip partitions,
the PCG dither and collected statistics; the list entry as a sub-batch pipeline, the compact outputs, the stream bytes and the merged-block encoder.  Compared: records,
shift words and all 11 planes (or the blocked planes and rectangles, the stream bytes, the counters).

The oracle pins EXACT on both libraries elsewhere; FAST has only tolerances against EXACT, so a product that drifted by one ulp in FAST mode would pass them -- only this
comparison sees it.  A one-ulp slip reaches an int16 record only next to a rounding boundary, so FAST also runs at 16384^2 RGB and 8192^2 RGBA (4.2 M and 1 M blocks)."""
import numpy as np
import pytest

import lib_axis as L
from oracle.bind import PLANES

pytestmark = pytest.mark.gpu

MODES = {"fused": dict(force_split=False, legacy_float_stage=False), "split": dict(force_split=True, legacy_float_stage=False),
         "legacy": dict(force_split=False, legacy_float_stage=True), "split_legacy": dict(force_split=True, legacy_float_stage=True)}
# (width, height) per shape: whole blocks (1024 work strips: the look-back), last block row partial, last block column partial, a corner block of 3 pixels
SHAPES = {"whole": (2048, 1024), "height_ragged": (1024, 301), "width_ragged": (509, 515), "corner": (3, 1)}


@pytest.fixture(scope="module")
def libs():
    ctx = {lib: L.open_context(lib) for lib in L.LIBS}
    yield ctx
    for g in ctx.values():
        g.set_options()
        g.check()
        g.close()


def _image(g, w, h, alpha, seed, unaligned=False):
    """photo-noise (RGBA) or an opaque gradient (RGB), made on the device; unaligned: a view that starts 4 bytes into an allocation"""
    import torch
    img = g.synth_device("photo_noise" if alpha else "random_gradient", w, h, seed=seed)
    if not unaligned:
        return img
    buf = torch.zeros(w * h + 8, dtype=torch.int32, device="cuda")
    view = buf[1:1 + w * h].view(h, w)
    view.copy_(img)
    assert view.data_ptr() % 16 == 4
    return view


def _encode(g, img, alpha, opts, compact=False, **kw):
    """one device encode on context g -> {plane name / "records" / "shifts": device tensor}"""
    import torch
    h, w = img.shape
    g.set_options(**opts)
    try:
        planes = g.alloc_planes_device(w, h)
        if compact:
            planes = {k: v for k, v in planes.items() if k.startswith("pFactors")}
        for v in planes.values():
            v.fill_(0x5A)
        n = ((w + 7) // 8) * ((h + 7) // 8)
        rec = torch.full((n, 16), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        sh = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        g.encode3d_device(img, alpha, planes, records=rec, shifts=sh, **kw)
        torch.cuda.synchronize()
        out = dict(planes, records=rec, shifts=sh)
        if opts.get("collect_stats"):
            out["stats"] = g.last_stats()
    finally:
        g.set_options()
    g.check()
    return out


def _assert_identical(a, b, ctx):
    import torch
    bad = []
    for k in a:
        if k == "stats":
            if not (np.array_equal(a[k][0], b[k][0]) and a[k][1] == b[k][1]):
                bad.append(k)
        elif not torch.equal(a[k], b[k]):
            bad.append((k, int((a[k] != b[k]).sum())))
    assert not bad, ("product != test build", ctx, bad)


def _both(libs, fn):
    return fn(libs["product"]), fn(libs["test"])


@pytest.mark.parametrize("shape", sorted(SHAPES) + ["unaligned"])
@pytest.mark.parametrize("fast", [True, False], ids=["fast_search", "accurate_search"])
@pytest.mark.parametrize("alpha", [True, False], ids=["rgba", "rgb"])
@pytest.mark.parametrize("float_fast", [False, True], ids=["exact", "fast_float"])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_encode_matrix(libs, mode, float_fast, alpha, fast, shape):
    w, h = SHAPES.get(shape, (2048, 512))
    img = _image(libs["test"], w, h, alpha, seed=w + h, unaligned=(shape == "unaligned"))
    opts = dict(MODES[mode], float_fast=float_fast)
    p, t = _both(libs, lambda g: _encode(g, img, alpha, opts, fast=fast))
    _assert_identical(p, t, (mode, float_fast, alpha, fast, shape))


@pytest.mark.parametrize("pool,pcg,stats", [(2, False, False), (0, True, False), (0, False, True), (2, True, True)])
@pytest.mark.parametrize("shape", ["whole", "height_ragged", "width_ragged"])
@pytest.mark.parametrize("float_fast", [False, True], ids=["exact", "fast_float"])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_encode_options(libs, mode, float_fast, shape, pool, pcg, stats):
    """strip partitions (pool 2: chains restart every few block rows), the PCG dither and the device-reduced statistics"""
    w, h = SHAPES[shape]
    img = _image(libs["test"], w, h, True, seed=7)
    opts = dict(MODES[mode], float_fast=float_fast, dither_pcg=pcg, collect_stats=stats)
    p, t = _both(libs, lambda g: _encode(g, img, True, opts, pool_threads=pool, error_factor=25 if pool else 100))
    _assert_identical(p, t, (mode, float_fast, shape, pool, pcg, stats))


@pytest.mark.parametrize("shape", ["whole", "height_ragged", "width_ragged"])
@pytest.mark.parametrize("float_fast", [False, True], ids=["exact", "fast_float"])
@pytest.mark.parametrize("mode", ["fused", "split"])
def test_compact_outputs_and_stream(libs, mode, float_fast, shape):
    """compact mode (factor planes + records + shift words) and the stream entry's bytes"""
    w, h = SHAPES[shape]
    img = _image(libs["test"], w, h, True, seed=11)
    opts = dict(MODES[mode], float_fast=float_fast)
    p, t = _both(libs, lambda g: _encode(g, img, True, opts, compact=True))
    _assert_identical(p, t, (mode, float_fast, shape, "compact"))
    for alpha in (True, False):
        streams = []
        for g in (libs["product"], libs["test"]):
            g.set_options(**opts)
            try:
                st, n = g.encode_stream_device(img, alpha)
                streams.append(st[:n].cpu().numpy())
            finally:
                g.set_options()
        assert streams[0].size == streams[1].size and np.array_equal(streams[0], streams[1]), (mode, float_fast, shape, alpha, "stream bytes")


@pytest.mark.parametrize("sub", [0, 2, 3])
@pytest.mark.parametrize("float_fast", [False, True], ids=["exact", "fast_float"])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_batch_pipeline(libs, mode, float_fast, sub):
    """limg_hip_encode3d_batch_device: 7 images of 512 x 72 as one launch pair (sub 0: the library's rule) or a pipeline of sub-batches of 2 / 3"""
    import torch
    W, H, n = 512, 72, 7
    imgs = [_image(libs["test"], W, H, i % 2 == 0, seed=60 + i) for i in range(n)]
    outs = {}
    for lib, g in libs.items():
        outs[lib] = [g.alloc_planes_device(W, H) for _ in imgs]
        g.set_options(**MODES[mode], float_fast=float_fast, batch_sub_images=sub)
        try:
            g.encode3d_batch_device(imgs, True, outs[lib])
            torch.cuda.synchronize()
        finally:
            g.set_options()
        g.check()
    for i in range(n):
        _assert_identical(outs["product"][i], outs["test"][i], (mode, float_fast, sub, i))


@pytest.mark.parametrize("kind,w,h,alpha", [("pn", 2048, 1024, True), ("rg", 1024, 512, True), ("rga", 203, 61, True), ("pn", 509, 515, False)])
def test_blocked_encoder(libs, oracle, kind, w, h, alpha):
    """the merged-block encoder (pass 1 runs the EncodeParams fit kernels): its 13 planes and the rectangles, also with float_mode set (it stays EXACT)"""
    import torch
    img = oracle.photo_noise(w, h, 5) if kind == "pn" else oracle.random_gradient(w, h, 5, kind == "rg")
    d_img = torch.from_numpy(img.view(np.int32)).cuda()
    for ff in (False, True):
        outs, regions = {}, {}
        for lib, g in libs.items():
            g.set_options(float_fast=ff)
            try:
                outs[lib] = g.alloc_blocked_planes_device(w, h)
                g.blocked_encode3d_device(d_img, alpha, outs[lib])
                torch.cuda.synchronize()
                regions[lib] = g.blocked_regions()
            finally:
                g.set_options()
            g.check()
        _assert_identical(outs["product"], outs["test"], (kind, w, h, alpha, ff))
        assert np.array_equal(regions["product"], regions["test"]), (kind, w, h, alpha, ff, "regions")


@pytest.mark.parametrize("alpha,W,pool", [(False, 16384, 0), (True, 8192, 2)], ids=["rgb16384", "rgba8192_pool2"])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_fast_float_at_size(libs, mode, alpha, W, pool):
    """FAST float mode where a one-ulp slip shows: 16384^2 RGB (one chain through 32 K work strips) and 8192^2 RGBA (8 chains), photo-noise, every mode; records, shift
    words and all planes compared on the device"""
    import torch
    img = libs["test"].synth_device("photo_noise", W, W, seed=5)
    opts = dict(MODES[mode], float_fast=True)
    p = _encode(libs["product"], img, alpha, opts, pool_threads=pool)
    t = _encode(libs["test"], img, alpha, opts, pool_threads=pool)
    _assert_identical(p, t, (mode, alpha, W))
    assert set(p) == set(PLANES) | {"records", "shifts"}
    del p, t, img
    torch.cuda.empty_cache()
