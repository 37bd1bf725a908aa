"""The stream splice (include/limg_hip.h) from C99: a C program links against the library, encodes an image and two strips of it, crops the image's stream with
limg_hip_stream_crop and joins the strips' streams with limg_hip_stream_splice, and compares what the results decode to -- pixel for pixel -- with the window decode
of the source and the decodes of the strips; the refusals that come back before anything touches a device too.  A second program, C++, does the same through the
shim's limg_crop_stream and limg_splice_streams."""
import os
import subprocess

import pytest

import lib_axis as L
from lib_axis import lib, lib_product  # noqa: F401  (fixtures: "test" / "product")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# both programs: a 72 x 28 image (9 x 4 blocks, the last row 4 pixels high), its stream, the streams of its rows 0 .. 15 and 16 .. 27
COMMON = r'''
#define W 72u
#define H 28u
#define CUT 16u

static void fill(uint32_t *img)
{
  uint32_t seed = 4711u, k;
  for (k = 0; k < W * H; k++)
  {
    const uint32_t x = k % W, y = k / W;
    seed = seed * 1664525u + 1013904223u;
    img[k] = ((3u * x) & 0xFFu) | (((y * 7u + (seed >> 29)) & 0xFFu) << 8) | ((((x + y) >> 1) & 0xFFu) << 16) | (((180u + (seed >> 27)) & 0xFFu) << 24);
  }
}
'''

C_SOURCE = r'''
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "limg_hip.h"
''' + COMMON + r'''
int main(void)
{
  limg_hip_context *ctx = NULL;
  static uint32_t img[W * H], full[W * H], a[W * H], b[W * H], win[W * H];
  limg_hip_splice_piece pieces[2];
  const size_t bound = limg_hip_stream_bound(W, H);
  uint8_t *st = (uint8_t *)malloc(bound), *top = (uint8_t *)malloc(bound), *bottom = (uint8_t *)malloc(bound), *out = (uint8_t *)malloc(bound);
  size_t n = 0, nTop = 0, nBottom = 0, nOut = 0, k, gx = 0, gy = 0, total = 0;
  int alpha = 0;
  if (sizeof(limg_hip_splice_piece) != 48 || bound == 0 || !st || !top || !bottom || !out) return 1;
  fill(img);
  if (limg_hip_stream_crop(NULL, st, 64, 0, 0, 8, 8, out, bound, &nOut) != limg_hip_error_ArgumentNull) return 10;
  if (limg_hip_stream_splice(NULL, pieces, 2, sizeof(pieces[0]), W, H, 1, 100, 1, out, bound, &nOut) != limg_hip_error_ArgumentNull) return 11;
  if (limg_hip_init(-1, &ctx) != limg_hip_success) return 3;
  if (limg_hip_encode_stream(ctx, img, W, H, 1, st, bound, &n, 100, 0, 1) != limg_hip_success) return 4;
  if (limg_hip_encode_stream(ctx, img, W, CUT, 1, top, bound, &nTop, 100, 0, 1) != limg_hip_success) return 5;
  if (limg_hip_encode_stream(ctx, img + W * CUT, W, H - CUT, 1, bottom, bound, &nBottom, 100, 0, 1) != limg_hip_success) return 6;
  if (limg_hip_decode_stream(ctx, st, n, full, W * H) != limg_hip_success) return 7;

  /* crop: columns 8 .. 71, rows 8 .. 27 -- down to the partial last row */
  memset(out, 0xA5, bound);
  if (limg_hip_stream_crop(ctx, st, n, 4, 8, 64, 20, out, bound, &nOut) != limg_hip_error_InvalidParameter) return 20; /* an origin off the block grid */
  if (limg_hip_stream_crop(ctx, st, n, 8, 8, 60, 20, out, bound, &nOut) != limg_hip_error_InvalidParameter) return 21; /* an end neither on a block nor the edge */
  if (limg_hip_stream_crop(ctx, st, n, 8, 8, 64, 20, out, 100, &nOut) != limg_hip_error_OutOfBounds || nOut <= 100) return 22; /* the size is reported */
  for (k = 0; k < bound; k++)
    if (out[k] != 0xA5) return 23; /* a refused call writes nothing */
  if (limg_hip_stream_crop(ctx, st, n, 8, 8, 64, 20, out, bound, &nOut) != limg_hip_success) return 24;
  if (limg_hip_stream_info(out, nOut, &gx, &gy, &alpha, &total) != limg_hip_success || gx != 64 || gy != 20 || !alpha || total != nOut) return 25;
  for (k = nOut; k < bound; k++)
    if (out[k] != 0xA5) return 26;
  if (limg_hip_decode_stream(ctx, out, nOut, a, W * H) != limg_hip_success) return 27;
  if (limg_hip_decode_stream_window(ctx, st, n, 8, 8, 64, 20, win, 64) != limg_hip_success) return 28;
  if (memcmp(a, win, 64 * 20 * sizeof(uint32_t)) != 0) { puts("the crop decodes to other pixels than the window"); return 29; }

  /* join: the two strips' streams into the image's */
  pieces[0].pStream = top; pieces[0].streamBytes = nTop; pieces[0].srcSizeX = W; pieces[0].srcSizeY = CUT;
  pieces[0].srcBx = 0; pieces[0].srcBy = 0; pieces[0].dstBx = 0; pieces[0].dstBy = 0; pieces[0].blocksW = 9; pieces[0].blocksH = 2;
  pieces[1] = pieces[0];
  pieces[1].pStream = bottom; pieces[1].streamBytes = nBottom; pieces[1].srcSizeY = H - CUT; pieces[1].dstBy = 2;
  memset(out, 0xA5, bound);
  if (limg_hip_stream_splice(ctx, pieces, 2, sizeof(pieces[0]) - 1, W, H, 1, 100, 1, out, bound, &nOut) != limg_hip_error_InvalidParameter) return 30;
  if (limg_hip_stream_splice(ctx, pieces, 0, sizeof(pieces[0]), W, H, 1, 100, 1, out, bound, &nOut) != limg_hip_error_InvalidParameter) return 31;
  if (limg_hip_stream_splice(ctx, pieces, 1, sizeof(pieces[0]), W, H, 1, 100, 1, out, bound, &nOut) != limg_hip_error_InvalidParameter) return 32; /* a gap */
  pieces[1].dstBy = 1;
  if (limg_hip_stream_splice(ctx, pieces, 2, sizeof(pieces[0]), W, H, 1, 100, 1, out, bound, &nOut) != limg_hip_error_InvalidParameter) return 33; /* an overlap */
  pieces[1].dstBy = 2;
  if (limg_hip_stream_splice(ctx, pieces, 2, sizeof(pieces[0]), W, H + 4, 1, 100, 1, out, bound, &nOut) != limg_hip_error_InvalidParameter) return 34; /* the edge rule */
  for (k = 0; k < bound; k++)
    if (out[k] != 0xA5) return 35;
  if (limg_hip_stream_splice(ctx, pieces, 2, sizeof(pieces[0]), W, H, 1, 100, 1, out, bound, &nOut) != limg_hip_success) return 36;
  if (limg_hip_stream_info(out, nOut, &gx, &gy, &alpha, &total) != limg_hip_success || gx != W || gy != H || !alpha || total != nOut) return 37;
  if (nOut != nTop + nBottom - 64) return 38; /* one header less, every entry and payload word kept */
  if (limg_hip_decode_stream(ctx, out, nOut, a, W * H) != limg_hip_success) return 39;
  if (limg_hip_decode_stream(ctx, top, nTop, b, W * H) != limg_hip_success) return 40;
  if (limg_hip_decode_stream(ctx, bottom, nBottom, b + W * CUT, W * H - W * CUT) != limg_hip_success) return 41;
  if (memcmp(a, b, W * H * sizeof(uint32_t)) != 0) { puts("the joined stream decodes to other pixels than its strips"); return 42; }
  /* a source whose header contradicts itself is refused */
  bottom[8] ^= 0x10; /* sizeX */
  if (limg_hip_stream_splice(ctx, pieces, 2, sizeof(pieces[0]), W, H, 1, 100, 1, out, bound, &nOut) == limg_hip_success) return 43;
  bottom[8] ^= 0x10;
  if (limg_hip_check_device_status(ctx) != limg_hip_success) return 50;
  limg_hip_shutdown(&ctx);
  puts("stream crop and join ok");
  return 0;
}
'''

CPP_SOURCE = r'''
#include <stdio.h>
#include <string.h>
#include <vector>
#include "limg_hip_shim.hpp"
''' + COMMON + r'''
int main()
{
  std::vector<uint32_t> img(W * H), a(W * H), b(W * H);
  fill(img.data());
  const size_t bound = limg_encode_bound(W, H);
  std::vector<uint8_t> st(bound), top(bound), bottom(bound), out(bound);
  size_t n = 0, nTop = 0, nBottom = 0, nOut = 0;
  if (limg_encode(img.data(), W, H, true, st.data(), bound, &n) != limg_success) return 1;
  if (limg_encode(img.data(), W, CUT, true, top.data(), bound, &nTop) != limg_success) return 2;
  if (limg_encode(img.data() + W * CUT, W, H - CUT, true, bottom.data(), bound, &nBottom) != limg_success) return 3;
  if (limg_crop_stream(st.data(), n, 4, 0, 8, 8, out.data(), bound, &nOut) != limg_error_InvalidParameter) return 4;
  if (limg_crop_stream(st.data(), n, 16, 0, 56, 28, out.data(), bound, &nOut) != limg_success) return 5;
  if (limg_decode(out.data(), nOut, a.data(), a.size()) != limg_success) return 6;
  if (limg_decode_window(st.data(), n, 16, 0, 56, 28, b.data(), 56) != limg_success) return 7;
  if (memcmp(a.data(), b.data(), 56 * 28 * sizeof(uint32_t)) != 0) return 8;
  const limg_hip_splice_piece pieces[2] = { { top.data(), nTop, W, CUT, 0, 0, 0, 0, 9, 2 }, { bottom.data(), nBottom, W, H - CUT, 0, 0, 0, 2, 9, 2 } };
  if (limg_splice_streams(pieces, 1, W, H, true, out.data(), bound, &nOut) != limg_error_InvalidParameter) return 9;
  if (limg_splice_streams(pieces, 2, W, H, true, out.data(), bound, &nOut, 100, 1) != limg_success) return 10;
  if (limg_decode(out.data(), nOut, a.data(), a.size()) != limg_success) return 11;
  if (limg_decode(top.data(), nTop, b.data(), b.size()) != limg_success) return 12;
  if (limg_decode(bottom.data(), nBottom, b.data() + W * CUT, b.size() - W * CUT) != limg_success) return 13;
  if (memcmp(a.data(), b.data(), W * H * sizeof(uint32_t)) != 0) return 14;
  puts("shim crop and join ok");
  return 0;
}
'''


def _link_flags(lib):
    rocm_lib = os.environ.get("ROCM_LIB", "/opt/rocm/lib")
    return ["-L", os.path.dirname(lib), "-l:" + os.path.basename(lib), "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath-link," + rocm_lib, "-Wl,-rpath," + rocm_lib]


def _compile_consumer(lib, tmp_path):
    path = L.PATHS[lib]
    (tmp_path / "consumer.c").write_text(C_SOURCE)
    exe = tmp_path / "consumer"
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(tmp_path / "consumer.c"), "-o", str(exe)] + _link_flags(path)
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, "the limg_hip_stream_splice / limg_hip_stream_crop entries of include/limg_hip.h do not work from C99:\n" + r.stderr[-3000:]
    return exe


def _compile_shim(lib, tmp_path):
    path = L.PATHS[lib]
    (tmp_path / "shim.cpp").write_text(CPP_SOURCE)
    exe = tmp_path / "shim"
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(tmp_path / "shim.cpp"), "-o", str(exe), "-lpthread"] + _link_flags(path)
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, "limg_crop_stream / limg_splice_streams of include/limg_hip_shim.hpp do not compile and link:\n" + r.stderr[-3000:]
    return exe


def test_consumers_compile_and_link(tmp_path):
    """without a GPU: the C99 consumer of the new entries and the shim's program compile and link against the product"""
    from limg_amd import build
    build.build()
    _compile_consumer("product", tmp_path)
    _compile_shim("product", tmp_path)


@pytest.mark.gpu
def test_c_consumer_crops_and_joins(lib, tmp_path):
    exe = _compile_consumer(lib, tmp_path)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-500:])
    assert "stream crop and join ok" in r.stdout


@pytest.mark.gpu
def test_shim_crops_and_joins(lib, tmp_path):
    exe = _compile_shim(lib, tmp_path)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-500:])
    assert "shim crop and join ok" in r.stdout


L.product_twins(globals())  # the programs against the product library as well as the test build (tests/lib_axis.py)
