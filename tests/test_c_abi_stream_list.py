"""The stream encode of a list of mixed shapes (include/limg_hip.h) from C99: a C program links against the library, runs limg_hip_encode_stream_list on 4 host
images of four shapes (one with partial edge blocks) at four factors and compares every stream, byte for byte, with limg_hip_encode_stream of that image at its
factor; limg_hip_encode_stream_quality_list against limg_hip_encode_stream_quality; the refusals that come back before anything touches a device too.  A second, C++
translation unit includes the shim and takes the addresses of limg_encode_list and limg_encode_quality_list: it compiles and links, and is not run."""
import os
import subprocess

import pytest

import lib_axis as L
from lib_axis import lib, lib_product  # noqa: F401  (fixtures: "test" / "product")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

C_SOURCE = r'''
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "limg_hip.h"

#define N 4

int main(void)
{
  limg_hip_context *ctx = NULL;
  static const uint32_t sx[N] = { 264u, 8u, 13u, 512u }, sy[N] = { 24u, 8u, 9u, 32u }, ef[N] = { 400u, 0u, 37u, 101u };
  limg_hip_stream_list_item items[N], bad[N];
  limg_hip_quality_result res[N], one_res;
  uint64_t limits[N];
  uint32_t *img[N];
  uint8_t *out[N], *single;
  size_t bound[N], bytes[N], one = 0, most = 0;
  uint32_t seed = 12345u;
  int i;
  size_t k;
  if (sizeof(limg_hip_stream_list_item) != 40) return 1;
  for (i = 0; i < N; i++)
  {
    const size_t px = (size_t)sx[i] * sy[i];
    bound[i] = limg_hip_stream_bound(sx[i], sy[i]);
    if (bound[i] == 0) return 1;
    if (bound[i] > most) most = bound[i];
    img[i] = (uint32_t *)malloc(px * sizeof(uint32_t));
    out[i] = (uint8_t *)malloc(bound[i]);
    if (!img[i] || !out[i]) return 2;
    for (k = 0; k < px; k++)
    { /* a gradient per image with a little noise on it, alpha varying */
      const uint32_t x = (uint32_t)(k % sx[i]), y = (uint32_t)(k / sx[i]);
      seed = seed * 1664525u + 1013904223u;
      img[i][k] = ((x + 40u * (uint32_t)i) & 0xFFu) | (((y * 9u + (seed >> 29)) & 0xFFu) << 8) | ((((x + y) >> 1) & 0xFFu) << 16) | (((200u + (seed >> 27)) & 0xFFu) << 24);
    }
    memset(out[i], 0xA5, bound[i]);
    bytes[i] = 0;
    items[i].pIn = img[i]; items[i].pStream = out[i]; items[i].capacity = bound[i];
    items[i].sizeX = sx[i]; items[i].sizeY = sy[i]; items[i].errorFactor = ef[i]; items[i].reserved = 0;
    memset(&res[i], 0, sizeof(res[i])); res[i].struct_size = sizeof(res[i]);
    limits[i] = limg_hip_error_sum_for_psnr(sx[i], sy[i], 1, 38.0);
  }
  single = (uint8_t *)malloc(most);
  if (!single) return 2;
  if (limg_hip_encode_stream_list(NULL, N, items, sizeof(items[0]), 1, bytes, 0, 1) != limg_hip_error_ArgumentNull) return 10;
  if (limg_hip_encode_stream_list_device(NULL, N, items, sizeof(items[0]), 1, bytes, 0, 1, NULL) != limg_hip_error_ArgumentNull) return 11;
  if (limg_hip_init(-1, &ctx) != limg_hip_success) return 3;
  if (limg_hip_encode_stream_list(ctx, N, NULL, sizeof(items[0]), 1, bytes, 0, 1) != limg_hip_error_ArgumentNull) return 12;
  if (limg_hip_encode_stream_list(ctx, N, items, sizeof(items[0]), 1, NULL, 0, 1) != limg_hip_error_ArgumentNull) return 13;
  if (limg_hip_encode_stream_list(ctx, N, items, sizeof(items[0]) - 1, 1, bytes, 0, 1) != limg_hip_error_InvalidParameter) return 14;
  memcpy(bad, items, sizeof(items)); bad[2].sizeX = 0;
  if (limg_hip_encode_stream_list(ctx, N, bad, sizeof(bad[0]), 1, bytes, 0, 1) != limg_hip_error_InvalidParameter) return 15;
  memcpy(bad, items, sizeof(items)); bad[3].reserved = 7;
  if (limg_hip_encode_stream_list(ctx, N, bad, sizeof(bad[0]), 1, bytes, 0, 1) != limg_hip_error_InvalidParameter) return 16;
  memcpy(bad, items, sizeof(items)); bad[1].pIn = NULL; bad[3].reserved = 7; /* the first offending item decides */
  if (limg_hip_encode_stream_list(ctx, N, bad, sizeof(bad[0]), 1, bytes, 0, 1) != limg_hip_error_ArgumentNull) return 17;
  if (limg_hip_encode_stream_quality_list(ctx, N, items, sizeof(items[0]), 1, NULL, 0, 0, 0, 1, res) != limg_hip_error_ArgumentNull) return 18;
  if (limg_hip_encode_stream_quality_list(ctx, N, items, sizeof(items[0]), 1, limits, 3, 0, 0, 1, res) != limg_hip_error_InvalidParameter) return 19;
  if (limg_hip_encode_stream_list(ctx, 0, items, sizeof(items[0]), 1, bytes, 0, 1) != limg_hip_success) return 20;
  for (i = 0; i < N; i++)
    for (k = 0; k < bound[i]; k++)
      if (out[i][k] != 0xA5) return 21; /* a refused call and an empty list write nothing */
  if (limg_hip_encode_stream_list(ctx, N, items, sizeof(items[0]), 1, bytes, 0, 1) != limg_hip_success) return 30;
  for (i = 0; i < N; i++)
  {
    size_t gx = 0, gy = 0, total = 0;
    int alpha = 0;
    if (limg_hip_encode_stream(ctx, img[i], sx[i], sy[i], 1, single, most, &one, ef[i], 0, 1) != limg_hip_success) return 31;
    if (one != bytes[i] || memcmp(single, out[i], one) != 0) { printf("stream %d differs (%lu / %lu bytes)\n", i, (unsigned long)bytes[i], (unsigned long)one); return 32; }
    if (limg_hip_stream_info(out[i], bytes[i], &gx, &gy, &alpha, &total) != limg_hip_success || gx != sx[i] || gy != sy[i] || !alpha || total != bytes[i]) return 33;
    for (k = bytes[i]; k < bound[i]; k++)
      if (out[i][k] != 0xA5) return 34; /* totalBytes of each stream are downloaded, not the capacity */
  }
  /* to a quality target: result and stream of every item are the single call's */
  if (limg_hip_encode_stream_quality_list(ctx, N, items, sizeof(items[0]), 1, limits, 0, 0, 0, 1, res) != limg_hip_success) return 40;
  for (i = 0; i < N; i++)
  {
    memset(&one_res, 0, sizeof(one_res)); one_res.struct_size = sizeof(one_res);
    if (limg_hip_encode_stream_quality(ctx, img[i], sx[i], sy[i], 1, single, most, limits[i], 0, 0, 0, 1, &one_res) != limg_hip_success) return 41;
    if (one_res.errorFactor != res[i].errorFactor || one_res.probes != res[i].probes || one_res.withinTarget != res[i].withinTarget || one_res.bytes != res[i].bytes ||
        one_res.errorSum != res[i].errorSum)
      return 42;
    if (memcmp(single, out[i], (size_t)one_res.bytes) != 0) return 43;
  }
  if (limg_hip_check_device_status(ctx) != limg_hip_success) return 50;
  limg_hip_shutdown(&ctx);
  puts("stream encode of a mixed-shape list ok");
  return 0;
}
'''

CPP_SOURCE = r'''
#include "limg_hip_shim.hpp"

typedef limg_result (*list_fn)(const uint32_t *const *, const size_t, const size_t *, const size_t *, const bool, uint8_t *const *, const size_t *, size_t *, const uint32_t *,
                               limg_thread_pool *, const bool);
typedef limg_result (*quality_fn)(const uint32_t *const *, const size_t, const size_t *, const size_t *, const bool, uint8_t *const *, const size_t *, size_t *, const double *,
                                  uint32_t *, double *, bool *, uint32_t *, const uint32_t, const uint32_t, limg_thread_pool *, const bool);

int main(int argc, char **)
{
  list_fn fn = &limg_encode_list;
  quality_fn qn = &limg_encode_quality_list;
  return fn != nullptr && qn != nullptr && argc > 0 ? 0 : 1;
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
    assert r.returncode == 0, "the limg_hip_encode_stream_list entries of include/limg_hip.h do not work from C99:\n" + r.stderr[-3000:]
    return exe


def test_c_consumer_compiles_and_links(tmp_path):
    """without a GPU: the C99 consumer of the new entries compiles and links against the product"""
    from limg_amd import build
    build.build()
    _compile_consumer("product", tmp_path)


@pytest.mark.gpu
def test_c_consumer_of_the_stream_list(lib, tmp_path):
    exe = _compile_consumer(lib, tmp_path)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-500:])
    assert "stream encode of a mixed-shape list ok" in r.stdout


def test_shim_declares_limg_encode_list(tmp_path):
    from limg_amd import build
    lib = build.build()
    (tmp_path / "shim.cpp").write_text(CPP_SOURCE)
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(tmp_path / "shim.cpp"), "-o", str(tmp_path / "shim"), "-lpthread"] + _link_flags(lib)
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, "limg_encode_list / limg_encode_quality_list of include/limg_hip_shim.hpp do not compile and link:\n" + r.stderr[-3000:]


L.product_twins(globals())  # the C program against the product library as well as the test build (tests/lib_axis.py)
