"""The batched stream encode with one error factor per image (include/limg_hip.h) from C99: a C program links against the library, runs
limg_hip_encode_stream_batch_ef on 3 host images at three factors and compares every stream, byte for byte, with limg_hip_encode_stream of that image at its factor;
the refusals that come back before anything touches a device too.  A second, C++ translation unit includes the shim and takes the address of limg_encode_batch_ef: it
compiles and links, and is not run."""
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

#define W 264
#define H 24
#define N 3

int main(void)
{
  limg_hip_context *ctx = NULL;
  const size_t bound = limg_hip_stream_bound(W, H);
  uint32_t *img[N];
  const uint32_t *in[N];
  uint8_t *batch[N], *single;
  size_t bytes[N], one = 0;
  uint32_t seed = 12345u;
  const uint32_t ef[N] = { 400u, 0u, 37u };
  int i;
  size_t k;
  if (bound == 0) return 1;
  single = (uint8_t *)malloc(bound);
  for (i = 0; i < N; i++)
  {
    img[i] = (uint32_t *)malloc(W * H * sizeof(uint32_t));
    batch[i] = (uint8_t *)malloc(bound);
    if (!img[i] || !batch[i] || !single) return 2;
    for (k = 0; k < (size_t)W * H; k++)
    { /* a gradient per image with a little noise on it, alpha varying */
      const uint32_t x = (uint32_t)(k % W), y = (uint32_t)(k / W);
      seed = seed * 1664525u + 1013904223u;
      img[i][k] = ((x + 40u * (uint32_t)i) & 0xFFu) | (((y * 9u + (seed >> 29)) & 0xFFu) << 8) | ((((x + y) >> 1) & 0xFFu) << 16) | (((200u + (seed >> 27)) & 0xFFu) << 24);
    }
    in[i] = img[i];
    memset(batch[i], 0xA5, bound);
    bytes[i] = 0;
  }
  if (limg_hip_encode_stream_batch_ef(NULL, N, in, W, H, 1, batch, bound, bytes, ef, 0, 1) != limg_hip_error_ArgumentNull) return 10;
  if (limg_hip_encode_stream_batch_ef_device(NULL, N, in, W, H, 1, batch, bound, bytes, ef, 0, 1, NULL) != limg_hip_error_ArgumentNull) return 11;
  if (limg_hip_init(-1, &ctx) != limg_hip_success) return 3;
  if (limg_hip_encode_stream_batch_ef(ctx, N, in, W, H, 1, batch, bound, NULL, ef, 0, 1) != limg_hip_error_ArgumentNull) return 12;
  if (limg_hip_encode_stream_batch_ef(ctx, N, in, W, H, 1, batch, bound, bytes, NULL, 0, 1) != limg_hip_error_ArgumentNull) return 17;
  if (limg_hip_encode_stream_batch_ef(ctx, N, in, 0, H, 1, batch, bound, bytes, NULL, 0, 1) != limg_hip_error_ArgumentNull) return 18; /* pointers first */
  if (limg_hip_encode_stream_batch_ef(ctx, N, in, W, H, 1, batch, bound - 1, bytes, ef, 0, 1) != limg_hip_error_OutOfBounds) return 13;
  if (limg_hip_encode_stream_batch_ef(ctx, N, in, 0, H, 1, batch, bound, bytes, ef, 0, 1) != limg_hip_error_InvalidParameter) return 14;
  if (limg_hip_encode_stream_batch_ef(ctx, 0, in, W, H, 1, batch, bound, bytes, ef, 0, 1) != limg_hip_success) return 15;
  for (i = 0; i < N; i++)
    for (k = 0; k < bound; k++)
      if (batch[i][k] != 0xA5) return 16; /* a refused call and an empty list write nothing */
  if (limg_hip_encode_stream_batch_ef(ctx, N, in, W, H, 1, batch, bound, bytes, ef, 0, 1) != limg_hip_success) return 20;
  for (i = 0; i < N; i++)
  {
    size_t sx = 0, sy = 0, total = 0;
    int alpha = 0;
    if (limg_hip_encode_stream(ctx, img[i], W, H, 1, single, bound, &one, ef[i], 0, 1) != limg_hip_success) return 21;
    if (one != bytes[i] || memcmp(single, batch[i], one) != 0) { printf("stream %d differs (%lu / %lu bytes)\n", i, (unsigned long)bytes[i], (unsigned long)one); return 22; }
    if (limg_hip_stream_info(batch[i], bytes[i], &sx, &sy, &alpha, &total) != limg_hip_success || sx != W || sy != H || !alpha || total != bytes[i]) return 23;
    for (k = bytes[i]; k < bound; k++)
      if (batch[i][k] != 0xA5) return 24; /* totalBytes of each stream are downloaded, not the capacity */
  }
  if (memcmp(batch[0], batch[1], bytes[0] < bytes[1] ? bytes[0] : bytes[1]) == 0) return 25; /* (different images: different streams) */
  if (limg_hip_check_device_status(ctx) != limg_hip_success) return 30;
  limg_hip_shutdown(&ctx);
  puts("batched stream encode with per-image error factors ok");
  return 0;
}
'''

CPP_SOURCE = r'''
#include "limg_hip_shim.hpp"

typedef limg_result (*batch_fn)(const uint32_t *const *, const size_t, const size_t, const size_t, const bool, uint8_t *const *, const size_t, size_t *, const uint32_t *,
                                limg_thread_pool *, const bool);

int main(int argc, char **)
{
  batch_fn fn = &limg_encode_batch_ef;
  return fn != nullptr && argc > 0 ? 0 : 1;
}
'''


def _link_flags(lib):
    rocm_lib = os.environ.get("ROCM_LIB", "/opt/rocm/lib")
    return ["-L", os.path.dirname(lib), "-l:" + os.path.basename(lib), "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath-link," + rocm_lib, "-Wl,-rpath," + rocm_lib]


@pytest.mark.gpu
def test_c_consumer_of_the_batched_stream_encode_ef(lib, tmp_path):
    path = L.PATHS[lib]
    (tmp_path / "consumer.c").write_text(C_SOURCE)
    exe = tmp_path / "consumer"
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(tmp_path / "consumer.c"), "-o", str(exe)] + _link_flags(path)
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, "the limg_hip_encode_stream_batch_ef entries of include/limg_hip.h do not work from C99:\n" + r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-500:])
    assert "batched stream encode with per-image error factors ok" in r.stdout


def test_shim_declares_limg_encode_batch_ef(tmp_path):
    from limg_amd import build
    lib = build.build()
    (tmp_path / "shim.cpp").write_text(CPP_SOURCE)
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(tmp_path / "shim.cpp"), "-o", str(tmp_path / "shim"), "-lpthread"] + _link_flags(lib)
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, "limg_encode_batch_ef of include/limg_hip_shim.hpp does not compile and link:\n" + r.stderr[-3000:]


L.product_twins(globals())  # the C program against the product library as well as the test build (tests/lib_axis.py)
