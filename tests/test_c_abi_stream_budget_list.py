"""The byte budget and the size probe for a list of mixed shapes (include/limg_hip.h) from C99: a C program links against the library, runs
limg_hip_encode_stream_budget_list on 4 host images of four shapes (one with partial edge blocks) and compares every result and stream, byte for byte, with
limg_hip_encode_stream_budget of that image; limg_hip_stream_sizes_list against limg_hip_stream_sizes; the refusals that come back before anything touches a device
too.  A second, C++ translation unit includes the shim and takes the addresses of limg_encode_budget_list and limg_stream_sizes_list: it compiles and links, and is
not run."""
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
#define F 3

int main(void)
{
  limg_hip_context *ctx = NULL;
  static const uint32_t sx[N] = { 264u, 8u, 13u, 512u }, sy[N] = { 24u, 8u, 9u, 32u }, factors[F] = { 0u, 37u, 400u };
  limg_hip_stream_list_item items[N], bad[N];
  limg_hip_budget_result res[N], one_res;
  size_t budgets[N], zero[N];
  uint32_t *img[N];
  uint8_t *out[N], *single;
  size_t bound[N], sizes[N * F], one[F], most = 0;
  uint32_t seed = 12345u;
  int i;
  size_t k;
  if (sizeof(limg_hip_stream_list_item) != 40 || sizeof(limg_hip_budget_result) != 24) return 1;
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
    items[i].pIn = img[i]; items[i].pStream = out[i]; items[i].capacity = bound[i];
    items[i].sizeX = sx[i]; items[i].sizeY = sy[i]; items[i].errorFactor = 999u; items[i].reserved = 0; /* (errorFactor is ignored) */
    memset(&res[i], 0, sizeof(res[i])); res[i].struct_size = sizeof(res[i]);
    budgets[i] = 64u + 56u * ((sx[i] + 7u) / 8u) * ((sy[i] + 7u) / 8u) + 40u * (size_t)((sx[i] + 7u) / 8u) * ((sy[i] + 7u) / 8u); /* the fixed bytes + 5 words per block */
    zero[i] = i == 2 ? 0u : budgets[i];
  }
  for (k = 0; k < N * F; k++) sizes[k] = 0xA5A5u;
  single = (uint8_t *)malloc(most);
  if (!single) return 2;
  if (limg_hip_encode_stream_budget_list(NULL, N, items, sizeof(items[0]), 1, budgets, 0, 0, 0, 1, res) != limg_hip_error_ArgumentNull) return 10;
  if (limg_hip_encode_stream_budget_list_device(NULL, N, items, sizeof(items[0]), 1, budgets, 0, 0, 0, 1, res, NULL) != limg_hip_error_ArgumentNull) return 11;
  if (limg_hip_stream_sizes_list(NULL, N, items, sizeof(items[0]), 1, factors, F, sizes, 0, 1) != limg_hip_error_ArgumentNull) return 12;
  if (limg_hip_stream_sizes_list_device(NULL, N, items, sizeof(items[0]), 1, factors, F, sizes, 0, 1, NULL) != limg_hip_error_ArgumentNull) return 13;
  if (limg_hip_init(-1, &ctx) != limg_hip_success) return 3;
  if (limg_hip_encode_stream_budget_list(ctx, N, NULL, sizeof(items[0]), 1, budgets, 0, 0, 0, 1, res) != limg_hip_error_ArgumentNull) return 14;
  if (limg_hip_encode_stream_budget_list(ctx, N, items, sizeof(items[0]), 1, NULL, 0, 0, 0, 1, res) != limg_hip_error_ArgumentNull) return 15;
  if (limg_hip_encode_stream_budget_list(ctx, N, items, sizeof(items[0]), 1, budgets, 0, 0, 0, 1, NULL) != limg_hip_error_ArgumentNull) return 16;
  if (limg_hip_encode_stream_budget_list(ctx, N, items, sizeof(items[0]) - 1, 1, budgets, 0, 0, 0, 1, res) != limg_hip_error_InvalidParameter) return 17;
  memcpy(bad, items, sizeof(items)); bad[2].sizeX = 0;
  if (limg_hip_encode_stream_budget_list(ctx, N, bad, sizeof(bad[0]), 1, budgets, 0, 0, 0, 1, res) != limg_hip_error_InvalidParameter) return 18;
  memcpy(bad, items, sizeof(items)); bad[1].pIn = NULL; bad[3].reserved = 7; /* the first offending item decides, and an item rule comes before a bound rule */
  if (limg_hip_encode_stream_budget_list(ctx, N, bad, sizeof(bad[0]), 1, budgets, 3, 0, 0, 1, res) != limg_hip_error_ArgumentNull) return 19;
  if (limg_hip_encode_stream_budget_list(ctx, N, items, sizeof(items[0]), 1, budgets, 3, 0, 0, 1, res) != limg_hip_error_InvalidParameter) return 20;
  if (limg_hip_encode_stream_budget_list(ctx, N, items, sizeof(items[0]), 1, budgets, 200, 100, 0, 1, res) != limg_hip_error_InvalidParameter) return 21;
  if (limg_hip_encode_stream_budget_list(ctx, N, items, sizeof(items[0]), 1, zero, 0, 0, 0, 1, res) != limg_hip_error_InvalidParameter) return 22;
  res[3].struct_size = 16;
  if (limg_hip_encode_stream_budget_list(ctx, N, items, sizeof(items[0]), 1, budgets, 0, 0, 0, 1, res) != limg_hip_error_InvalidParameter) return 23;
  res[3].struct_size = sizeof(res[3]);
  if (limg_hip_encode_stream_budget_list(ctx, 0, items, sizeof(items[0]), 1, budgets, 0, 0, 0, 1, res) != limg_hip_success) return 24;
  memcpy(bad, items, sizeof(items)); bad[0].pStream = NULL; bad[0].capacity = 0; /* the sizes list does not look at either */
  if (limg_hip_stream_sizes_list(ctx, N, bad, sizeof(bad[0]), 1, NULL, F, sizes, 0, 1) != limg_hip_error_ArgumentNull) return 25;
  if (limg_hip_stream_sizes_list(ctx, N, bad, sizeof(bad[0]), 1, factors, F, NULL, 0, 1) != limg_hip_error_ArgumentNull) return 26;
  bad[1].reserved = 1;
  if (limg_hip_stream_sizes_list(ctx, N, bad, sizeof(bad[0]), 1, factors, F, sizes, 0, 1) != limg_hip_error_InvalidParameter) return 27;
  bad[1].reserved = 0;
  if (limg_hip_stream_sizes_list(ctx, N, bad, sizeof(bad[0]), 1, factors, 0, sizes, 0, 1) != limg_hip_success) return 28;
  if (limg_hip_stream_sizes_list(ctx, 0, bad, sizeof(bad[0]), 1, factors, F, sizes, 0, 1) != limg_hip_success) return 29;
  for (i = 0; i < N; i++)
  {
    if (res[i].errorFactor != 0 || res[i].bytes != 0) return 30;
    for (k = 0; k < bound[i]; k++)
      if (out[i][k] != 0xA5) return 31; /* a refused call and an empty list write nothing */
  }
  for (k = 0; k < N * F; k++)
    if (sizes[k] != 0xA5A5u) return 32;
  /* the sizes of every image at every factor are the single call's */
  if (limg_hip_stream_sizes_list(ctx, N, bad, sizeof(bad[0]), 1, factors, F, sizes, 0, 1) != limg_hip_success) return 40;
  for (i = 0; i < N; i++)
  {
    if (limg_hip_stream_sizes(ctx, img[i], sx[i], sy[i], 1, factors, F, one, 0, 1) != limg_hip_success) return 41;
    for (k = 0; k < F; k++)
      if (one[k] != sizes[(size_t)i * F + k]) { printf("size %d / %lu differs (%lu / %lu bytes)\n", i, (unsigned long)k, (unsigned long)sizes[(size_t)i * F + k], (unsigned long)one[k]); return 42; }
  }
  /* to a byte budget: result and stream of every item are the single call's */
  if (limg_hip_encode_stream_budget_list(ctx, N, items, sizeof(items[0]), 1, budgets, 0, 0, 0, 1, res) != limg_hip_success) return 50;
  for (i = 0; i < N; i++)
  {
    size_t gx = 0, gy = 0, total = 0;
    int alpha = 0;
    memset(&one_res, 0, sizeof(one_res)); one_res.struct_size = sizeof(one_res);
    if (limg_hip_encode_stream_budget(ctx, img[i], sx[i], sy[i], 1, single, most, budgets[i], 0, 0, 0, 1, &one_res) != limg_hip_success) return 51;
    if (one_res.errorFactor != res[i].errorFactor || one_res.probes != res[i].probes || one_res.withinBudget != res[i].withinBudget || one_res.bytes != res[i].bytes)
    {
      printf("result %d differs: %u %u %u %lu / %u %u %u %lu\n", i, res[i].errorFactor, res[i].probes, res[i].withinBudget, (unsigned long)res[i].bytes, one_res.errorFactor,
             one_res.probes, one_res.withinBudget, (unsigned long)one_res.bytes);
      return 52;
    }
    if (memcmp(single, out[i], (size_t)one_res.bytes) != 0) return 53;
    if (limg_hip_stream_info(out[i], (size_t)res[i].bytes, &gx, &gy, &alpha, &total) != limg_hip_success || gx != sx[i] || gy != sy[i] || !alpha || total != res[i].bytes) return 54;
    for (k = (size_t)res[i].bytes; k < bound[i]; k++)
      if (out[i][k] != 0xA5) return 55; /* totalBytes of each stream are downloaded, not the capacity */
  }
  if (limg_hip_check_device_status(ctx) != limg_hip_success) return 60;
  limg_hip_shutdown(&ctx);
  puts("budget and sizes of a mixed-shape list ok");
  return 0;
}
'''

CPP_SOURCE = r'''
#include "limg_hip_shim.hpp"

typedef limg_result (*budget_fn)(const uint32_t *const *, const size_t, const size_t *, const size_t *, const bool, uint8_t *const *, const size_t *, size_t *, const size_t *,
                                 uint32_t *, bool *, uint32_t *, const uint32_t, const uint32_t, limg_thread_pool *, const bool);
typedef limg_result (*sizes_fn)(const uint32_t *const *, const size_t, const size_t *, const size_t *, const bool, const uint32_t *, const size_t, size_t *, limg_thread_pool *,
                                const bool);

int main(int argc, char **)
{
  budget_fn bn = &limg_encode_budget_list;
  sizes_fn sn = &limg_stream_sizes_list;
  return bn != nullptr && sn != nullptr && argc > 0 ? 0 : 1;
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
    assert r.returncode == 0, "the limg_hip_encode_stream_budget_list / limg_hip_stream_sizes_list entries of include/limg_hip.h do not work from C99:\n" + r.stderr[-3000:]
    return exe


def test_c_consumer_compiles_and_links(tmp_path):
    """without a GPU: the C99 consumer of the new entries compiles and links against the product"""
    from limg_amd import build
    build.build()
    _compile_consumer("product", tmp_path)


@pytest.mark.gpu
def test_c_consumer_of_the_budget_list(lib, tmp_path):
    exe = _compile_consumer(lib, tmp_path)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-500:])
    assert "budget and sizes of a mixed-shape list ok" in r.stdout


def test_shim_declares_the_list_functions(tmp_path):
    from limg_amd import build
    lib = build.build()
    (tmp_path / "shim.cpp").write_text(CPP_SOURCE)
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(tmp_path / "shim.cpp"), "-o", str(tmp_path / "shim"), "-lpthread"] + _link_flags(lib)
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, "limg_encode_budget_list / limg_stream_sizes_list of include/limg_hip_shim.hpp do not compile and link:\n" + r.stderr[-3000:]


L.product_twins(globals())  # the C program against the product library as well as the test build (tests/lib_axis.py)
