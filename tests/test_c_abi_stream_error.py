"""The stream error and quality declarations of include/limg_hip.h from C99, without a GPU: a C program includes the header, prints the layout of the three new structs,
links against the library and calls the entries with a NULL context -- limg_hip_error_ArgumentNull (NaN for limg_hip_stream_compare) comes back before anything touches a
device -- and the host-only limg_hip_error_sum_for_psnr.  Both libraries export the new names and nothing the header does not declare, the Python structs have the
header's layout, and a C++ translation unit that includes the shim takes the addresses of limg_compare_stream, limg_encode_quality and limg_encode_quality_batch."""
import ctypes as C
import os
import re
import subprocess

import pytest

import limg_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("limg_hip_decode_stream_windows_error_device", "limg_hip_blocked_decode_stream_windows_error_device", "limg_hip_decode_stream_windows_error",
         "limg_hip_blocked_decode_stream_windows_error", "limg_hip_stream_compare", "limg_hip_error_sum_for_psnr", "limg_hip_encode_stream_quality_device",
         "limg_hip_encode_stream_quality", "limg_hip_encode_stream_quality_batch_device", "limg_hip_encode_stream_quality_batch")

C_SOURCE = r'''
#include <stddef.h>
#include <stdio.h>
#include "limg_hip.h"

int main(void)
{
  static uint32_t px[64];
  static unsigned char stream[4096];
  uint64_t sums[2] = { 7, 7 }, limits[2] = { 1000, 0 };
  double mse = 7.0, max = 7.0, psnr;
  limg_hip_error_window win = { 0, 0, 8, 8, px, 8 };
  limg_hip_error_window_job job;
  limg_hip_quality_result res[2] = { { sizeof(limg_hip_quality_result), 7, 7, 7, 7, 7 }, { sizeof(limg_hip_quality_result), 7, 7, 7, 7, 7 } };
  const uint32_t *ins[2] = { px, px };
  uint8_t *outs[2] = { stream, stream + 2048 };
  job.pStream = stream; job.streamBytes = sizeof stream; job.sizeX = 8; job.sizeY = 8; job.window = win;
  if (limg_hip_decode_stream_windows_error_device(NULL, &job, 1, sums, NULL, NULL) != limg_hip_error_ArgumentNull) return 10;
  if (limg_hip_blocked_decode_stream_windows_error_device(NULL, &job, 1, sums, NULL, NULL) != limg_hip_error_ArgumentNull) return 11;
  if (limg_hip_decode_stream_windows_error(NULL, stream, sizeof stream, &win, 1, sums) != limg_hip_error_ArgumentNull) return 12;
  if (limg_hip_blocked_decode_stream_windows_error(NULL, stream, sizeof stream, &win, 1, sums) != limg_hip_error_ArgumentNull) return 13;
  psnr = limg_hip_stream_compare(NULL, stream, sizeof stream, px, 64, &mse, &max);
  if (psnr == psnr || mse != 7.0 || max != 7.0) return 14; /* NaN, and nothing written */
  if (limg_hip_encode_stream_quality_device(NULL, px, 8, 8, 1, stream, sizeof stream, 1000, 0, 0, 0, 1, &res[0], NULL) != limg_hip_error_ArgumentNull) return 15;
  if (limg_hip_encode_stream_quality(NULL, px, 8, 8, 1, stream, sizeof stream, 1000, 0, 0, 0, 1, &res[0]) != limg_hip_error_ArgumentNull) return 16;
  if (limg_hip_encode_stream_quality_batch_device(NULL, 2, ins, 8, 8, 1, outs, 2048, limits, 0, 0, 0, 1, res, NULL) != limg_hip_error_ArgumentNull) return 17;
  if (limg_hip_encode_stream_quality_batch(NULL, 2, ins, 8, 8, 1, outs, 2048, limits, 0, 0, 0, 1, res) != limg_hip_error_ArgumentNull) return 18;
  if (res[0].errorFactor != 7 || res[1].probes != 7 || res[0].withinTarget != 7 || res[1].bytes != 7 || res[0].errorSum != 7 || sums[0] != 7 || sums[1] != 7) return 19;
  if (limg_hip_error_sum_for_psnr(8, 8, 1, 38.0) != 7914 || limg_hip_error_sum_for_psnr(0, 8, 1, 38.0) != 0) return 20;
  printf("window %lu %lu %lu %lu %lu %lu %lu\n", (unsigned long)sizeof(limg_hip_error_window), (unsigned long)offsetof(limg_hip_error_window, x0),
         (unsigned long)offsetof(limg_hip_error_window, y0), (unsigned long)offsetof(limg_hip_error_window, width), (unsigned long)offsetof(limg_hip_error_window, height),
         (unsigned long)offsetof(limg_hip_error_window, pOriginal), (unsigned long)offsetof(limg_hip_error_window, originalStridePixels));
  printf("job %lu %lu %lu %lu %lu %lu\n", (unsigned long)sizeof(limg_hip_error_window_job), (unsigned long)offsetof(limg_hip_error_window_job, pStream),
         (unsigned long)offsetof(limg_hip_error_window_job, streamBytes), (unsigned long)offsetof(limg_hip_error_window_job, sizeX),
         (unsigned long)offsetof(limg_hip_error_window_job, sizeY), (unsigned long)offsetof(limg_hip_error_window_job, window));
  printf("result %lu %lu %lu %lu %lu %lu %lu\n", (unsigned long)sizeof(limg_hip_quality_result), (unsigned long)offsetof(limg_hip_quality_result, struct_size),
         (unsigned long)offsetof(limg_hip_quality_result, errorFactor), (unsigned long)offsetof(limg_hip_quality_result, probes),
         (unsigned long)offsetof(limg_hip_quality_result, withinTarget), (unsigned long)offsetof(limg_hip_quality_result, bytes),
         (unsigned long)offsetof(limg_hip_quality_result, errorSum));
  return 0;
}
'''

CPP_SOURCE = r'''
#include "limg_hip_shim.hpp"

int main(int argc, char **)
{
  const void *a = (const void *)&limg_compare_stream, *b = (const void *)&limg_encode_quality, *c = (const void *)&limg_encode_quality_batch;
  return a && b && c && argc > 0 ? 0 : 1;
}
'''


def _link_flags(lib):
    rocm_lib = os.environ.get("ROCM_LIB", "/opt/rocm/lib")
    return ["-L", os.path.dirname(lib), "-llimg_hip", "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath-link," + rocm_lib, "-Wl,-rpath," + rocm_lib]


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    from limg_amd import build
    return build.build(), build.build(test_hooks=True), tmp_path_factory.mktemp("c_abi_stream_error")


def _layout(struct):
    return [C.sizeof(struct)] + [getattr(struct, f).offset for f, _ in struct._fields_]


def test_c_consumer_and_the_structs_layout(built):
    lib, _, d = built
    (d / "consumer.c").write_text(C_SOURCE)
    exe = d / "consumer"
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(d / "consumer.c"), "-o", str(exe)] + _link_flags(lib)
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, "the stream error and quality entries of include/limg_hip.h do not work from C99:\n" + r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-500:])
    got = {line.split()[0]: [int(v) for v in line.split()[1:]] for line in r.stdout.splitlines()}
    z = C.sizeof(C.c_size_t)
    assert got["window"] == _layout(limg_amd.ErrorWindow) == [6 * z] + [k * z for k in range(6)], got
    assert got["job"] == _layout(limg_amd.ErrorWindowJob) == [10 * z] + [k * z for k in range(5)], got
    assert got["result"] == _layout(limg_amd.QualityResult) == [32, 0, 4, 8, 12, 16, 24], got


def test_shim_has_the_three_functions(built):
    lib, _, d = built
    (d / "shim.cpp").write_text(CPP_SOURCE)
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(d / "shim.cpp"), "-o", str(d / "shim"), "-lpthread"] + _link_flags(lib)
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def test_both_libraries_export_the_new_names_and_nothing_else_new(built):
    for lib, allowed in zip(built[:2], (set(limg_amd.ABI_SYMBOLS), set(limg_amd.ABI_SYMBOLS) | set(limg_amd.TEST_ABI_SYMBOLS))):
        defined = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
        exported = set(re.findall(r" T (limg_hip_\w+)", defined))
        assert set(NAMES) <= exported, (lib, set(NAMES) - exported)
        assert exported <= allowed, (lib, exported - allowed)
    assert set(NAMES) <= set(limg_amd.ABI_SYMBOLS) and len(set(limg_amd.ABI_SYMBOLS)) == len(limg_amd.ABI_SYMBOLS)
    header = open(os.path.join(ROOT, "include", "limg_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, header), name
    for name in ("decode_stream_windows_error", "decode_stream_windows_error_device", "blocked_decode_stream_windows_error", "blocked_decode_stream_windows_error_device",
                 "stream_compare", "error_sum_for_psnr", "encode_stream_quality", "encode_stream_quality_device", "encode_stream_quality_batch",
                 "encode_stream_quality_batch_device"):
        assert callable(getattr(limg_amd.LimgHip, name))
