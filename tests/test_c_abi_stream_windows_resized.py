"""The resized window decode declarations of include/limg_hip.h from C99: a C program includes the header, checks the layout of the four structs -- the members up to
the strides at the offsets they have in limg_hip_window / limg_hip_tensor_window --, links against the library and calls the eight entries with a NULL context:
limg_hip_error_ArgumentNull comes back before anything touches a device, so this runs everywhere.  Both libraries export the eight names.  A C++ translation unit
includes the shim and takes the addresses of limg_decode_windows_resized and limg_decode_windows_resized_tensor: it compiles and links, and is not run."""
import ctypes as C
import os
import subprocess

import pytest

import limg_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = tuple(v + "decode_stream_windows_resized" + t + d for v in ("limg_hip_", "limg_hip_blocked_") for t in ("", "_tensor") for d in ("_device", ""))

C_SOURCE = r'''
#include <stddef.h>
#include <stdio.h>
#include "limg_hip.h"

int main(void)
{
  static unsigned char stream[128];
  static uint32_t px[4];
  static float out[12];
  limg_hip_tensor_format fmt = { LIMG_HIP_TENSOR_F32, 3, { 1.0f, 1.0f, 1.0f, 1.0f }, { 0.0f, 0.0f, 0.0f, 0.0f } };
  limg_hip_resized_window win = { 0, 0, 4, 4, NULL, 2, 2, 2, LIMG_HIP_RESIZE_AUTO, LIMG_HIP_RESIZE_FLIP_X };
  limg_hip_resized_tensor_window twin = { 0, 0, 4, 4, NULL, 2, 4, 2, 2, 1, 0 };
  limg_hip_resized_window_job job = { NULL, sizeof stream, 8, 8, { 0, 0, 4, 4, NULL, 2, 2, 2, 1, 0 } };
  limg_hip_resized_tensor_window_job tjob = { NULL, sizeof stream, 8, 8, { 0, 0, 4, 4, NULL, 2, 4, 2, 2, 1, 0 } };
  win.pOut = px; twin.pOut = out;
  job.pStream = stream; job.window = win;
  tjob.pStream = stream; tjob.window = twin;
  if (LIMG_HIP_RESIZE_AUTO != 0xFFFFFFFFu || LIMG_HIP_RESIZE_FLIP_X != 1u) return 20;
  if (sizeof(limg_hip_resized_window) != 9 * sizeof(size_t) || offsetof(limg_hip_resized_window, outWidth) != 6 * sizeof(size_t)) return 1;
  if (offsetof(limg_hip_resized_window, outHeight) != 7 * sizeof(size_t) || offsetof(limg_hip_resized_window, log2Scale) != 8 * sizeof(size_t)) return 1;
  if (offsetof(limg_hip_resized_window, flags) != 8 * sizeof(size_t) + 4) return 1;
  if (sizeof(limg_hip_resized_tensor_window) != 10 * sizeof(size_t) || offsetof(limg_hip_resized_tensor_window, outWidth) != 7 * sizeof(size_t)) return 2;
  if (offsetof(limg_hip_resized_tensor_window, log2Scale) != 9 * sizeof(size_t) || offsetof(limg_hip_resized_tensor_window, flags) != 9 * sizeof(size_t) + 4) return 2;
  if (sizeof(limg_hip_resized_window_job) != 13 * sizeof(size_t) || offsetof(limg_hip_resized_window_job, window) != 4 * sizeof(size_t)) return 3;
  if (sizeof(limg_hip_resized_tensor_window_job) != 14 * sizeof(size_t) || offsetof(limg_hip_resized_tensor_window_job, window) != 4 * sizeof(size_t)) return 4;
  if (offsetof(limg_hip_resized_window, x0) != offsetof(limg_hip_window, x0) || offsetof(limg_hip_resized_window, height) != offsetof(limg_hip_window, height)) return 5;
  if (offsetof(limg_hip_resized_window, pOut) != offsetof(limg_hip_window, pOut) || offsetof(limg_hip_resized_window, outStridePixels) != offsetof(limg_hip_window, outStridePixels)) return 5;
  if (offsetof(limg_hip_resized_tensor_window, pOut) != offsetof(limg_hip_tensor_window, pOut) || offsetof(limg_hip_resized_tensor_window, rowStride) != offsetof(limg_hip_tensor_window, rowStride)) return 6;
  if (offsetof(limg_hip_resized_tensor_window, planeStride) != offsetof(limg_hip_tensor_window, planeStride)) return 6;
  if (sizeof(limg_hip_window) != 6 * sizeof(size_t) || sizeof(limg_hip_tensor_window) != 7 * sizeof(size_t)) return 7; /* the existing structs keep their layout */
  if (sizeof(limg_hip_scaled_window) != 7 * sizeof(size_t) || sizeof(limg_hip_scaled_tensor_window) != 8 * sizeof(size_t)) return 7;
  if (limg_hip_decode_stream_windows_resized_device(NULL, &job, 1, NULL, NULL) != limg_hip_error_ArgumentNull) return 10;
  if (limg_hip_blocked_decode_stream_windows_resized_device(NULL, &job, 1, NULL, NULL) != limg_hip_error_ArgumentNull) return 11;
  if (limg_hip_decode_stream_windows_resized_tensor_device(NULL, &tjob, 1, &fmt, NULL, NULL) != limg_hip_error_ArgumentNull) return 12;
  if (limg_hip_blocked_decode_stream_windows_resized_tensor_device(NULL, &tjob, 1, &fmt, NULL, NULL) != limg_hip_error_ArgumentNull) return 13;
  if (limg_hip_decode_stream_windows_resized(NULL, stream, sizeof stream, &win, 1) != limg_hip_error_ArgumentNull) return 14;
  if (limg_hip_blocked_decode_stream_windows_resized(NULL, stream, sizeof stream, &win, 1) != limg_hip_error_ArgumentNull) return 15;
  if (limg_hip_decode_stream_windows_resized_tensor(NULL, stream, sizeof stream, &twin, 1, &fmt) != limg_hip_error_ArgumentNull) return 16;
  if (limg_hip_blocked_decode_stream_windows_resized_tensor(NULL, stream, sizeof stream, &twin, 1, &fmt) != limg_hip_error_ArgumentNull) return 17;
  puts("resized window decode entries ok");
  return 0;
}
'''

CPP_SOURCE = r'''
#include "limg_hip_shim.hpp"

typedef limg_result (*resized_fn)(const uint8_t *, const size_t, const limg_hip_resized_window *, const size_t);
typedef limg_result (*resized_tensor_fn)(const uint8_t *, const size_t, const limg_hip_resized_tensor_window *, const size_t, const limg_hip_tensor_format *);

int main(int argc, char **)
{
  resized_fn a = &limg_decode_windows_resized;
  resized_tensor_fn b = &limg_decode_windows_resized_tensor;
  return a != nullptr && b != nullptr && argc > 0 ? 0 : 1;
}
'''


def _link_flags(lib):
    rocm_lib = os.environ.get("ROCM_LIB", "/opt/rocm/lib")
    return ["-L", os.path.dirname(lib), "-llimg_hip", "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath-link," + rocm_lib, "-Wl,-rpath," + rocm_lib]


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    from limg_amd import build
    return build.build(), build.build(test_hooks=True), tmp_path_factory.mktemp("c_abi_stream_windows_resized")


def test_c_consumer_of_the_resized_window_entries(built):
    lib, _, d = built
    (d / "consumer.c").write_text(C_SOURCE)
    exe = d / "consumer"
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(d / "consumer.c"), "-o", str(exe)] + _link_flags(lib)
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, "the resized window decode entries of include/limg_hip.h do not work from C99:\n" + r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-500:])
    assert "resized window decode entries ok" in r.stdout


def test_both_libraries_export_the_eight_names(built):
    assert len(set(NAMES)) == 8
    for lib in built[:2]:
        defined = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
        for name in NAMES:
            assert (" T " + name + "\n") in defined, (lib, name)
    assert set(NAMES) <= set(limg_amd.ABI_SYMBOLS)


def test_python_structs_match_the_header():
    z = C.sizeof(C.c_size_t)
    assert C.sizeof(limg_amd.ResizedWindow) == 9 * z and C.sizeof(limg_amd.ResizedWindowJob) == 13 * z
    assert C.sizeof(limg_amd.ResizedTensorWindow) == 10 * z and C.sizeof(limg_amd.ResizedTensorWindowJob) == 14 * z
    assert limg_amd.ResizedWindow.outWidth.offset == 6 * z and limg_amd.ResizedWindow.flags.offset == 8 * z + 4
    assert limg_amd.ResizedTensorWindow.outWidth.offset == 7 * z and limg_amd.ResizedTensorWindow.flags.offset == 9 * z + 4
    assert (limg_amd.RESIZE_AUTO, limg_amd.RESIZE_FLIP_X) == (0xFFFFFFFF, 1)
    for name in ("decode_stream_windows_resized_device", "decode_stream_windows_resized_tensor_device", "decode_stream_windows_resized", "decode_stream_windows_resized_tensor"):
        assert callable(getattr(limg_amd.LimgHip, name)) and callable(getattr(limg_amd.LimgHip, "blocked_" + name))
    assert callable(limg_amd.LimgHip.decode_crops_resized_device)
    assert dict(limg_amd.TestOptions._fields_)["resize_tile_pixels"] is C.c_int32 and limg_amd.TestOptions._fields_[-1][0] == "resize_tile_pixels"


def test_shim_declares_the_resized_window_decodes(built):
    lib, _, d = built
    (d / "shim.cpp").write_text(CPP_SOURCE)
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(d / "shim.cpp"), "-o", str(d / "shim"), "-lpthread"] + _link_flags(lib)
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, "the resized window decodes of include/limg_hip_shim.hpp do not compile and link:\n" + r.stderr[-3000:]
