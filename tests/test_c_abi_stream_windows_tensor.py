"""The tensor window decode declarations of include/limg_hip.h from C99: a C program includes the header, checks the layout of the three structs, links against the
library and calls the four entries with a NULL context -- limg_hip_error_ArgumentNull comes back before anything touches a device, so this runs everywhere.  Both
libraries export the four names.  A C++ translation unit includes the shim and takes the address of limg_decode_windows_tensor: it compiles and links, and is not run."""
import os
import subprocess

import pytest

import limg_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("limg_hip_decode_stream_windows_tensor_device", "limg_hip_blocked_decode_stream_windows_tensor_device", "limg_hip_decode_stream_windows_tensor",
         "limg_hip_blocked_decode_stream_windows_tensor")

C_SOURCE = r'''
#include <stddef.h>
#include <stdio.h>
#include "limg_hip.h"

int main(void)
{
  static unsigned char stream[128];
  float out[12];
  limg_hip_tensor_format fmt = { LIMG_HIP_TENSOR_F32, 3, { 1.0f, 1.0f, 1.0f, 1.0f }, { 0.0f, 0.0f, 0.0f, 0.0f } };
  limg_hip_tensor_window win = { 0, 0, 2, 2, NULL, 2, 4 };
  limg_hip_tensor_window_job job = { NULL, sizeof stream, 8, 8, { 0, 0, 2, 2, NULL, 2, 4 } };
  win.pOut = out;
  job.pStream = stream;
  job.window = win;
  if (LIMG_HIP_TENSOR_F32 != 0 || LIMG_HIP_TENSOR_F16 != 1) return 1;
  if (sizeof(limg_hip_tensor_format) != 40) return 2;
  if (sizeof(limg_hip_tensor_window) != 7 * sizeof(size_t)) return 3;
  if (sizeof(limg_hip_tensor_window_job) != 11 * sizeof(size_t)) return 4;
  if (offsetof(limg_hip_tensor_format, scale) != 8 || offsetof(limg_hip_tensor_format, bias) != 24) return 5;
  if (offsetof(limg_hip_tensor_window, pOut) != 4 * sizeof(size_t) || offsetof(limg_hip_tensor_window, planeStride) != 6 * sizeof(size_t)) return 6;
  if (offsetof(limg_hip_tensor_window_job, window) != 4 * sizeof(size_t)) return 7;
  if (limg_hip_decode_stream_windows_tensor_device(NULL, &job, 1, &fmt, NULL, NULL) != limg_hip_error_ArgumentNull) return 10;
  if (limg_hip_blocked_decode_stream_windows_tensor_device(NULL, &job, 1, &fmt, NULL, NULL) != limg_hip_error_ArgumentNull) return 11;
  if (limg_hip_decode_stream_windows_tensor(NULL, stream, sizeof stream, &win, 1, &fmt) != limg_hip_error_ArgumentNull) return 12;
  if (limg_hip_blocked_decode_stream_windows_tensor(NULL, stream, sizeof stream, &win, 1, &fmt) != limg_hip_error_ArgumentNull) return 13;
  puts("tensor window decode entries ok");
  return 0;
}
'''

CPP_SOURCE = r'''
#include "limg_hip_shim.hpp"

typedef limg_result (*tensor_fn)(const uint8_t *, const size_t, const limg_hip_tensor_window *, const size_t, const limg_hip_tensor_format *);

int main(int argc, char **)
{
  tensor_fn fn = &limg_decode_windows_tensor;
  return fn != nullptr && argc > 0 ? 0 : 1;
}
'''


def _link_flags(lib):
    rocm_lib = os.environ.get("ROCM_LIB", "/opt/rocm/lib")
    return ["-L", os.path.dirname(lib), "-llimg_hip", "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath-link," + rocm_lib, "-Wl,-rpath," + rocm_lib]


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    from limg_amd import build
    return build.build(), build.build(test_hooks=True), tmp_path_factory.mktemp("c_abi_stream_windows_tensor")


def test_c_consumer_of_the_tensor_window_entries(built):
    lib, _, d = built
    (d / "consumer.c").write_text(C_SOURCE)
    exe = d / "consumer"
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(d / "consumer.c"), "-o", str(exe)] + _link_flags(lib)
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, "the tensor window decode entries of include/limg_hip.h do not work from C99:\n" + r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-500:])
    assert "tensor window decode entries ok" in r.stdout


def test_both_libraries_export_the_four_names(built):
    for lib in built[:2]:
        defined = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
        for name in NAMES:
            assert (" T " + name + "\n") in defined, (lib, name)
    assert set(NAMES) <= set(limg_amd.ABI_SYMBOLS)


def test_python_structs_match_the_header():
    import ctypes as C
    assert C.sizeof(limg_amd.TensorFormat) == 40 and C.sizeof(limg_amd.TensorWindow) == 7 * C.sizeof(C.c_size_t)
    assert C.sizeof(limg_amd.TensorWindowJob) == 11 * C.sizeof(C.c_size_t)


def test_shim_declares_limg_decode_windows_tensor(built):
    lib, _, d = built
    (d / "shim.cpp").write_text(CPP_SOURCE)
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(d / "shim.cpp"), "-o", str(d / "shim"), "-lpthread"] + _link_flags(lib)
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, "limg_decode_windows_tensor of include/limg_hip_shim.hpp does not compile and link:\n" + r.stderr[-3000:]
