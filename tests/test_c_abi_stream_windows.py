"""The batched window decode declarations of include/limg_hip.h from C99: a C program includes the header, checks the layout of the two structs, links against
liblimg_hip.so and calls the four entries with a NULL context -- limg_hip_error_ArgumentNull comes back before anything touches a device, so this runs everywhere.  A
second, C++ translation unit includes the shim and takes the address of limg_decode_windows: it compiles and links, and is not run."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

C_SOURCE = r'''
#include <stddef.h>
#include <stdio.h>
#include "limg_hip.h"

int main(void)
{
  static unsigned char stream[128];
  uint32_t out[4];
  limg_hip_window win = { 0, 0, 2, 2, NULL, 2 };
  limg_hip_window_job job = { NULL, sizeof stream, 8, 8, { 0, 0, 2, 2, NULL, 2 } };
  win.pOut = out;
  job.pStream = stream;
  job.window = win;
  if (sizeof(limg_hip_window) != 6 * sizeof(size_t)) return 1;
  if (sizeof(limg_hip_window_job) != 10 * sizeof(size_t)) return 2;
  if (offsetof(limg_hip_window, pOut) != 4 * sizeof(size_t) || offsetof(limg_hip_window_job, window) != 4 * sizeof(size_t)) return 3;
  if (limg_hip_decode_stream_windows_device(NULL, &job, 1, NULL, NULL) != limg_hip_error_ArgumentNull) return 10;
  if (limg_hip_blocked_decode_stream_windows_device(NULL, &job, 1, NULL, NULL) != limg_hip_error_ArgumentNull) return 11;
  if (limg_hip_decode_stream_windows(NULL, stream, sizeof stream, &win, 1) != limg_hip_error_ArgumentNull) return 12;
  if (limg_hip_blocked_decode_stream_windows(NULL, stream, sizeof stream, &win, 1) != limg_hip_error_ArgumentNull) return 13;
  puts("batched window decode entries ok");
  return 0;
}
'''

CPP_SOURCE = r'''
#include "limg_hip_shim.hpp"

typedef limg_result (*windows_fn)(const uint8_t *, const size_t, const limg_hip_window *, const size_t);

int main(int argc, char **)
{
  windows_fn fn = &limg_decode_windows;
  return fn != nullptr && argc > 0 ? 0 : 1;
}
'''


def _link_flags(lib):
    rocm_lib = os.environ.get("ROCM_LIB", "/opt/rocm/lib")
    return ["-L", os.path.dirname(lib), "-llimg_hip", "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath-link," + rocm_lib, "-Wl,-rpath," + rocm_lib]


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    from limg_amd import build
    return build.build(), tmp_path_factory.mktemp("c_abi_stream_windows")


def test_c_consumer_of_the_batched_window_entries(built):
    lib, d = built
    (d / "consumer.c").write_text(C_SOURCE)
    exe = d / "consumer"
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(d / "consumer.c"), "-o", str(exe)] + _link_flags(lib)
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, "the batched window decode entries of include/limg_hip.h do not work from C99:\n" + r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-500:])
    assert "batched window decode entries ok" in r.stdout


def test_shim_declares_limg_decode_windows(built):
    lib, d = built
    (d / "shim.cpp").write_text(CPP_SOURCE)
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(d / "shim.cpp"), "-o", str(d / "shim"), "-lpthread"] + _link_flags(lib)
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, "limg_decode_windows of include/limg_hip_shim.hpp does not compile and link:\n" + r.stderr[-3000:]
