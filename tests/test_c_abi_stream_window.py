"""The window decode declarations of include/limg_hip.h from C99: a C program includes the header, links against liblimg_hip.so and calls the four entries with a
NULL context -- limg_hip_error_ArgumentNull comes back before anything touches a device, so this runs everywhere."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

C_SOURCE = r'''
#include <stdio.h>
#include "limg_hip.h"

int main(void)
{
  static unsigned char stream[128];
  uint32_t out[4];
  if (limg_hip_decode_stream_window_device(NULL, stream, sizeof stream, 8, 8, 0, 0, 2, 2, out, 2, NULL) != limg_hip_error_ArgumentNull) return 10;
  if (limg_hip_blocked_decode_stream_window_device(NULL, stream, sizeof stream, 8, 8, 0, 0, 2, 2, out, 2, NULL) != limg_hip_error_ArgumentNull) return 11;
  if (limg_hip_decode_stream_window(NULL, stream, sizeof stream, 0, 0, 2, 2, out, 2) != limg_hip_error_ArgumentNull) return 12;
  if (limg_hip_blocked_decode_stream_window(NULL, stream, sizeof stream, 0, 0, 2, 2, out, 2) != limg_hip_error_ArgumentNull) return 13;
  puts("window decode entries ok");
  return 0;
}
'''


@pytest.fixture(scope="module")
def c_program(tmp_path_factory):
    from limg_amd import build
    lib = build.build()
    d = tmp_path_factory.mktemp("c_abi_stream_window")
    (d / "consumer.c").write_text(C_SOURCE)
    exe = d / "consumer"
    rocm_lib = os.environ.get("ROCM_LIB", "/opt/rocm/lib")
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(d / "consumer.c"), "-o", str(exe),
           "-L", os.path.dirname(lib), "-llimg_hip", "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath-link," + rocm_lib, "-Wl,-rpath," + rocm_lib]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, "the window decode entries of include/limg_hip.h do not work from C99:\n" + r.stderr[-3000:]
    return str(exe)


def test_c_consumer_of_the_window_entries(c_program):
    r = subprocess.run([c_program], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-500:])
    assert "window decode entries ok" in r.stdout
