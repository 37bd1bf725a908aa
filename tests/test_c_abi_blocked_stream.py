"""The version 2 stream declarations of include/limg_hip.h from C99: a C program includes the header, links against liblimg_hip.so and calls the host-only entries
limg_hip_blocked_stream_bound / limg_hip_blocked_stream_info -- no device is touched, so this runs everywhere."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

C_SOURCE = r'''
#include <stdio.h>
#include <string.h>
#include "limg_hip.h"

int main(void)
{
  struct limg_hip_stream_header h;
  unsigned char buf[sizeof h];
  size_t sx = 0, sy = 0, total = 0, rects = 0;
  int alpha = -1;
  if (sizeof(struct limg_hip_stream_header) != 64 || sizeof(struct limg_hip_stream_rect) != 64) return 10;
  if (limg_hip_blocked_stream_bound(24, 16) != 64 + 6 * 64 + 6 * 192) return 11;
  if (limg_hip_blocked_stream_bound(0, 16) != 0 || limg_hip_blocked_stream_bound(8 * 65536ul, 8) != 0) return 12;
  memset(&h, 0, sizeof h);
  h.magic = LIMG_HIP_STREAM_MAGIC; h.version = LIMG_HIP_STREAM_VERSION_BLOCKED;
  h.sizeX = 24; h.sizeY = 16; h.channels = 3; h.errorFactor = 100; h.blocksX = 3; h.blocksY = 2;
  h.payloadWords = 7; h.flags = 1u | LIMG_HIP_STREAM_FLAG_MERGED;
  h.reserved[LIMG_HIP_STREAM_RESERVED_RECTANGLES] = 2;
  h.totalBytes = sizeof h + 2 * sizeof(struct limg_hip_stream_rect) + 7 * 8;
  memcpy(buf, &h, sizeof h);
  if (limg_hip_blocked_stream_info(buf, sizeof buf, &sx, &sy, &alpha, &total, &rects) != limg_hip_success) return 13;
  if (sx != 24 || sy != 16 || alpha != 0 || total != 64 + 128 + 56 || rects != 2) return 14;
  if (limg_hip_stream_info(buf, sizeof buf, &sx, &sy, &alpha, &total) != limg_hip_error_InvalidParameter) return 15; /* version 1's check refuses version 2 */
  if (limg_hip_blocked_stream_info(buf, sizeof buf - 1, NULL, NULL, NULL, NULL, NULL) != limg_hip_error_OutOfBounds) return 16;
  h.reserved[LIMG_HIP_STREAM_RESERVED_RECTANGLES] = 7; /* more rectangles than blocks */
  memcpy(buf, &h, sizeof h);
  if (limg_hip_blocked_stream_info(buf, sizeof buf, NULL, NULL, NULL, NULL, NULL) != limg_hip_error_InvalidParameter) return 17;
  if (limg_hip_blocked_stream_info(NULL, 64, NULL, NULL, NULL, NULL, NULL) != limg_hip_error_ArgumentNull) return 18;
  printf("version 2 header ok: %lu bytes, %lu rectangles\n", (unsigned long)total, (unsigned long)rects);
  return 0;
}
'''


@pytest.fixture(scope="module")
def c_program(tmp_path_factory):
    from limg_amd import build
    lib = build.build()
    d = tmp_path_factory.mktemp("c_abi_blocked_stream")
    (d / "consumer.c").write_text(C_SOURCE)
    exe = d / "consumer"
    rocm_lib = os.environ.get("ROCM_LIB", "/opt/rocm/lib")
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(d / "consumer.c"), "-o", str(exe),
           "-L", os.path.dirname(lib), "-llimg_hip", "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath-link," + rocm_lib, "-Wl,-rpath," + rocm_lib]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, "include/limg_hip.h does not work from C99:\n" + r.stderr[-3000:]
    return str(exe)


def test_c_consumer_of_the_version_2_header(c_program):
    r = subprocess.run([c_program], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-500:])
    assert "version 2 header ok: 248 bytes, 2 rectangles" in r.stdout
