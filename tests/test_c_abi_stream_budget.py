"""The size probe and budget entries of include/limg_hip.h from C99, without a GPU: a C program includes the header, prints the layout of limg_hip_budget_result, links
against the library and calls the four entries with a NULL context -- limg_hip_error_ArgumentNull comes back before anything touches a device.  Both libraries export
the four names, the Python struct has the header's layout, and a C++ translation unit that includes the shim takes the address of limg_encode_budget: it compiles and
links, and is not run."""
import ctypes as C
import os
import subprocess

import pytest

import limg_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("limg_hip_stream_sizes_device", "limg_hip_stream_sizes", "limg_hip_encode_stream_budget_device", "limg_hip_encode_stream_budget")

C_SOURCE = r'''
#include <stddef.h>
#include <stdio.h>
#include "limg_hip.h"

int main(void)
{
  static uint32_t px[64];
  static unsigned char stream[4096];
  const uint32_t efs[2] = { 0, 100 };
  size_t sizes[2] = { 0, 0 };
  limg_hip_budget_result res = { sizeof(limg_hip_budget_result), 7, 7, 7, 7 };
  if (limg_hip_stream_sizes_device(NULL, px, 8, 8, 1, efs, 2, sizes, 0, 1, NULL) != limg_hip_error_ArgumentNull) return 10;
  if (limg_hip_stream_sizes(NULL, px, 8, 8, 1, efs, 2, sizes, 0, 1) != limg_hip_error_ArgumentNull) return 11;
  if (limg_hip_encode_stream_budget_device(NULL, px, 8, 8, 1, stream, sizeof stream, 1000, 0, 0, 0, 1, &res, NULL) != limg_hip_error_ArgumentNull) return 12;
  if (limg_hip_encode_stream_budget(NULL, px, 8, 8, 1, stream, sizeof stream, 1000, 0, 0, 0, 1, &res) != limg_hip_error_ArgumentNull) return 13;
  if (res.errorFactor != 7 || res.probes != 7 || res.withinBudget != 7 || res.bytes != 7 || sizes[0] || sizes[1]) return 14; /* a refused call writes nothing */
  printf("layout %lu %lu %lu %lu %lu %lu\n", (unsigned long)sizeof(limg_hip_budget_result), (unsigned long)offsetof(limg_hip_budget_result, struct_size),
         (unsigned long)offsetof(limg_hip_budget_result, errorFactor), (unsigned long)offsetof(limg_hip_budget_result, probes),
         (unsigned long)offsetof(limg_hip_budget_result, withinBudget), (unsigned long)offsetof(limg_hip_budget_result, bytes));
  return 0;
}
'''

CPP_SOURCE = r'''
#include "limg_hip_shim.hpp"

typedef limg_result (*budget_fn)(const uint32_t *, const size_t, const size_t, const bool, uint8_t *, const size_t, size_t *, const size_t, uint32_t *, bool *, uint32_t *,
                                 const uint32_t, const uint32_t, limg_thread_pool *, const bool);

int main(int argc, char **)
{
  budget_fn a = &limg_encode_budget;
  return a != nullptr && argc > 0 ? 0 : 1;
}
'''


def _link_flags(lib):
    rocm_lib = os.environ.get("ROCM_LIB", "/opt/rocm/lib")
    return ["-L", os.path.dirname(lib), "-llimg_hip", "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath-link," + rocm_lib, "-Wl,-rpath," + rocm_lib]


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    from limg_amd import build
    return build.build(), build.build(test_hooks=True), tmp_path_factory.mktemp("c_abi_stream_budget")


def test_c_consumer_and_the_result_structs_layout(built):
    lib, _, d = built
    (d / "consumer.c").write_text(C_SOURCE)
    exe = d / "consumer"
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(d / "consumer.c"), "-o", str(exe)] + _link_flags(lib)
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, "the budget entries of include/limg_hip.h do not work from C99:\n" + r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-500:])
    B = limg_amd.BudgetResult
    want = [C.sizeof(B)] + [getattr(B, f).offset for f in ("struct_size", "errorFactor", "probes", "withinBudget", "bytes")]
    assert [int(v) for v in r.stdout.split()[1:]] == want == [24, 0, 4, 8, 12, 16], (r.stdout, want)


def test_shim_has_limg_encode_budget(built):
    lib, _, d = built
    (d / "shim.cpp").write_text(CPP_SOURCE)
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(d / "shim.cpp"), "-o", str(d / "shim"), "-lpthread"] + _link_flags(lib)
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def test_both_libraries_export_the_four_names(built):
    for lib in built[:2]:
        defined = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
        for name in NAMES:
            assert (" T " + name + "\n") in defined, (lib, name)
    assert set(NAMES) <= set(limg_amd.ABI_SYMBOLS)
    for name in ("stream_sizes", "stream_sizes_device", "encode_stream_budget", "encode_stream_budget_device"):
        assert callable(getattr(limg_amd.LimgHip, name))
