"""The budgeted list entries of include/limg_hip.h from C99, without a GPU: a C program includes the header, links against the library and calls the two entries with
a NULL context and with NULL arrays -- limg_hip_error_ArgumentNull comes back before anything touches a device, and nothing is written.  Both libraries export the two
names and nothing else new, Python has the two methods, and a C++ translation unit that includes the shim takes the address of limg_encode_budget_batch: it compiles
and links, and is not run."""
import os
import subprocess

import pytest

import limg_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("limg_hip_encode_stream_budget_batch_device", "limg_hip_encode_stream_budget_batch")

C_SOURCE = r'''
#include <stddef.h>
#include <stdio.h>
#include "limg_hip.h"

int main(void)
{
  static uint32_t px[2][64];
  static unsigned char stream[2][4096];
  const uint32_t *ins[2] = { px[0], px[1] };
  uint8_t *outs[2] = { stream[0], stream[1] };
  const size_t budgets[2] = { 1000, 2000 };
  limg_hip_budget_result res[2] = { { sizeof(limg_hip_budget_result), 7, 7, 7, 7 }, { sizeof(limg_hip_budget_result), 7, 7, 7, 7 } };
  int i;
  if (limg_hip_encode_stream_budget_batch_device(NULL, 2, ins, 8, 8, 1, outs, sizeof stream[0], budgets, 0, 0, 0, 1, res, NULL) != limg_hip_error_ArgumentNull) return 10;
  if (limg_hip_encode_stream_budget_batch(NULL, 2, ins, 8, 8, 1, outs, sizeof stream[0], budgets, 0, 0, 0, 1, res) != limg_hip_error_ArgumentNull) return 11;
  if (limg_hip_encode_stream_budget_batch_device(NULL, 0, NULL, 8, 8, 1, NULL, 0, NULL, 0, 0, 0, 1, NULL, NULL) != limg_hip_error_ArgumentNull) return 12;
  if (limg_hip_encode_stream_budget_batch(NULL, 0, NULL, 8, 8, 1, NULL, 0, NULL, 0, 0, 0, 1, NULL) != limg_hip_error_ArgumentNull) return 13;
  for (i = 0; i < 2; i++)
    if (res[i].errorFactor != 7 || res[i].probes != 7 || res[i].withinBudget != 7 || res[i].bytes != 7 || stream[i][0]) return 14; /* a refused call writes nothing */
  printf("ok\n");
  return 0;
}
'''

CPP_SOURCE = r'''
#include "limg_hip_shim.hpp"

typedef limg_result (*budget_batch_fn)(const uint32_t *const *, const size_t, const size_t, const size_t, const bool, uint8_t *const *, const size_t, size_t *, const size_t *,
                                       uint32_t *, bool *, uint32_t *, const uint32_t, const uint32_t, limg_thread_pool *, const bool);

int main(int argc, char **)
{
  budget_batch_fn a = &limg_encode_budget_batch;
  return a != nullptr && argc > 0 ? 0 : 1;
}
'''


def _link_flags(lib):
    rocm_lib = os.environ.get("ROCM_LIB", "/opt/rocm/lib")
    return ["-L", os.path.dirname(lib), "-llimg_hip", "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath-link," + rocm_lib, "-Wl,-rpath," + rocm_lib]


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    from limg_amd import build
    return build.build(), build.build(test_hooks=True), tmp_path_factory.mktemp("c_abi_stream_budget_batch")


def test_c_consumer(built):
    lib, _, d = built
    (d / "consumer.c").write_text(C_SOURCE)
    exe = d / "consumer"
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(d / "consumer.c"), "-o", str(exe)] + _link_flags(lib)
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, "the budgeted list entries of include/limg_hip.h do not work from C99:\n" + r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.split() == ["ok"], (r.returncode, r.stdout, r.stderr[-500:])


def test_shim_has_limg_encode_budget_batch(built):
    lib, _, d = built
    (d / "shim.cpp").write_text(CPP_SOURCE)
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(d / "shim.cpp"), "-o", str(d / "shim"), "-lpthread"] + _link_flags(lib)
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def test_both_libraries_export_the_two_names_and_nothing_else_new(built):
    """every exported limg_hip_* name is one the header declares (limg_amd.ABI_SYMBOLS; the test build: plus its hooks), the two new ones among them"""
    for lib, allowed in zip(built[:2], (set(limg_amd.ABI_SYMBOLS), set(limg_amd.ABI_SYMBOLS) | set(limg_amd.TEST_ABI_SYMBOLS))):
        out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
        exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
        for name in NAMES:
            assert name in exported, (lib, name)
        assert exported <= allowed, (lib, sorted(exported - allowed))
    assert len(set(limg_amd.ABI_SYMBOLS)) == len(limg_amd.ABI_SYMBOLS)
    header = open(os.path.join(ROOT, "include", "limg_hip.h")).read()
    for name in NAMES:
        assert header.count(name + "(") == 1, name
    for name in ("encode_stream_budget_batch", "encode_stream_budget_batch_device"):
        assert callable(getattr(limg_amd.LimgHip, name))
