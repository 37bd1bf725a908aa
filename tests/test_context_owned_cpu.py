"""limg_amd/csrc/limg_hip_owned.h -- the types through which a context owns its device buffers, pinned buffers, streams and events -- without a GPU:
tests/helpers/owned_check.cpp defines the HIP entry points the header calls on top of malloc / free (with a switch that makes the next calls fail) and checks growth,
failed allocations, failed event / stream creation, the device-byte total and that every scope gives back all it took.  Built with AddressSanitizer (LeakSanitizer
with it) and UBSan as a stand-alone program: no HIP runtime is linked, nothing is preloaded."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "helpers", "owned_check.cpp")
ROCM_INCLUDE = os.environ.get("ROCM_INCLUDE", "/opt/rocm/include")


def test_owned_types_release_what_they_take(tmp_path):
    gxx = shutil.which("g++")
    if not gxx or not os.path.exists(os.path.join(ROCM_INCLUDE, "hip", "hip_runtime_api.h")):
        pytest.skip("needs g++ and the ROCm headers")
    exe = str(tmp_path / "owned_check")
    subprocess.check_call([gxx, "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + ROCM_INCLUDE, "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", "-Wall",
                           "-static-libasan", "-static-libubsan", SRC, "-o", exe])  # (the runtimes inside the program: it does not matter what else the loader brings)
    r = subprocess.run([exe], env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, r.stdout
    assert "owned_check ok" in r.stdout, r.stdout
