"""Completeness of the library axis (tests/lib_axis.py), without a GPU: every GPU test that encodes in this process has a product twin (<name>_product, the same
parameter ids), unless lib_axis names it -- HOOK_ONLY (about a test hook as a whole) or NO_AXIS (programs that load the product themselves) -- and those lists name only
tests that exist."""
import os
import re
import subprocess
import sys

import lib_axis as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gpu_test_ids():
    """{(module file, test function): [parameter ids]} of the tests `-m gpu` selects, as pytest collects them"""
    r = subprocess.run([sys.executable, "-m", "pytest", "tests", "-q", "-m", "gpu", "--collect-only", "-p", "no:cacheprovider"], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    out = {}
    for line in r.stdout.splitlines():
        m = re.match(r"^tests/(test_\w+\.py)::(\w+)(?:\[(.*)\])?$", line.strip())
        if m:
            out.setdefault((m.group(1), m.group(2)), []).append(m.group(3) or "")
    assert len(out) > 50, r.stdout[-2000:]
    return out


def test_every_gpu_test_runs_on_the_product_or_is_listed():
    tests = _gpu_test_ids()
    missing = []
    for (mod, name), ids in sorted(tests.items()):
        if name.endswith(L.TWIN_SUFFIX):
            assert (mod, name[:-len(L.TWIN_SUFFIX)]) in tests, (mod, name, "a product twin without its test-build test")
            continue
        key = "%s::%s" % (mod, name)
        twin = tests.get((mod, name + L.TWIN_SUFFIX))
        if key in L.HOOK_ONLY or key in L.NO_AXIS or mod in L.NO_AXIS:
            assert twin is None, (key, "listed as test-build only / without the axis, yet it has a product twin")
        elif twin is None:
            missing.append(key)
        else:
            assert sorted(twin) == sorted(ids), (key, "the product twin runs other parameters", sorted(set(twin) ^ set(ids))[:8])
    assert not missing, "GPU tests without a product twin (take a context argument of lib_axis.AXIS_ARGS, or list them in tests/lib_axis.py with a reason): %s" % missing


def test_the_lists_name_existing_tests():
    tests = _gpu_test_ids()
    keys = {"%s::%s" % k for k in tests}
    mods = {m for m, _ in tests}
    stale = [k for k in L.HOOK_ONLY if k not in keys]
    stale += [k for k in L.NO_AXIS if k not in keys and k not in mods]
    assert not stale, "tests/lib_axis.py names GPU tests that do not exist: %s" % stale
    assert all(r.strip() for r in list(L.HOOK_ONLY.values()) + list(L.NO_AXIS.values()))


def test_twins_open_the_product():
    """the twin hands its body the product's fixture: lib_axis swaps exactly the context arguments"""
    ns = {"__file__": "test_x.py"}

    def test_y(oracle, lib, w):
        return lib, w
    ns["test_y"] = test_y
    L.product_twins(ns)
    import inspect
    assert list(inspect.signature(ns["test_y_product"]).parameters) == ["oracle", "lib_product", "w"]
    assert ns["test_y_product"](oracle=None, lib_product="product", w=3) == ("product", 3)
