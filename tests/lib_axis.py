"""The library axis of the in-process GPU suite.  The build makes two libraries from one source tree: the PRODUCT (limg_amd/liblimg_hip.so: what bench.py, the shim,
the CLI and smoke() load) and the TEST build (limg_amd/liblimg_hip_test.so, -DLIMG_HIP_TEST_HOOKS: the same sources plus the hooks of include/limg_hip_test_hooks.h).
Every kernel that takes EncodeParams is a separate code object in each (tests/test_product_library.py pins which), so a test that encodes in-process runs on both.

A GPU test reaches its library through one of the context arguments of AXIS_ARGS: the module's context fixture (`gpu`, or `ctxs`) or `lib` ("test" / "product", for
tests that open their contexts in the body; the fixtures `lib` / `lib_product` below).  As before, those give the test build.  A module ends with
`L.product_twins(globals())`: every such test gets a twin `<name>_product` -- same body, same parameters and ids -- that takes `gpu_product` / `ctxs_product` /
`lib_product` instead: the module defines its context fixture twice, through open_context("test") and open_context("product").  So the test build's test ids stay what
they were and the product's read test_x_product[...].  A test wholly about a hook gets no twin: it is on HOOK_ONLY below.  A test that needs a hook for one leg of several
runs that leg where has_hooks(context) holds -- on the test build exactly what it asserted before, on the product every other leg."""
import inspect
import os

import pytest

import limg_amd

PRODUCT = os.path.join(limg_amd.HERE, "liblimg_hip.so")
TEST = limg_amd.TEST_LIB_PATH
LIBS = ("test", "product")
PATHS = {"test": TEST, "product": PRODUCT}
AXIS_ARGS = ("gpu", "ctxs", "lib")  # the arguments through which a test gets its library; the product twin takes <arg>_product
TWIN_SUFFIX = "_product"

# GPU tests that run on the test build only: each one is about a hook of include/limg_hip_test_hooks.h as a whole (the product has none to set).
HOOK_ONLY = {
    "test_gpu_parity.py::test_generic_trial_path": "record_limit hook: sends blocks through the generic 32-bit trial, which byte pixels never reach",
    "test_gpu_search_tables.py::test_generic_trial_accurate": "record_limit hook: the accurate search's literal loops behind the generic 32-bit trial",
    "test_gpu_concurrency.py::test_lookback_timeout_is_loud": "lookback_spins / skip_publish_strip hooks: a strip that never publishes",
    "test_gpu_fullsize.py::test_one_strip_base_error_is_caught": "base_error_strip hook: the sensitivity of the hash pin to one wrong chain base",
    "test_gpu_blocked.py::test_similarity_bits_equal_host_evaluation_with_and_without_the_bound": "blocked_no_bound hook: A/B of the match kernel's bounds",
    "test_gpu_blocked.py::test_large_first_order_and_vector_stores_change_nothing": "blocked_no_order / blocked_no_vec_store hooks: A/B of the store ordering",
    "test_gpu_context_resources.py::test_every_family_then_close": "limg_hip_test_live_resources hook: the counts of live GPU resources, which the product does not keep",
    "test_gpu_context_resources.py::test_two_contexts": "limg_hip_test_live_resources hook: the counts of live GPU resources, which the product does not keep",
    "test_gpu_context_resources.py::test_unused_context": "limg_hip_test_live_resources hook: the counts of live GPU resources, which the product does not keep",
    "test_gpu_context_resources.py::test_open_encode_close_cycles": "limg_hip_test_live_resources hook: the counts of live GPU resources, which the product does not keep",
}

# GPU tests without the axis because they do not encode in this process on a library of their choosing: they start programs that load the product themselves, or
# they are the product's own checks.  The completeness guard (tests/test_lib_axis.py) accepts these and nothing else without a product twin.
NO_AXIS = {
    "test_gpu_collective.py::test_rccl_two_ranks": "rank scripts load the test build on purpose (abort-rule hook) and need two GPUs",
    "test_gpu_ref_main.py": "the reference's main linked to the shim: a program that loads the product",
    "test_gpu_rehearsal.py": "bench.py rank processes: they load the product",
    "test_product_library.py": "the product library's own checks",
    "test_gpu_library_identity.py": "every test runs the product and the test build side by side",
    "test_c_abi.py": "a C program linked to the product",
    "test_cli.py": "the CLI: a program that loads the product",
    "test_shim_ref_main.py": "the shim: programs that load the product",
    "test_shim_threads.py": "the shim: programs that load the product",
}


def open_context(lib, device=0):
    """A context on `lib` ("test" / "product") -- refuses to hand out the other build."""
    g = limg_amd.LimgHip(device, lib_path=PATHS[lib])
    assert g.has_test_hooks == (lib == "test"), (lib, PATHS[lib], g.has_test_hooks)
    g.library = lib
    return g


def has_hooks(g):
    """True where a leg that needs a test hook runs: contexts on the test build."""
    return g.has_test_hooks


@pytest.fixture
def lib():
    return "test"


@pytest.fixture
def lib_product():
    return "product"


def _twin(fn, name):
    sig = inspect.signature(fn)
    swap = {a: a + TWIN_SUFFIX for a in AXIS_ARGS if a in sig.parameters}

    def twin(**kw):
        for a, b in swap.items():
            kw[a] = kw.pop(b)
        return fn(**kw)
    twin.__name__ = twin.__qualname__ = name
    twin.__module__ = fn.__module__
    twin.__doc__ = fn.__doc__
    twin.__signature__ = sig.replace(parameters=[p.replace(name=swap.get(p.name, p.name)) for p in sig.parameters.values()])
    if hasattr(fn, "pytestmark"):
        twin.pytestmark = list(fn.pytestmark)  # the parametrisation, and with it the ids
    return twin


def product_twins(ns):
    """Add `<name>_product` to a test module's namespace for every test that takes a context argument (AXIS_ARGS) and is not on HOOK_ONLY."""
    module = os.path.basename(ns["__file__"])
    for name, fn in list(ns.items()):
        if not (name.startswith("test_") and inspect.isfunction(fn)) or name.endswith(TWIN_SUFFIX) or "%s::%s" % (module, name) in HOOK_ONLY:
            continue
        if any(a in inspect.signature(fn).parameters for a in AXIS_ARGS):
            assert name + TWIN_SUFFIX not in ns, name
            ns[name + TWIN_SUFFIX] = _twin(fn, name + TWIN_SUFFIX)
