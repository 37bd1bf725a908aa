"""The lists of mixed shapes that the tests of the budgeted list and the sizes list share (tests/test_gpu_stream_budget_list.py, tests/test_gpu_stream_sizes_list.py):
the smallest shapes that reach each way the list probe can go wrong, and the image of an index.  Not a test module."""

SMALL = ((264, 24), (8, 8), (256, 8), (24, 40), (512, 32))  # the five shapes `sixty_six` cycles through
# name: (alpha, shapes (w, h), encode arguments)
LISTS = {
    "edges": (True, ((264, 24), (8, 8), (256, 8), (520, 16), (8, 512), (24, 40), (512, 32)), {}),
    "one_strip_each": (True, ((256, 8), (8, 8), (248, 8), (16, 8), (256, 8)), {}),
    "rgb": (False, ((512, 32), (40, 24), (264, 8)), {}),
    "sixty_six": (True, tuple(SMALL[i % 5] for i in range(66)), {}),
    "ragged_inside": (True, ((264, 24), (13, 9), (256, 20), (8, 8)), {}),
    "pool": (True, ((128, 256), (64, 24), (8, 8), (256, 40)), {"pool_threads": 2}),
}


def image(oracle, w, h, i):
    """photo-noise and random-gradient (varying alpha) images alternate, as in tests/test_gpu_stream_list.py"""
    return oracle.photo_noise(w, h, 3 + 2 * (i % 8)) if i % 2 == 0 else oracle.random_gradient(w, h, 3 + 2 * (i % 8), False)
