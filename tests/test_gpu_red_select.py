"""The trial without the red-weight select (trial_pixel_error<.., NOSEL>, limg_hip_search.h), which a launch takes where red_select_dead (limg_hip_encode_rules.h)
holds for its pixel limit: errorFactor <= 1561.  Images of 512x64 (whole blocks) and 508x64 (partial blocks at the right edge: the table loop with masked lanes) of
uniform random bytes, photo-noise and crafted red steps, with and without alpha, at error factors on both sides of the rule's bound, through the persistent kernel and
the split path, default and accurate search, on the test build and on the product library: all 11 planes bit-identical to the oracle.

What the comparison rests on is checked on the CPU first (test_inputs_exercise_the_select, and the `wanted` fixture every GPU test takes): replayed with the oracle's
trial, the default search of these inputs executes trials with a pixel of dR^2 >= 0x4000 at an error factor <= 1561 -- the select that is dropped there would have
acted -- and, at error factors 1562, 1563 and 3000, trials whose verdict differs between the two weightings -- so a launch that took the select-free trial above the bound
would walk another path."""
import numpy as np
import pytest

import lib_axis as L
from lib_axis import lib, lib_product  # noqa: F401  (fixtures: "test" / "product")
import search_hot_inputs as inputs
from oracle.bind import PLANES

ERROR_FACTORS = (0, 100, 1560, 1561, 1562, 1563, 3000)
W, H = 512, 64


def red_steps(seed=5, blocks=(W // 8) * (H // 8)):
    """Per 8x8 block: red nearly flat with a few outliers a step above it, green and blue flat with a little noise.  With factor A at shift 8 the outliers' red
    difference is about the step while the other two stay small.  Upper half of the image: steps of 126..130, at the select's threshold of 128 -- the pixels on which
    the two weightings part at a pixel limit just above 0x8000 (errorFactor 1562, 1563).  Lower half: steps of 120..164 and more noise, for the larger limits."""
    narrow, wide = np.random.default_rng(seed), np.random.default_rng(seed + 1)
    img = np.zeros((H, W), dtype=np.uint32)
    for i in range(blocks):
        if i < blocks // 2:
            rng = narrow
            lo, step, k = int(rng.integers(0, 120)), int(rng.integers(126, 131)), int(rng.integers(1, 4))
            r = np.full(64, lo) + rng.integers(0, int(rng.integers(1, 3)), 64)
            r[rng.choice(64, k, replace=False)] = lo + step
            top, amp = 220, int(rng.integers(1, 30))
        else:
            rng = wide
            lo, step, k = int(rng.integers(0, 90)), int(rng.integers(120, 165)), int(rng.integers(1, 6))
            r = np.full(64, lo) + rng.integers(0, int(rng.integers(1, 40)), 64)
            r[rng.choice(64, k, replace=False)] = lo + step
            top, amp = 196, int(rng.integers(1, 60))
        g = int(rng.integers(0, top)) + rng.integers(0, amp, 64)
        b = int(rng.integers(0, top)) + rng.integers(0, amp, 64)
        by, bx = divmod(i, W // 8)
        img[by * 8:by * 8 + 8, bx * 8:bx * 8 + 8] = (r | (g << 8) | (b << 16) | (255 << 24)).astype(np.uint32).reshape(8, 8)
    return img


def images(oracle):
    """{name: 512x64 image}; the 508x64 ones are their left 508 columns"""
    return {"random_bytes": inputs.image(oracle, "random_bytes"), "photo_noise": inputs.image(oracle, "photo_noise"), "red_steps": red_steps()}


def select_statistics(oracle, img, ef, stop_at_high_red=False):
    """The default search of every whole block of `img` (4 channels) replayed with the oracle's trial -> (trials, trials with a pixel of dR^2 >= 0x4000, trials whose
    verdict differs between the weighting with the select and the one without).  The weighting with the select, restated here from the differences, must give the
    oracle's verdict for every trial."""
    from make_search_table import search_fast
    x = oracle.encode3d(img, True, planes=False, extras=True, error_factor=ef)
    max_pixel, max_block = 42 * (ef // 2), 28 * (ef // 2)
    trials = high = differ = 0

    def verdict(e):
        return not (e > max_pixel).any() and int(e.sum()) * 16 < max_block * 64

    for by in range(img.shape[0] // 8):
        for bx in range(img.shape[1] // 8):
            sl = (slice(by * 8, by * 8 + 8), slice(bx * 8, bx * 8 + 8))
            px = np.ascontiguousarray(img[sl]).ravel()
            rec = np.ascontiguousarray(x["records"][by, bx:bx + 1])
            fac = [np.ascontiguousarray(x[k][sl]).ravel() for k in ("preA", "preB", "preC")]
            g = search_fast()
            try:
                t = next(g)
                while True:
                    ok, _ = oracle.block_trial(px, 4, rec, fac[0], fac[1], fac[2], t, ef)
                    crushed = [f >> s if s < 8 else np.zeros_like(f) for f, s in zip(fac, t)]
                    est = oracle.block_decode(8, 8, 4, rec, crushed[0], crushed[1], crushed[2], t).ravel()
                    r2, g2, b2 = ((((px >> s) & 0xFF).astype(np.int64) - ((est >> s) & 0xFF).astype(np.int64)) ** 2 for s in (0, 8, 16))
                    with_select = np.where(r2 >= 0x4000, 3 * r2 + 4 * g2 + 2 * b2, 2 * r2 + 4 * g2 + 3 * b2)
                    assert verdict(with_select) == ok, (by, bx, t, ef)
                    trials += 1
                    high += int((r2 >= 0x4000).any())
                    differ += int(verdict(2 * r2 + 4 * g2 + 3 * b2) != ok)
                    if stop_at_high_red and high:
                        return trials, high, differ
                    t = g.send(ok)
            except StopIteration:
                pass
    return trials, high, differ


def check_inputs(oracle, imgs):
    _, high, _ = select_statistics(oracle, imgs["random_bytes"], 100, stop_at_high_red=True)
    assert high > 0, "no executed trial with dR^2 >= 0x4000 at errorFactor 100: the dropped select would never have acted"
    for ef in (1562, 1563, 3000):
        trials, _, differ = select_statistics(oracle, imgs["red_steps"], ef)
        assert differ > 0, "errorFactor %d: none of %d executed trials depends on the select: a wrong dispatch would go unseen" % (ef, trials)


def test_inputs_exercise_the_select(oracle):
    check_inputs(oracle, images(oracle))


@pytest.fixture(scope="module")
def wanted(oracle):
    """{accurate: [(name, image, has_alpha, errorFactor, the oracle's planes)]}, computed once for both paths and both libraries -- after the inputs' own check"""
    imgs = images(oracle)
    check_inputs(oracle, imgs)
    out = {False: [], True: []}
    for accurate in out:
        for kind, full in imgs.items():
            for img in (full, np.ascontiguousarray(full[:, :508])):
                for alpha in (True, False):
                    for ef in ERROR_FACTORS:
                        name = "%s %dx%d alpha=%s errorFactor %d %s" % (kind, img.shape[1], img.shape[0], alpha, ef, "accurate" if accurate else "default")
                        out[accurate].append((name, img, alpha, ef, oracle.encode3d(img, alpha, error_factor=ef, fast=not accurate)))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("search", ["default", "accurate"])
@pytest.mark.parametrize("mode", ["persistent", "split"])
def test_both_sides_of_the_bound_are_bit_identical_to_the_oracle(lib, wanted, mode, search):
    g = L.open_context(lib)
    try:
        g.set_options(force_split=(mode == "split"))
        for name, img, alpha, ef, want in wanted[search == "accurate"]:
            got = g.encode3d(img, alpha, error_factor=ef, fast=(search == "default"))
            bad = [(k, int((got[k] != want[k]).sum())) for k in PLANES if not np.array_equal(got[k], want[k])]
            assert len(PLANES) == 11 and not bad, (name, mode, bad)
        g.check()
    finally:
        g.close()


L.product_twins(globals())
