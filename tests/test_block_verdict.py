"""The stored verdict-edge blocks (tests/golden/block_verdict_blocks.npz, tests/block_verdict_inputs.py) still are what tests/test_gpu_block_verdict.py needs them to be:
tiled into their images, every block has a trial that the default search really runs whose block sum is exactly blockLimit - 1 (and passes) or exactly blockLimit (and
fails) -- with the CPU oracle alone.  CPU only."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import block_verdict_inputs as inputs  # noqa: E402


def test_the_file_holds_enough_blocks_of_each_kind():
    px, efs, kinds = inputs.stored_blocks()
    assert px.shape == (len(efs), 64) and len(kinds) == len(efs)
    assert int((kinds == inputs.BELOW).sum()) >= 8 and int((kinds == inputs.AT).sum()) >= 8
    both = [ef for ef in set(efs.tolist()) if {inputs.BELOW, inputs.AT} <= set(kinds[efs == ef].tolist())]
    assert len(both) >= 2, both
    assert os.path.getsize(inputs.GOLDEN) < 64 * 1024


def test_block_limit_is_the_smallest_failing_sum():
    for ef in (0, 1, 2, 25, 50, 100, 400):
        max_block = 4 * (ef // 2) * 7
        lim = inputs.block_limit(ef)
        assert lim * 16 >= max_block * 64 and (lim == 0 or (lim - 1) * 16 < max_block * 64)


def test_every_stored_block_has_its_edge_trial(oracle):
    images = inputs.edge_images()
    assert len(images) >= 2
    for img, ef, kinds in images:
        assert img.shape == (8, 8 * len(kinds))
        found = inputs.edge_trials(oracle, img, ef)
        for i, kind in enumerate(kinds):
            assert kind in found.get((0, i), ()), (ef, i, kind, found.get((0, i)))
