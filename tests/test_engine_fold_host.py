"""Host-side gate of the engine's Adam fold (no GPU needed, the built
extension is enough): a wgrad launch may carry an Adam step only if its
dW/db slices tile the flat gradient buffer exactly once."""

import pytest


@pytest.fixture(scope="module")
def tiles():
    from torch_actor_critic_amd.ops import require_extension
    return require_extension().ranges_tile_exactly


def test_ranges_tile_exactly(tiles):
    # w|b slices of two layers, given out of order
    assert tiles([(6, 2), (0, 6), (8, 12), (20, 3)], 23)
    assert tiles([(0, 5), (5, 0), (5, 1)], 6)              # empty bias
    assert not tiles([(0, 6), (8, 12), (20, 3)], 23)       # hole
    assert not tiles([(0, 6), (5, 3), (8, 15)], 23)        # overlap
    assert not tiles([(0, 6), (0, 6), (6, 17)], 23)        # doubled
    assert not tiles([(0, 6), (6, 2)], 23)                 # tail missing
    assert not tiles([(1, 22)], 23)                        # head missing
    assert not tiles([(0, 24)], 23)                        # overrun
    assert not tiles([(-2, 25)], 23)
    assert not tiles([], 23)


def test_split_query_follows_the_compute_dtype():
    """The engine's default folds Adam only where the wgrad launch splits
    along M; the launcher answers that for the current compute dtype."""
    from torch_actor_critic_amd.ops import functional as Fo
    from torch_actor_critic_amd.ops import require_extension
    ext = require_extension()
    # flagship critic phase at batch 64: 48 tiles
    Ns = [256, 256, 256, 256, 1, 1]
    Ks = [23, 23, 256, 256, 256, 256]
    try:
        Fo.set_compute_dtype("bf16")      # 64-row K-step: one chunk
        assert ext.mwgrad_het_adam_split([64] * 6, Ns, Ks) == 1
        assert ext.mwgrad_het_adam_split([4096] * 6, Ns, Ks) > 1
        Fo.set_compute_dtype("fp32")      # 16-row K-step: four chunks
        assert ext.mwgrad_het_adam_split([64] * 6, Ns, Ks) == 4
        # >= 384 tiles never split, whatever M
        assert ext.mwgrad_het_adam_split([4096] * 12, [256] * 12,
                                         [512] * 12) == 1
    finally:
        Fo.set_compute_dtype("fp32")
