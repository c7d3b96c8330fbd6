"""CPU: the occlusion-robustness test's instance mask (reference utils/func.py:14-40 random_mask_square_instance, drawn by the
dataset in __getitem__: dataset/PatchWSI.py:80-81) -- advmil_amd.utils.func.square_instance_keep / random_mask_square_instance
against kept sets recorded from the reference itself (tests/golden/gen_golden_mask.py -> mask_v1.npz), and the argument checks of
the staging entry point that applies the mask on the device (advmil_stage_bag_masked rejects before any launch: no GPU needed)."""
import ctypes
import os

import numpy as np
import pytest
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mask_v1.npz")
EINVAL = -1
A16 = 0x7F0000001000          # a fake, 16-byte aligned "device address": never dereferenced when validation does its job


@pytest.fixture(scope="module")
def gold():
    g = np.load(GOLD)
    return {k: g[k] for k in g.files}


def cases(gold):
    return [(int(n), float(r), gold[f"keep_{i}"]) for i, (n, r) in enumerate(zip(gold["rows"], gold["ratio"]))]


def test_square_instance_keep_reproduces_the_reference_draws(gold):
    """One stream of the global np.random under the fixture's seed: the same kept sets, bag after bag, and the same next draw behind
    them (the amount of RNG consumed). 160 rows at 0.8 keep ONE region: 10 * (1 - 0.8) is 1.9999999999999996."""
    from advmil_amd.utils.func import square_instance_keep
    np.random.seed(int(gold["seed"]))
    for n, ratio, want in cases(gold):
        got = square_instance_keep(n, ratio)
        assert got.dtype == np.int64 and np.array_equal(got, want), (n, ratio, got, want)
        assert np.all(np.diff(got) > 0) and got.min() >= 0 and got.max() < n // 16
    assert int(np.random.randint(1 << 30)) == int(gold["next_draw"])
    by = {(n, r): k for n, r, k in cases(gold)}
    assert len(by[(160, .8)]) == 1 and len(by[(48, 1.0)]) == 1 and len(by[(48, .999)]) == 1 and len(by[(8192, .5)]) == 256


def test_square_instance_keep_draws_from_a_given_random_state(gold):
    """rng=RandomState(seed): the same sets, and the global stream is left alone."""
    from advmil_amd.utils.func import square_instance_keep
    rng = np.random.RandomState(int(gold["seed"]))
    np.random.seed(123)
    before = np.random.get_state()
    for n, ratio, want in cases(gold):
        assert np.array_equal(square_instance_keep(n, ratio, rng=rng), want)
    assert int(rng.randint(1 << 30)) == int(gold["next_draw"])
    after = np.random.get_state()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]


@pytest.mark.parametrize("way", ["mask_zero", "discard"])
def test_random_mask_square_instance_matches_the_reference_rows(gold, way):
    """Host tensors [N, 8] through the reference-signature function under the fixture's seed: bit for bit the bag with every region
    outside the recorded kept set zeroed (mask_zero) / the kept rows alone (discard)."""
    from advmil_amd.utils.func import random_mask_square_instance
    g = torch.Generator().manual_seed(5)
    np.random.seed(int(gold["seed"]))
    for n, ratio, keep in cases(gold):
        bag = torch.randn(n, 8, generator=g)
        bag[::7] = -0.0                                                       # (signed zeros survive as they are in kept rows)
        rows = (torch.from_numpy(keep).reshape(-1, 1) * 16 + torch.arange(16).reshape(1, -1)).reshape(-1)
        got = random_mask_square_instance(bag, ratio, scale=4, mask_way=way)
        if way == "discard":
            want = bag[rows]
        else:
            want = torch.zeros(n, 8)
            want[rows] = bag[rows]
        assert got is not bag and got.shape == want.shape and got.dtype == bag.dtype
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (n, ratio)
    assert int(np.random.randint(1 << 30)) == int(gold["next_draw"])


@pytest.mark.parametrize("ratio", [0, -1, 1.5])
def test_ratios_the_reference_ignores_return_the_bag_and_draw_nothing(ratio):
    from advmil_amd.utils.func import random_mask_square_instance, square_instance_keep
    np.random.seed(11)
    before = np.random.get_state()
    bag = torch.randn(24, 4)                                                  # (not even whole regions: the ratio is looked at first)
    assert random_mask_square_instance(bag, ratio) is bag
    assert random_mask_square_instance(bag, ratio, mask_way="x") is bag
    assert square_instance_keep(24, ratio) is None
    after = np.random.get_state()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]


def test_a_bag_that_is_not_whole_regions_raises():
    from advmil_amd.utils.func import random_mask_square_instance, square_instance_keep
    with pytest.raises(AssertionError, match="bag must consist of square instances."):
        square_instance_keep(24, 0.5)
    with pytest.raises(AssertionError, match="bag must consist of square instances."):
        random_mask_square_instance(torch.zeros(24, 4), 0.5)


def test_an_unknown_mask_way_raises():
    from advmil_amd.utils.func import random_mask_square_instance
    with pytest.raises(NotImplementedError, match="mask_way=x"):
        random_mask_square_instance(torch.zeros(32, 4), 0.5, mask_way="x")


def test_keep_bitmap_words():
    """Bit r & 31 of word r >> 5 = region r."""
    from advmil_amd.utils.func import keep_bitmap
    w = keep_bitmap(np.array([0, 31, 32, 64]), 65)
    assert w.dtype == np.uint32 and w.tolist() == [0x80000001, 1, 1]
    assert keep_bitmap(np.array([0]), 1).tolist() == [1] and keep_bitmap(np.arange(33), 33).tolist() == [0xFFFFFFFF, 1]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from advmil_amd import _lib
    return _lib.lib()


def test_stage_bag_masked_rejects_bad_arguments_before_any_launch(lib):
    """The sibling's checks plus the bitmap's: NULL source, NULL keep_bits, misaligned pointers, rows % 16, one plane only, and no
    destination rows without planes to derive. 64 rows x 8 fp32 channels; no address here is ever dereferenced."""
    P = ctypes.c_void_p
    rows, C = 64, 8
    nb = rows * C * 4
    src, dst, hi, lo, shi, slo, bits = A16, A16 + (1 << 20), A16 + (2 << 20), A16 + (3 << 20), A16 + (4 << 20), A16 + (5 << 20), A16 + (6 << 20)

    def call(dst_rows=dst, src_rows=src, rows_bytes=nb, n_rows=rows, dst_hi=hi, src_hi=None, dst_lo=lo, src_lo=None, plane_bytes=nb // 2,
             keep_bits=bits):
        p = lambda v: None if v is None else P(v)      # noqa: E731
        return lib.advmil_stage_bag_masked(p(dst_rows), p(src_rows), rows_bytes, n_rows, p(dst_hi), p(src_hi), p(dst_lo), p(src_lo),
                                           plane_bytes, p(keep_bits), None)
    none = dict(dst_hi=None, dst_lo=None, plane_bytes=0)
    assert call(src_rows=None) == EINVAL                                      # NULL source
    assert call(keep_bits=None) == EINVAL                                     # NULL bitmap
    assert call(keep_bits=bits + 2) == EINVAL                                 # bitmap words are 4-byte aligned
    for k, v in (("dst_rows", dst + 4), ("src_rows", src + 8), ("dst_hi", hi + 2), ("dst_lo", lo + 4)):
        assert call(**{k: v}) == EINVAL, k                                    # 16-byte alignment
    assert call(src_hi=shi + 4, src_lo=slo) == EINVAL
    assert call(n_rows=rows - 8, rows_bytes=(rows - 8) * C * 4, plane_bytes=(rows - 8) * C * 2) == EINVAL      # rows % 16
    assert call(n_rows=0) == EINVAL and call(rows_bytes=0) == EINVAL
    assert call(dst_lo=None) == EINVAL and call(dst_hi=None) == EINVAL        # one plane only
    assert call(src_hi=shi) == EINVAL and call(src_lo=slo) == EINVAL          # one held plane only
    assert call(plane_bytes=0) == EINVAL and call(plane_bytes=nb // 2 - 16) == EINVAL
    assert call(dst_rows=None, **none) == EINVAL                              # nothing to write at all
    assert call(dst_rows=None, src_hi=shi, src_lo=slo) == EINVAL              # planes-only staging derives its planes
