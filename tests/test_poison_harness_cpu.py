"""No GPU: the allocation-poisoning harness itself (tests/poison.py) -- every entry point is filled with both patterns, the originals
come back, ops._ws is reached, and three stand-in "kernels" show what the harness catches that a recycled buffer hides."""
import math

import pytest
import torch

from tests import poison as P
from tests.poison import poison  # noqa: F401  (the fixture, by name)

DTYPES = [torch.float32, torch.bfloat16, torch.int32, torch.int64, torch.bool]
ENTRY = {
    "empty": lambda dt: torch.empty(5, 3, dtype=dt),
    "empty_like": lambda dt: torch.empty_like(torch.zeros(5, 3, dtype=dt)),
    "empty_strided": lambda dt: torch.empty_strided((5, 3), (3, 1), dtype=dt),
    "new_empty": lambda dt: torch.zeros(2, dtype=dt).new_empty((5, 3)),
}


@pytest.mark.parametrize("byte", P.PATTERNS)
@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("entry", sorted(ENTRY))
def test_every_entry_point_is_filled(entry, dt, byte):
    with P.poisoned_allocations(byte, host=True):
        t = ENTRY[entry](dt)
    assert t.shape == (5, 3) and t.dtype == dt
    if dt == torch.bool:
        assert bool(t.all())
        return
    assert bool((t.view(torch.uint8) == byte).all())
    if dt.is_floating_point:
        if byte == 0xFF:
            assert bool(torch.isnan(t).all())
        else:                                                   # finite, and two of them overflow an fp32 sum
            assert bool(torch.isfinite(t).all()) and float(t.float()[0, 0]) > 3.3e38
            assert math.isinf(float(t.float()[0, 0] + t.float()[0, 1]))
    else:
        assert int(t[0, 0]) == {(0xFF, torch.int32): -1, (0xFF, torch.int64): -1, (0x7F, torch.int32): 2139062143,
                                (0x7F, torch.int64): 0x7F7F7F7F7F7F7F7F}[(byte, dt)]


def test_pageable_host_memory_only_on_request_and_gapped_strides():
    z = torch.zeros(64)
    del z
    with P.poisoned_allocations(0xFF):
        t = torch.empty(4, dtype=torch.int32)
        t.fill_(3)                                              # (left alone: whatever it held, no fill ran over it afterwards)
        assert int(t.sum()) == 12
    with P.poisoned_allocations(0x7F, host=True):
        s = torch.empty_strided((4, 2), (4, 1), dtype=torch.int32)            # two of every four elements are gaps
        t = torch.empty_strided((3, 4), (1, 3), dtype=torch.float32)          # dense, permuted
        e = torch.empty(0)
    whole = torch.empty(0, dtype=torch.uint8).set_(s.untyped_storage())
    assert bool((whole == 0x7F).all()) and whole.numel() >= 14 * 4
    assert bool((t.t().contiguous().view(torch.uint8) == 0x7F).all()) and e.numel() == 0


def test_leaf_that_requires_grad_and_zero_dim_tensors_are_filled_too():
    with P.poisoned_allocations(0xFF, host=True):
        t = torch.empty(3, requires_grad=True)
        z = torch.empty((), dtype=torch.int32)
    assert t.requires_grad and t.is_leaf and bool(torch.isnan(t.detach()).all()) and int(z) == -1
    P.assert_same_bits([[torch.tensor(1.5)], [torch.tensor(1.5)]])
    with pytest.raises(AssertionError):
        P.assert_same_bits([[torch.tensor(1.5)], [torch.tensor(2.5)]])


def test_originals_are_restored_after_exit_and_after_an_exception():
    orig = (torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty)
    with P.poisoned_allocations(0xFF, host=True):
        assert torch.empty is not orig[0] and torch.Tensor.new_empty is not orig[3]
    assert (torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty) == orig
    with pytest.raises(ZeroDivisionError):
        with P.poisoned_allocations(0x7F, host=True):
            assert torch.empty_like is not orig[1]
            1 / 0
    assert (torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty) == orig
    with P.poisoned_allocations(0xFF, host=True):               # nesting: the inner one hands back the outer patch, then the originals
        outer = torch.empty
        with P.poisoned_allocations(0x7F, host=True):
            assert bool((torch.empty(4, dtype=torch.uint8) == 0x7F).all()) and P.active() == 0x7F
        assert torch.empty is outer and bool((torch.empty(4, dtype=torch.uint8) == 0xFF).all())
    assert torch.empty is orig[0] and P.active() is None


@pytest.mark.parametrize("byte", P.PATTERNS)
def test_ops_workspace_comes_back_filled(byte):
    from advmil_amd import ops
    with P.poisoned_allocations(byte, host=True):
        w = ops._ws(1000, "cpu")
        pl = ops.Planes.alloc((4, 8), torch.device("cpu"))
    assert w.dtype == torch.float32 and w.numel() >= 250 and bool((w.view(torch.uint8) == byte).all())
    assert bool((pl.hi.view(torch.uint8) == byte).all()) and bool((pl.lo.view(torch.uint8) == byte).all())


SEEN = []


def test_the_fixture_patches_for_the_test_body_once_per_pattern(poison):
    SEEN.append(poison)
    assert poison in P.PATTERNS and P.active() == poison
    assert torch.empty(4).is_pinned() is False                  # (pageable host memory is left alone by the fixture)
    if len(SEEN) == 2:
        assert tuple(SEEN) == P.PATTERNS == (0xFF, 0x7F)


def test_assert_same_bits_compares_bits_structure_and_scalars():
    a = {"y": torch.tensor([1.0, float("nan")]), "n": 3, "pl": [torch.tensor([True, False])]}
    P.assert_same_bits([a, P._snapshot(a), P._snapshot(a), P._snapshot(a)])            # a NaN that is always there is equal here ...
    with pytest.raises(AssertionError):
        P.assert_finite(a)                                                              # ... and caught here
    b = P._snapshot(a); b["y"][0] = 1.0 + 2 ** -23
    with pytest.raises(AssertionError, match="poisoned 0xFF differs from plain at r\\['y'\\]"):
        P.assert_same_bits([a, P._snapshot(a), b, P._snapshot(a)])
    c = P._snapshot(a); c["n"] = 4
    with pytest.raises(AssertionError):
        P.assert_same_bits([a, c])
    with pytest.raises(AssertionError):
        P.assert_same_bits([a, {"y": a["y"]}])
    with pytest.raises(AssertionError):
        P.assert_same_bits([{}, {}])
    z = torch.zeros(2)
    with pytest.raises(AssertionError):                                                 # -0.0 == 0.0 as numbers, not as bits
        P.assert_same_bits([[z], [-z]])


# ------------------------------------------------------------------------------------------------------------------------------
# teeth: three stand-in kernels that a recycled-buffer comparison passes
# ------------------------------------------------------------------------------------------------------------------------------
X = torch.arange(1.0, 1025.0)


def _recycled():
    """torch.empty as a test sees it from the caching allocator: the block just freed, still holding what was written last (a zero
    page at first sight). Under poisoned_allocations the request goes to the patched torch.empty, as every real call site's does."""
    pool = {}

    def empty(*shape, dtype=torch.float32):
        if P.active() is not None:
            return torch.empty(*shape, dtype=dtype)
        key = (tuple(shape), dtype)
        if key not in pool:
            pool[key] = torch.zeros(*shape, dtype=dtype)
        return pool[key]
    return empty


def _run3(kernel):
    return P.three_runs(kernel, host=True)


def test_teeth_output_element_not_written():
    """A 'kernel' that skips the last output element on every launch but the first: the repeat loop of a test sees the previous
    launch's answer in the recycled block and passes; both patterns catch it."""
    empty = _recycled()
    calls = []

    def kernel():
        out = empty(1024)
        n = 1024 if not calls else 1023
        calls.append(n)
        out[:n] = 2 * X[:n]
        return out

    want = 2 * X
    for _ in range(4):                                           # the recycled-buffer comparison: passes
        assert torch.equal(kernel(), want)
    trees = _run3(kernel)
    assert torch.equal(trees[0], trees[1])
    for k in (2, 3):
        with pytest.raises(AssertionError):
            P.assert_same_bits([trees[0], trees[k]])
    with pytest.raises(AssertionError, match="poisoned 0xFF"):
        P.assert_same_bits(trees)
    assert math.isnan(float(trees[2][-1])) and float(trees[3][-1]) > 3.3e38


def test_teeth_workspace_read_before_written():
    """A 'kernel' that sums a workspace it only half wrote (a grid sized by the longest bag over a shorter one): zero pages and its
    own earlier partials make the plain result right; both patterns catch it."""
    empty = _recycled()

    def kernel():
        ws = empty(8)
        ws[:4] = X[:1024].reshape(4, 256).sum(1)                 # four real partials of eight launched
        return ws.sum().reshape(1)

    assert float(kernel()) == float(X.sum()) == float(kernel())
    trees = _run3(kernel)
    assert torch.equal(trees[0], trees[1]) and float(trees[0]) == float(X.sum())
    assert math.isnan(float(trees[2])) and math.isinf(float(trees[3]))
    for k in (2, 3):
        with pytest.raises(AssertionError):
            P.assert_same_bits([trees[0], trees[k]])


def test_teeth_unwritten_element_behind_a_relu_needs_the_finite_pattern():
    """The same read behind max(z, 0) -- the fmaxf / z > 0 ? z : 0 forms of the ReLU and softmax code map a NaN to 0: the NaN pattern
    passes, the finite one overflows the sum."""
    empty = _recycled()

    def kernel():
        ws = empty(8)
        ws[:4] = X[:4] - 2.0
        z = torch.fmax(ws, torch.zeros(()))                      # clamp_min(0) as the kernels write it: fmaxf(z, 0.f) drops a NaN
        return z.sum().reshape(1)

    trees = _run3(kernel)
    assert float(trees[0]) == 3.0
    P.assert_same_bits([trees[0], trees[1], trees[2]], names=P.RUN_NAMES[:3])          # 0xFF: missed
    with pytest.raises(AssertionError, match="poisoned 0x7F"):
        P.assert_same_bits(trees)                                                       # 0x7F: caught
    assert float(trees[3]) > 3.3e38
    assert math.isnan(float(torch.tensor(float("nan")).clamp_min(0)))                   # (torch's own clamp_min hands a NaN through)
