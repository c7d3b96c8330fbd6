"""Allocation poisoning ("Allocation poisoning"), as one helper.

Every device buffer of the HIP path is a `torch.empty` block of the caching allocator: outputs, operand planes, saved statistics
and the workspaces of ops._ws(). What such a block held before the launch is whatever the previous owner left there -- in a test,
usually the previous launch's correct answer or a fresh zero page. `poisoned_allocations(byte)` takes that luck away: while it is
active torch.empty / torch.empty_like / torch.empty_strided / Tensor.new_empty fill every byte of what they return with `byte`.

Two patterns, because neither is enough alone:

  0xFF   fp32 / bf16 NaN, integers -1        a NaN spreads through every sum that reads it;
  0x7F   fp32 3.39e38 (finite), int32 2139062143, int64 9.19e18
                                              fmaxf(z, 0), z > 0 ? z : 0, running maxima and > 0 masks turn a NaN into 0; the finite
                                              pattern survives them and overflows the next sum.

The rule the tests assert: a result must not move, bit for bit, with what its buffers held before -- `three_runs(fn)` runs `fn` plain,
plain again (determinism, the precondition), under 0xFF and under 0x7F; `assert_same_bits` compares the four result trees."""
import contextlib

import pytest
import torch

NAN_BYTE = 0xFF        # NaN in fp32 / bf16, -1 in the integer types
BIG_BYTE = 0x7F        # 3.39e38 in fp32 / bf16: finite, survives max(z, 0) and overflows the next sum
PATTERNS = (NAN_BYTE, BIG_BYTE)


_ACTIVE = []           # the bytes of the poisoned_allocations contexts that are open, innermost last


def active():
    """The byte fresh allocations are filled with right now, or None outside every poisoned_allocations context."""
    return _ACTIVE[-1] if _ACTIVE else None


def _capturing():
    return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()


def _fill(t, byte, host, empty, pinned=False):
    """Fill every byte of a freshly allocated tensor (device and pinned host memory; pageable host memory only with host=True).
    `pinned`: the call asked for pin_memory=True. A host tensor that inherits its pinning (empty_like / new_empty of a pinned tensor) is
    recognised by asking the driver, which is not done while a stream is being captured: inside a capture only the keyword counts."""
    if not isinstance(t, torch.Tensor) or t.layout != torch.strided or t.numel() == 0 or t.device.type == "meta":
        return t
    if t.device.type == "cpu" and not (host or pinned or (not _capturing() and t.is_pinned())):
        return t
    with torch.no_grad():
        d = t.detach()
        if d.dtype == torch.bool:
            d.fill_(True)
        elif d.is_contiguous():
            d.reshape(-1).view(torch.uint8).fill_(byte)             # (reshape: a 0-dim tensor has no last dimension to re-type)
        else:                                   # empty_strided with gaps or permuted strides: the whole block behind it
            empty(0, dtype=torch.uint8, device=d.device).set_(d.untyped_storage()).fill_(byte)
    return t


@contextlib.contextmanager
def poisoned_allocations(byte, host=False):
    """While active, the four allocation entry points return blocks filled with `byte` (capturable: the fill is an ordinary kernel).
    The callers look the torch attributes up at call time, so patching them reaches ops._ws, Planes.alloc, the handlers and the
    stager alike. The originals are put back on exit, after an exception too."""
    byte = int(byte)
    assert 0 <= byte <= 0xFF, byte
    orig = (torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty)
    empty = orig[0]

    def wrap(f):
        def poisoned(*a, **k):
            return _fill(f(*a, **k), byte, host, empty, bool(k.get("pin_memory")))
        poisoned.__wrapped__ = f
        poisoned.__name__ = getattr(f, "__name__", "empty")
        return poisoned

    torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty = (wrap(f) for f in orig)
    _ACTIVE.append(byte)
    try:
        yield byte
    finally:
        _ACTIVE.pop()
        torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty = orig


@pytest.fixture(params=PATTERNS, ids=["nan_ff", "big_7f"])
def poison(request):
    """The test body runs with every fresh allocation poisoned; once per pattern. Test modules import this fixture by name."""
    with poisoned_allocations(request.param):
        yield request.param


# ------------------------------------------------------------------------------------------------------------------------------
# result trees: tensors, objects holding hi / lo planes, lists / tuples / dicts of them, None and plain numbers
# ------------------------------------------------------------------------------------------------------------------------------
def tensors(tree, path="r"):
    """-> [(path, tensor)] of every tensor of a result tree, in a fixed order."""
    if tree is None or isinstance(tree, (bool, int, float, str)):
        return []
    if isinstance(tree, torch.Tensor):
        return [(path, tree)]
    if isinstance(tree, dict):
        return [x for k in tree for x in tensors(tree[k], f"{path}[{k!r}]")]
    if isinstance(tree, (list, tuple)):
        return [x for i, v in enumerate(tree) for x in tensors(v, f"{path}[{i}]")]
    if hasattr(tree, "hi") and hasattr(tree, "lo"):                 # ops.Planes
        return tensors(tree.hi, path + ".hi") + tensors(tree.lo, path + ".lo")
    raise TypeError(f"{path}: {type(tree).__name__} in a result tree")


def _scalars(tree, path="r"):
    if isinstance(tree, (bool, int, float, str)):
        return [(path, tree)]
    if isinstance(tree, dict):
        return [x for k in tree for x in _scalars(tree[k], f"{path}[{k!r}]")]
    if isinstance(tree, (list, tuple)):
        return [x for i, v in enumerate(tree) for x in _scalars(v, f"{path}[{i}]")]
    return []


def _snapshot(tree):
    """The tree with every tensor replaced by a detached copy of its own (taken outside any poisoning, by clone: a result that is a
    view of a recycled workspace must not change under the later runs)."""
    if isinstance(tree, torch.Tensor):
        return tree.detach().clone()
    if isinstance(tree, dict):
        return {k: _snapshot(v) for k, v in tree.items()}
    if isinstance(tree, (list, tuple)):
        return [_snapshot(v) for v in tree]
    if tree is not None and hasattr(tree, "hi") and hasattr(tree, "lo"):
        return {"hi": _snapshot(tree.hi), "lo": _snapshot(tree.lo)}
    return tree


def three_runs(fn, host=False):
    """fn() plain, plain again, under 0xFF and under 0x7F -> the four result trees (snapshots)."""
    out = [_snapshot(fn()), _snapshot(fn())]
    for byte in PATTERNS:
        with poisoned_allocations(byte, host=host):
            r = fn()
        out.append(_snapshot(r))
    return out


RUN_NAMES = ("plain", "plain again", "poisoned 0xFF", "poisoned 0x7F")


def _bits(t):
    t = t.detach().contiguous().reshape(-1)
    return t.to(torch.uint8) if t.dtype == torch.bool else t.view(torch.uint8)


def assert_same_bits(trees, names=RUN_NAMES):
    """Every tree equals the first one: same structure, shapes and types, and the same BITS in every tensor (NaNs compare by their
    bits, so a NaN that is there in every run passes this check and fails assert_finite)."""
    ref = tensors(trees[0])
    ref_s = _scalars(trees[0])
    assert ref or ref_s, "empty result tree: nothing would be compared"
    for name, tree in zip(names[1:], trees[1:]):
        got = tensors(tree)
        assert [p for p, _ in got] == [p for p, _ in ref], (name, [p for p, _ in got], [p for p, _ in ref])
        assert _scalars(tree) == ref_s, (name, _scalars(tree), ref_s)
        for (p, a), (_, b) in zip(got, ref):
            assert a.dtype == b.dtype and a.shape == b.shape, (name, p, a.dtype, b.dtype, tuple(a.shape), tuple(b.shape))
            ba, bb = _bits(a), _bits(b)
            if not torch.equal(ba, bb):
                item = max(a.element_size(), 1)
                bad = (ba.reshape(-1, item) != bb.reshape(-1, item)).any(dim=1) if a.dtype != torch.bool else (ba != bb).reshape(-1)
                first = int(bad.nonzero()[0])
                raise AssertionError(f"{name} differs from {names[0]} at {p}: {int(bad.sum())} of {a.numel()} elements, first at flat "
                                     f"index {first}: {a.reshape(-1)[first].item()!r} vs {b.reshape(-1)[first].item()!r}")


def assert_finite(tree):
    for p, t in tensors(tree):
        if t.is_floating_point():
            assert bool(torch.isfinite(t).all()), f"{p}: {int((~torch.isfinite(t)).sum())} non-finite of {t.numel()}"
