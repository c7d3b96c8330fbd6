"""CPU: the negative paths of advmil_logrank_rows (include/advmil_hip.h). Validation runs before anything is enqueued, so none of these
calls needs a device: every out-of-range argument answers ADVMIL_EINVAL (-1), a short workspace ADVMIL_EWORKSPACE (-2); a positive
return would be a hipError_t, i.e. the call got as far as a launch."""
import ctypes
import os
import re

import pytest

EINVAL, EWORKSPACE = -1, -2
A16 = 0x7F0000001000          # a fake, 16-byte aligned "device address": never dereferenced when validation does its job
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from advmil_amd import _lib
    return _lib


def _p(k, off=0):
    return ctypes.c_void_p(A16 + (k << 24) + off)


GOOD = dict(stime=_p(0), sevent=_p(1), order=_p(2), n=64, groups=_p(3), ldg=64, weights=_p(4), ldw=64, R=8, at=_p(5), Q=16, counts=_p(6),
            sums=_p(7), km=_p(8), median=_p(9), ws=_p(10), ws_bytes=64 * 4)
NAMES = list(GOOD)


def _call(L, **kw):
    a = dict(GOOD, **kw)
    return L.lib().advmil_logrank_rows(*(a[k] for k in NAMES), None)


def test_symbols_are_declared_bound_and_exported(L):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "advmil_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(advmil_[a-z0-9_]+)\s*\(", hdr))
    handle = ctypes.CDLL(L.LIB_PATH)
    for name in ("advmil_logrank_rows", "advmil_logrank_rows_workspace_bytes"):
        assert name in declared and name in L.SIGNATURES and hasattr(handle, name), name
    assert len(L.SIGNATURES["advmil_logrank_rows"][1]) == len(NAMES) + 1


def test_workspace_query_is_a_pure_host_function(L):
    f = L.lib().advmil_logrank_rows_workspace_bytes
    assert f(1000, 0) == 0 and f(1000, 100) == 4000 and f(1, 1) == 4 and f(1 << 20, 1 << 16) == 4 << 20 and f(0, 5) == 0


def test_every_null_pointer_is_refused(L):
    for name in ("stime", "sevent", "order", "groups", "counts", "sums", "median", "at", "km", "ws"):
        assert _call(L, **{name: None}) == EINVAL, name


def test_what_may_be_absent_is_refused_for_the_next_reason_only(L):
    """weights NULL means all ones, and with Q == 0 neither at, km nor ws is needed: such a call passes validation -- shown by making
    it fail on ANOTHER argument, since a valid call would launch."""
    assert _call(L, weights=None, ldw=0, n=0) == EINVAL
    assert _call(L, weights=None, ldw=0, ws_bytes=64 * 4 - 1) == EWORKSPACE          # got past every EINVAL check without weights
    assert _call(L, Q=0, at=None, km=None, ws=None, ws_bytes=0, counts=_p(6, 4)) == EINVAL
    assert _call(L, ldg=0, ws_bytes=0) == EWORKSPACE                                  # ldg == 0: one shared row of groups


@pytest.mark.parametrize("kw", [dict(n=0, ldg=0), dict(n=-1), dict(n=(1 << 20) + 1, ldg=1 << 21, ldw=1 << 21, ws_bytes=1 << 30),
                                dict(R=0), dict(R=-3), dict(R=(1 << 20) + 1), dict(Q=-1), dict(Q=(1 << 16) + 1, ws_bytes=1 << 30),
                                dict(ldg=63), dict(ldg=1), dict(ldg=-64), dict(ldw=63), dict(ldw=0), dict(ldw=-64)],
                         ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_out_of_range_shapes(L, kw):
    assert _call(L, **kw) == EINVAL


@pytest.mark.parametrize("name,off", [("stime", 2), ("sevent", 1), ("order", 2), ("weights", 2), ("at", 1), ("ws", 2), ("counts", 4), ("sums", 4),
                                      ("km", 4), ("median", 4)])
def test_misaligned_pointers(L, name, off):
    k = NAMES.index(name)
    assert _call(L, **{name: _p(k, off)}) == EINVAL
    assert _call(L, **{name: _p(k, 16), "ws_bytes": 0}) == EWORKSPACE                 # (aligned elsewhere: validation goes on to the workspace)


def test_workspace_too_small(L):
    need = L.lib().advmil_logrank_rows_workspace_bytes(64, 16)
    assert _call(L, ws_bytes=need - 1) == EWORKSPACE and _call(L, ws_bytes=0) == EWORKSPACE
    assert _call(L, ws_bytes=need - 1, n=0) == EINVAL                                 # the argument checks come first
