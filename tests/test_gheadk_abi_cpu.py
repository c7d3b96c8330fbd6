"""CPU: the width-K generator head's C ABI (advmil_gheadk_workspace_bytes / _fwd / _bwd, the wide form of csrc/ghead.hip) without a device:
exported and bound, the argument block laid out as C lays it out, the workspace query a pure host function that grows with K where a slice's share is
[B, K], and every argument check answered before anything is launched (the pointers below are host addresses no kernel may ever see)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("advmil_gheadk_workspace_bytes", "advmil_gheadk_fwd", "advmil_gheadk_bwd")
EINVAL, EWORKSPACE = -1, -2


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from advmil_amd import _lib
    return _lib


def test_symbols_are_declared_bound_and_exported(built):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "advmil_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(advmil_[a-z0-9_]+)\s*\(", txt))
    handle = ctypes.CDLL(built.LIB_PATH)
    for n in NAMES:
        assert n in declared and n in built.SIGNATURES and hasattr(handle, n), n
    assert built.SIGNATURES["advmil_gheadk_fwd"][1][0] is ctypes.POINTER(built.GHeadK)
    assert built.SIGNATURES["advmil_gheadk_bwd"][1][0] is ctypes.POINTER(built.GHeadK)
    assert len(built.SIGNATURES["advmil_gheadk_workspace_bytes"][1]) == 5


def test_struct_layout_matches_c(built, tmp_path):
    """sizeof / offsetof of advmil_gheadk_t from a C program compiled against the header, against the ctypes mirror."""
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    cls, cname = built.GHeadK, "advmil_gheadk_t"
    body = f'printf("%zu\\n", sizeof({cname}));' + "".join(f'printf("%zu\\n", offsetof({cname}, {f}));' for f, _ in cls._fields_)
    src = tmp_path / "layout_gheadk.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "advmil_hip.h"\n' f"int main(void){{{body}return 0;}}\n")
    exe = tmp_path / "layout_gheadk"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out == [ctypes.sizeof(cls)] + [getattr(cls, f).offset for f, _ in cls._fields_]
    names = [f for f, _ in cls._fields_]
    assert names[:8] == ["B", "d0", "d1", "d2", "K", "noise_mode", "out_act", "reserved"] and names[8:] == [f for f, _ in built.GHead._fields_[6:]]


def test_workspace_query_is_a_pure_host_function(built):
    L = built.lib()
    q = L.advmil_gheadk_workspace_bytes
    # d1 > 0: shares of MLPs[0]'s pre-activation [B, d2] forward, of dX [B, d0] backward -- nothing depends on K
    assert q(32, 384, 384, 192, 1) == q(32, 384, 384, 192, 32) == 24 * 32 * 384 * 4
    # d1 == 0: a slice's share of the output layer is [B, K]: max(d0, d2, K) floats per (slice, bag)
    assert q(4, 128, 0, 64, 4) == 4 * 4 * 128 * 4
    assert q(3, 8, 0, 16, 5) == 1 * 3 * 16 * 4 and q(3, 8, 0, 16, 17) == 1 * 3 * 17 * 4 and q(3, 8, 0, 16, 32) == 1 * 3 * 32 * 4
    assert q(3, 8, 0, 16, 16) < q(3, 8, 0, 16, 17) < q(3, 8, 0, 16, 32)
    assert q(0, 8, 0, 16, 4) == 0 and q(3, 8, 0, 16, 0) == 0
    # K = 1 asks for what the width-1 head asks for
    for shape in ((32, 384, 384, 192), (5, 384, 0, 192), (1, 128, 0, 64)):
        assert q(*shape, 1) == L.advmil_ghead_workspace_bytes(*shape)


def _block(built, bufs, B=4, d0=128, d1=0, d2=64, K=4, noise_mode=1, **over):
    """A valid argument block over host memory (16-byte aligned): nothing of it may be dereferenced by a call that returns an error."""
    L = built.lib()
    n = 1 << 16
    buf = (ctypes.c_float * n)()
    bufs.append(buf)
    base = (ctypes.addressof(buf) + 15) // 16 * 16
    a = built.GHeadK()
    a.B, a.d0, a.d1, a.d2, a.K, a.noise_mode, a.out_act = B, d0, d1, d2, K, noise_mode, 1
    for i, f in enumerate(("x", "Wr", "br", "W0", "b0", "W1", "b1", "hs", "h2", "pred", "dpred", "dx", "ws")):
        setattr(a, f, base + 1024 * i)
    a.ldx = a.lddx = d0
    a.ws_bytes = L.advmil_gheadk_workspace_bytes(B, d0, d1, d2, K)
    for k, v in over.items():
        setattr(a, k, v)
    return a


def test_argument_errors_return_einval_before_any_launch(built):
    L = built.lib()
    bufs = []
    bad = [dict(K=0), dict(K=33), dict(B=33), dict(W1=None), dict(pred=None), dict(d2=62), dict(d2=66)]
    for over in bad:
        for d1 in (0, 384):
            a = _block(built, bufs, d1=d1, **over)
            a.ws_bytes = 1 << 30                  # (never the reason)
            assert L.advmil_gheadk_fwd(ctypes.byref(a), None) == EINVAL, (over, d1)
            assert L.advmil_gheadk_bwd(ctypes.byref(a), None) == EINVAL, (over, d1)
    a = _block(built, bufs, dpred=None)
    assert L.advmil_gheadk_bwd(ctypes.byref(a), None) == EINVAL
    assert L.advmil_gheadk_fwd(None, None) == EINVAL and L.advmil_gheadk_bwd(None, None) == EINVAL


@pytest.mark.parametrize("shape", [(4, 128, 0, 64, 4), (32, 384, 384, 192, 32), (3, 8, 0, 16, 32)])
def test_short_workspace_returns_eworkspace(built, shape):
    L = built.lib()
    bufs = []
    B, d0, d1, d2, K = shape
    a = _block(built, bufs, B=B, d0=d0, d1=d1, d2=d2, K=K)
    assert a.ws_bytes > 0
    a.ws_bytes -= 1
    assert L.advmil_gheadk_fwd(ctypes.byref(a), None) == EWORKSPACE
    assert L.advmil_gheadk_bwd(ctypes.byref(a), None) == EWORKSPACE
