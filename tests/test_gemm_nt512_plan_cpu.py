"""CPU: when the plan of the plane-fed NT kernel answers the 512x128 tile (code 87, csrc/gemm_host.hip::advmil_gemm_f32_plan_planes)
and what advmil_gemm_f32_tiled refuses for it. The refusals return before any launch, so they are asked of the library itself on fake
addresses, as tests/test_gemm_walks_plan_cpu.py asks its own."""
import ctypes

import pytest

EINVAL = -1
A16 = 0x7F0000001000          # a fake, 16-byte aligned "device address": never dereferenced when validation does its job


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from advmil_amd import _lib
    lib = _lib.lib()
    prev = lib.advmil_get_gemm_mode()
    lib.advmil_set_gemm_mode(1)
    yield _lib
    lib.advmil_set_gemm_mode(prev)


def plan(lib, M, N, K):
    t = ctypes.c_int(-1)
    assert lib.advmil_gemm_f32_plan_planes(1, 1, M, N, K, ctypes.byref(t)) == 0
    return t.value


def test_the_plan_answers_87_for_deep_n128_slabs_only(L, monkeypatch):
    lib = L.lib()
    monkeypatch.delenv("ADVMIL_NT_PLANES_TN", raising=False)
    for shape in ((131072, 128, 1024), (524288, 128, 1024), (131072, 128, 64)):
        assert plan(lib, *shape) == 87, shape
    # one wave of 256x128 tiles (PatchGCN) and a row count that 512 does not divide keep 256x128
    for shape in ((65536, 128, 1024), (131072 + 256, 128, 1024)):
        assert plan(lib, *shape) == 82, shape
    # every other width answers as before: the widest tile that divides N (and none for 192, which the plan's N % 128 turns away)
    assert [plan(lib, 131072, n, 1024) for n in (192, 256, 384, 768)] == [0, 82, 83, 83]
    # ... and nothing below the kernel's own limits
    assert plan(lib, 131072, 128, 32) == 0 and plan(lib, 131072, 128, 1024 + 16) == 0
    # the same-build A/B switch
    monkeypatch.setenv("ADVMIL_NT_PLANES_TN", "2")
    assert plan(lib, 131072, 128, 1024) == 82
    monkeypatch.setenv("ADVMIL_NT_PLANES_TN", "3")
    assert plan(lib, 131072, 128, 1024) == 87          # (192 does not divide 128: the switch does not apply)


def test_no_gate_blocks_and_no_column_sums(L):
    lib = L.lib()
    assert lib.advmil_gemm_f32_gate_blocks(87, 128) == 0
    assert lib.advmil_gemm_f32_colsum_rows(87, 131072, 128) == 0


def tiled(L, M=512, N=128, K=64, splits=1, b_planes=2, **fields):
    """advmil_gemm_f32_tiled(tile = 87) on fake addresses, both operands as planes; `fields` are written into the epilogue."""
    lib = L.lib()
    e = L.Epilogue()
    e.alpha, e.act_split = 1.0, 1 << 30
    pa, pb = A16 + (1 << 36), A16 + (2 << 36)
    e.a_hi, e.a_lo = pa, pa + (1 << 34)
    e.b_hi, e.b_lo = pb, (pb + (1 << 34)) if b_planes == 2 else None
    for k, v in fields.items():
        setattr(e, k, v)
    wsb = lib.advmil_gemm_f32_workspace_bytes(M, N, splits)
    return lib.advmil_gemm_f32_tiled(1, 1, M, N, K, ctypes.c_void_p(A16), K, ctypes.c_void_p(A16 + (3 << 36)), K, ctypes.c_void_p(A16 + (4 << 36)), N,
                                     ctypes.byref(e), splits, 87, ctypes.c_void_p(A16 + (6 << 36)), wsb, None)


FAKE = A16 + (7 << 36)
REFUSED = {
    "M%512": dict(M=768),
    "N=256": dict(N=256),
    "K=32": dict(K=32),
    "K%32": dict(K=80),
    "splits=2": dict(K=128, splits=2),
    "accumulate": dict(accumulate=1),
    "rowv": dict(rowv=FAKE, colv=FAKE + 4096),
    "maskbits": dict(maskbits=FAKE, ldbits=4, mask_scale=2.0),
    "single-plane-B": dict(b_planes=1),
    "A-planes-span-2^32": dict(M=1 << 21, K=1024),
}


@pytest.mark.parametrize("why", sorted(REFUSED))
def test_refusals_before_any_launch(L, why):
    """ADVMIL_EINVAL; a positive return would be a hipError_t: the call got to a launch."""
    assert tiled(L, **REFUSED[why]) == EINVAL, why
