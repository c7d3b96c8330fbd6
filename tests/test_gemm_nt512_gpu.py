"""GPU: every walk of the 512x128 form of the plane-fed NT kernel (tile code 87, csrc/gemm_nt_planes.hip: TM = 4, two ring slots of
80 KB, the plain streaming epilogue), by the method of tests/test_gemm_walks_gpu.py and against the same oracle (tests/gemm_ref.py).

All four operand planes hold independent small integers, so every product and partial sum of `al bh + ah bl + ah bh` is an integer
below 2^24, exact in fp32 in any order: the result must be EQUAL (torch.equal) to the float64 evaluation of that formula and of an
epilogue kept exact (alpha 1 / 0.5, integer bias, ReLU). Both operands travel with no usable fp32 image (None, or NaN under
fp32_stale). The tile is forced through `tile=`, so the shapes are the smallest that reach each walk:
  M = 512              one tile, one workgroup
  M = 1024             two workgroups
  M = 512 * 9          the `rem` branch of tile_of (mtiles = 9)
  M = 512 * (CUs + 1)  one workgroup walks two tiles: the ring runs across tiles, dA != 0, the epilogue's stores stay in flight under
                       the next tile's first (counted) wait. K = 64 keeps it small.
  K / 32 = 2, 3, 4, 5  (two ring slots: even and odd chunk counts end in different slots, where the epilogue patch then lives)
  pitch > K, ldc > N; bias with and without ReLU; emitted planes; two-plane and single-plane A (the latter's patch sits behind the ring).
One random-valued case per A form: the output of tile 87 is torch.equal to that of tile 82 on the same operands -- the k order is the
same, so every output bit is.
Every launch asserts the kernel ops.gemm recorded (ops.KERNEL_PROFILE)."""
import collections

import pytest
import torch

from tests import gemm_ref as R
from tests.gemm_ref import Epi

pytestmark = pytest.mark.gpu
DEV = R.DEV
TILE, N = 87, 128
NAME = "gemm_nt_planes_kernel<2,plain,512>"
RELU = R.ACT_RELU
NCU = torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256

Case = collections.namedtuple("Case", "M K a pad ldc_pad epi feed")
E_NONE = Epi()
E_BIAS = Epi(bias=True)
E_RELU = Epi(alpha=0.5, bias=True, act0=RELU)
E_CPL = Epi(bias=True, act0=RELU, cplanes="yes")


def cases():
    out = []
    for a in (2, 1):
        out += [Case(512, 64, a, 0, 0, E_NONE, "none"),                 # one tile
                Case(1024, 96, a, 0, 0, E_RELU, "stale"),               # two workgroups, three chunks
                Case(512 * 9, 128, a, 0, 0, E_BIAS, "none"),            # tile_of's `rem` branch, four chunks
                Case(512 * (NCU + 1), 64, a, 0, 0, E_RELU, "none"),     # one workgroup walks two tiles
                Case(512, 160, a, 8, 4, E_BIAS, "stale"),               # five chunks, pitch > K, ldc > N
                Case(1024, 64, a, 8, 0, E_CPL, "none")]                 # planes of the result beside C
    return out


def case_id(c):
    e = c.epi
    return f"M{c.M}-K{c.K}-a{c.a}-pad{c.pad}-ldc{c.ldc_pad}-" + ("relu" if e.act0 else "bias" if e.bias else "none") + ("-cpl" if e.cplanes != "no" else "") + "-" + c.feed


_INPUTS, _REFS = {}, {}


def inputs(M, K, a, epi, vals="int"):
    key = (M, K, a, epi, vals)
    if key not in _INPUTS:
        make = R.int_operand if vals == "int" else R.split_operand
        _INPUTS[key] = dict(a=make(M, K, a == 1, 21), b=make(N, K, False, 22), d=R.epi_data(M, N, epi, K))
    return _INPUTS[key]


def reference(c):
    key = (c.M, c.K, c.a, c.epi)
    if key not in _REFS:
        inp = inputs(c.M, c.K, c.a, c.epi)
        _REFS[key] = R.apply_epilogue(R.contract(inp["a"], inp["b"], "NT"), inp["d"], c.epi)
    return _REFS[key]


def launch(ops, inp, M, K, tile, name, pad=0, ldc_pad=0, epi=E_NONE, feed="none"):
    """One forced-tile launch with both operands as planes only -> (whole C buffer, c_hi, c_lo)."""
    apl, bpl = R.place_planes(inp["a"], pad), R.place_planes(inp["b"], pad)
    A = B = None
    if feed == "stale":                                   # an fp32 image full of NaN that the launch must not read
        A, B = R.place_image(inp["a"], K + pad, nan=True), R.place_image(inp["b"], K + pad, nan=True)
        apl.fp32_stale = bpl.fp32_stale = True
    out, buf = R.place_out(M, N, ldc_pad)
    cpl = wide = None
    if epi.cplanes != "no":
        wide = [torch.full((M, N + ldc_pad), 55.0, dtype=torch.bfloat16).to(DEV) for _ in range(2)]
        cpl = ops.Planes(wide[0][:, :N], wide[1][:, :N])
    kw = {"bias": inp["d"]["bias"].to(DEV)} if epi.bias else {}
    prof, ops.KERNEL_PROFILE = ops.KERNEL_PROFILE, []
    try:
        got = ops.gemm(A, B, True, True, M, N, K, out=out, ldc=out.stride(0), act0=epi.act0, alpha=epi.alpha, splits=1, tile=tile,
                       a_planes=apl, b_planes=bpl, c_planes=cpl, **kw)
        launched = [rec[0] for rec in ops.KERNEL_PROFILE]
    finally:
        ops.KERNEL_PROFILE = prof
    assert got is out
    assert launched == [name], launched
    torch.cuda.synchronize()
    return buf.cpu(), (None if wide is None else [w.cpu() for w in wide])


@pytest.fixture(scope="module")
def ops():
    from advmil_amd import _lib, ops as O
    _lib.lib()
    prev = O.get_gemm_mode()
    O.set_gemm_mode("bf16x3")
    yield O
    O.set_gemm_mode(prev)


@pytest.mark.parametrize("c", cases(), ids=case_id)
def test_tile_87_walks(ops, c):
    inp, ref = inputs(c.M, c.K, c.a, c.epi), reference(c)
    buf, wide = launch(ops, inp, c.M, c.K, TILE, NAME, c.pad, c.ldc_pad, c.epi, c.feed)
    assert bool((buf[:, N:] == 77.0).all()), "pad columns of the output were written"
    C = buf[:, :N].double()
    assert torch.equal(C, ref["C"]), (case_id(c), int((C != ref["C"]).sum()), float((C - ref["C"]).abs().max()))
    if wide is not None:
        for w, k in zip(wide, ("c_hi", "c_lo")):
            assert bool((w[:, N:].float() == 55.0).all())
            assert torch.equal(w[:, :N].double(), ref[k]), (case_id(c), k)


@pytest.mark.parametrize("a", (2, 1), ids=("a2", "a1"))
def test_tile_87_is_bit_identical_to_tile_82(ops, a):
    """Random-valued operands (true splits of randn), bias + ReLU, five tiles of 512 rows against ten of 256, six chunks."""
    M, K = 512 * 5, 192
    inp = inputs(M, K, a, E_RELU, "randn")
    wide87, _ = launch(ops, inp, M, K, 87, NAME, epi=E_RELU)
    wide82, _ = launch(ops, inp, M, K, 82, "gemm_nt_planes_kernel<2>", epi=E_RELU)
    assert bool(torch.isfinite(wide87).all()) and float(wide87.abs().max()) > 0.0
    assert torch.equal(wide87, wide82), int((wide87 != wide82).sum())
