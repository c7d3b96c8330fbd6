"""advmil_stage_bag_masked (include/advmil_hip.h; csrc/optim.hip) against torch: the staging launch of a cached bag with a keep
bitmap over its 16-row regions -- kept regions copied (planes copied or derived), masked regions WRITTEN as zeros in the rows and in
both planes, nothing outside the destination touched, the source of the out-of-place forms left as it was. Every form of the entry
point, region counts that put a word boundary inside the bitmap, both row widths' ends (C = 8: one 32-byte unit per row, the split
form's minimum; C = 1024: the product's), under both allocation-poison patterns (tests/poison.py)."""
import ctypes

import numpy as np
import pytest
import torch

from tests.poison import poison  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GUARD = 16                     # rows in front of and behind every destination, filled with SENTINEL
SENTINEL = 0x5A


def patterns(R):
    """all / none but region 0 / none but the last / alternating / only bits 31 and 32 (those of them the bag has)."""
    return {"all": np.arange(R), "first": np.array([0]), "last": np.array([R - 1]), "alternating": np.arange(0, R, 2),
            "bits31_32": np.array([r for r in (31, 32) if r < R], dtype=np.int64)}


def guarded(rows, C, dtype):
    """A destination of `rows` rows inside a sentinel-filled block, GUARD rows on either side -> (block, destination view)."""
    blk = torch.empty(rows + 2 * GUARD, C, dtype=dtype, device=DEV)
    blk.view(torch.uint8).fill_(SENTINEL)
    return blk, blk[GUARD:GUARD + rows]


def guards_intact(blk):
    b = blk.view(torch.uint8)
    return bool((b[:GUARD] == SENTINEL).all()) and bool((b[-GUARD:] == SENTINEL).all())


def bits_of(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


@pytest.mark.parametrize("R", [1, 2, 33, 65])
@pytest.mark.parametrize("C", [8, 1024])
def test_masked_staging_every_form(poison, C, R):  # noqa: F811
    from advmil_amd import _lib, ops
    from advmil_amd.utils.func import keep_bitmap
    L = _lib.lib()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    n = 16 * R
    g = torch.Generator().manual_seed(100 * C + R)
    x = torch.randn(n, C, generator=g).to(DEV)
    xb = x.to(torch.bfloat16)
    x_planes = ops.split_planes(x)
    x0, xb0, xh0, xl0 = x.clone(), xb.clone(), x_planes.hi.clone(), x_planes.lo.clone()
    P = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())      # noqa: E731

    def run(dst, src, hi, shi, lo, slo, bits):
        esz = src.element_size()
        rc = L.advmil_stage_bag_masked(P(dst), P(src), n * C * esz, n, P(hi), P(shi), P(lo), P(slo), 0 if hi is None else n * C * 2, P(bits), st)
        assert rc == 0, rc

    for name, keep in patterns(R).items():
        bits = torch.from_numpy(keep_bitmap(keep, R).view(np.int32)).to(DEV)
        keep_rows = torch.zeros(R, dtype=torch.bool)
        keep_rows[torch.from_numpy(keep)] = True
        keep_rows = keep_rows.repeat_interleave(16).to(DEV).unsqueeze(1)
        want = torch.where(keep_rows, x, torch.zeros_like(x))
        want_b = torch.where(keep_rows, xb, torch.zeros_like(xb))
        want_pl = ops.split_planes(want)

        def check(rows, hi, lo, blocks, what, w=want):
            if rows is not None:
                assert torch.equal(rows, (x if w is want else xb) * keep_rows), (name, what, "rows")
                assert torch.equal(bits_of(rows), bits_of(w)), (name, what, "rows: masked regions are zeros, kept regions the source's bits")
            if hi is not None:
                assert torch.equal(bits_of(hi), bits_of(want_pl.hi)), (name, what, "hi")
                assert torch.equal(bits_of(lo), bits_of(want_pl.lo)), (name, what, "lo")
            for blk in blocks:
                assert guards_intact(blk), (name, what, "guard")

        # (a) fp32 rows -> fp32 rows + derived planes
        rb, r = guarded(n, C, torch.float32)
        hb, h = guarded(n, C, torch.bfloat16)
        lb, l = guarded(n, C, torch.bfloat16)
        run(r, x, h, None, l, None, bits)
        check(r, h, l, (rb, hb, lb), "a")
        # (b) planes only: dst_rows = NULL
        hb, h = guarded(n, C, torch.bfloat16)
        lb, l = guarded(n, C, torch.bfloat16)
        run(None, x, h, None, l, None, bits)
        check(None, h, l, (hb, lb), "b")
        # (c) rows + held planes copied
        rb, r = guarded(n, C, torch.float32)
        hb, h = guarded(n, C, torch.bfloat16)
        lb, l = guarded(n, C, torch.bfloat16)
        run(r, x, h, x_planes.hi, l, x_planes.lo, bits)
        check(r, h, l, (rb, hb, lb), "c")
        # the sources of the out-of-place forms are as they were
        assert torch.equal(bits_of(x), bits_of(x0)) and torch.equal(bits_of(x_planes.hi), bits_of(xh0)) and torch.equal(bits_of(x_planes.lo), bits_of(xl0))
        # (d) rows only, 2-byte elements; and fp32 rows only (the exact mode's slab, the back-fill of a planes-only span)
        rb, r = guarded(n, C, torch.bfloat16)
        run(r, xb, None, None, None, None, bits)
        check(r, None, None, (rb,), "d", want_b)
        assert torch.equal(bits_of(xb), bits_of(xb0))
        rb, r = guarded(n, C, torch.float32)
        run(r, x, None, None, None, None, bits)
        check(r, None, None, (rb,), "d fp32")
        # (e) in place: fp32 with planes, fp32 rows alone, 2-byte rows alone
        rb, r = guarded(n, C, torch.float32)
        r.copy_(x)
        hb, h = guarded(n, C, torch.bfloat16)
        lb, l = guarded(n, C, torch.bfloat16)
        run(r, r, h, None, l, None, bits)
        check(r, h, l, (rb, hb, lb), "e planes")
        rb, r = guarded(n, C, torch.float32)
        r.copy_(x)
        run(r, r, None, None, None, None, bits)
        check(r, None, None, (rb,), "e fp32")
        rb, r = guarded(n, C, torch.bfloat16)
        r.copy_(xb)
        run(r, r, None, None, None, None, bits)
        check(r, None, None, (rb,), "e bf16", want_b)
    torch.cuda.synchronize()
