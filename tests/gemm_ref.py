"""float64 restatements of the contraction engine's bf16x3 arithmetic (csrc/gemm_core.h), shared by tests/test_gemm_walks_gpu.py,
tests/test_gemm_walks_plan_cpu.py and tests/test_poison_kernels_gpu.py. Nothing here is shared with the kernels.

The kernels take operand planes as given: `hi` and `lo` are two independent bf16 arrays, and what they compute, in fp32, is

    C = epi( sum_k  al bh + ah bl + ah bh )

(`al bl` is never formed; a single-plane operand has lo == 0). An operand that is NOT read from its planes is split on the fly from
its fp32 image x: hi = bf16(x), lo = bf16(x - hi). With planes of independent small integers the two paths give different numbers --
x = hi + lo is itself a small integer, so its split is (x, 0) and the product gains the `al bl` term -- and every product and partial
sum is an integer below 2^24, exact in fp32 in any order: the result must EQUAL the float64 evaluation here. The epilogue stays
exact with alpha in {1, 0.5}, integer side data, ReLU, mask_scale = 2 and p = 0.5.

Operands are built in their STORAGE layout, [rows, extent]: [M | N, K] when k-contiguous, [K, M | N] when not."""
import collections

import torch

DEV = "cuda:0"
ACT_NONE, ACT_RELU = 0, 1
LAYOUTS = {"NT": (True, True), "NN": (True, False), "TN": (False, False), "TT": (False, True)}      # (a_kc, b_kc)
INT_RANGE = 7

# what the epilogue of a launch does; the side data itself (bias values, masks, ...) comes from epi_data()
Epi = collections.namedtuple("Epi", "alpha bias act0 act1 act_split accumulate maskref rowv rowseg maskbits colsum drop cplanes n_split bias2")
Epi.__new__.__defaults__ = (1.0, False, ACT_NONE, None, None, False, False, False, False, False, False, False, "no", 0, False)
MASK_SCALE = 2.0
DROP_P, DROP_SEED, DROP_SID = 0.5, 1234, 3
NSEG = 3


def _gen(*key):
    s = 17
    for k in key:
        s = (s * 1000003 + int(k)) % ((1 << 31) - 1)
    return torch.Generator().manual_seed(s)


def _ints(shape, g, lo=-INT_RANGE, hi=INT_RANGE):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


class Operand:
    """One operand in storage layout: hi / lo as float64 CPU tensors holding bf16-representable values (lo None: single plane);
    x: the fp32 matrix the planes were split from (true splits), else None (integer planes: the fp32 image is hi + lo)."""

    def __init__(self, hi, lo, x=None):
        self.hi, self.lo, self.x = hi, lo, x

    @property
    def single(self):
        return self.lo is None

    def image(self):
        """The operand's fp32 image."""
        if self.x is not None:
            return self.x.clone()
        return (self.hi if self.lo is None else self.hi + self.lo).float()

    def effective(self, from_planes, kc, dtype=torch.float64):
        """(hi, lo) as the kernel sees them, logical orientation [M | N, K]: the planes as given, or the on-the-fly split of the image."""
        if from_planes:
            hi, lo = self.hi, (torch.zeros_like(self.hi) if self.lo is None else self.lo)
        else:
            hi, lo = split_bf16(self.image())
        hi, lo = (hi, lo) if kc else (hi.t(), lo.t())
        return hi.to(dtype), lo.to(dtype)


def split_bf16(x32):
    """hi = bf16(x), lo = bf16(x - hi), round to nearest even on the host; both as float64."""
    x32 = x32.float()
    hi = x32.to(torch.bfloat16)
    lo = (x32 - hi.float()).to(torch.bfloat16)
    return hi.double(), lo.double()


def int_operand(rows, ext, single, *key):
    """Independent small integers in [-7, 7], one stream per plane."""
    return Operand(_ints((rows, ext), _gen(1, rows, ext, *key)), None if single else _ints((rows, ext), _gen(2, rows, ext, *key)))


def split_operand(rows, ext, single, *key, scale=1.0):
    """True split of randn. Single plane: the matrix IS bf16 (x = hi)."""
    x = scale * torch.randn(rows, ext, generator=_gen(3, rows, ext, *key))
    hi, lo = split_bf16(x)
    if single:
        return Operand(hi, None, hi.float())
    return Operand(hi, lo, x)


def contract(a, b, lay, a_from_planes=True, b_from_planes=True, dtype=torch.float64):
    """sum_k al bh + ah bl + ah bh over the operands as the kernel sees them -> [M, N]."""
    a_kc, b_kc = LAYOUTS[lay]
    ah, al = a.effective(a_from_planes, a_kc, dtype)
    bh, bl = b.effective(b_from_planes, b_kc, dtype)
    return al @ bh.t() + ah @ bl.t() + ah @ bh.t()


def true_product(a, b, lay):
    """float64 product of the fp32 images."""
    a_kc, b_kc = LAYOUTS[lay]
    A, B = a.image().double(), b.image().double()
    return (A if a_kc else A.t()) @ (B.t() if b_kc else B)


# ------------------------------------------------------------------------------------------------------------------------------
# the epilogue
# ------------------------------------------------------------------------------------------------------------------------------
def epi_data(M, N, e, *key):
    """Integer side data of an exact epilogue (CPU tensors; dtype as the launch wants them)."""
    g = _gen(4, M, N, *key)
    d = {}
    if e.bias:
        d["bias"] = _ints((N,), g).float()
    # (two-layer form: one [N] vector here; the launch hands its tail over as bias2)
    if e.accumulate:
        d["C0"] = _ints((M, N), g, -50, 50).float()
    if e.maskref:
        d["maskref"] = _ints((M, N), g, -3, 3).float()                     # the mask is the SIGN: zeros and negatives drop
    if e.rowv:
        d["rowv"] = _ints((M,), g, -3, 3).float()
        d["colv"] = _ints((NSEG if e.rowseg else 1, N), g, -3, 3).float()
        if e.rowseg:
            d["rowseg"] = torch.randint(0, NSEG, (M,), generator=g).to(torch.int32)
    if e.maskbits:
        d["maskbits"] = torch.randint(-(1 << 31), 1 << 31, (M, N // 32), generator=g).to(torch.int32)
    if e.drop:
        from advmil_amd import synth
        d["keep"] = torch.from_numpy(synth.dropout_keep(DROP_SEED, DROP_SID, M * N, DROP_P).reshape(M, N))
    return d


def unpack_bits(words, N):
    """[M, N / 32] int32 words -> [M, N] bool, bit (n & 31) of word n >> 5."""
    w = words.to(torch.int64) & 0xFFFFFFFF
    sh = torch.arange(32, dtype=torch.int64)
    return ((w[:, :, None] >> sh) & 1).reshape(words.shape[0], -1)[:, :N].bool()


def apply_epilogue(acc, d, e, dtype=torch.float64):
    """csrc/gemm_core.h::epilogue_elem and the streaming form, restated: alpha, bias, rank-1 term, activation, dropout, masks, accumulate.
    -> dict(C [M, N] (every column: the two-layer form's second layer is C[:, n_split:]), keep, c_hi, c_lo, colsum)."""
    M, N = acc.shape
    v = acc.to(dtype) * e.alpha
    if e.bias:
        v = v + d["bias"].to(dtype)
    if e.rowv:
        colv = d["colv"].to(dtype)
        v = v + d["rowv"].to(dtype)[:, None] * (colv[d["rowseg"].long()] if e.rowseg else colv[0][None, :])
    act1 = e.act0 if e.act1 is None else e.act1
    split = N if e.act_split is None else e.act_split
    cols = torch.arange(N)
    relu = torch.where(cols < split, torch.tensor(e.act0 == ACT_RELU), torch.tensor(act1 == ACT_RELU))
    v = torch.where(relu[None, :], torch.relu(v), v)
    out = {}
    if e.drop:
        out["keep"] = d["keep"]
        v = torch.where(d["keep"], 2.0 * v, torch.zeros_like(v))
    if e.maskref:
        v = v * torch.where(d["maskref"] > 0, MASK_SCALE, 0.0).to(dtype)
    if e.accumulate:
        v = v + d["C0"].to(dtype)
    if e.maskbits:
        v = v * torch.where(unpack_bits(d["maskbits"], N), MASK_SCALE, 0.0).to(dtype)
    out["C"] = v
    if e.cplanes != "no":
        n1 = e.n_split or N
        out["c_hi"], out["c_lo"] = split_bf16(v[:, :n1].float())
    if e.colsum:
        out["colsum"] = v.reshape(M // 64, 64, N).sum(1)                    # one partial row per 64 rows (a wave's 32 TM rows, TM = 2)
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# device placement: planes as column slices of wider allocations
# ------------------------------------------------------------------------------------------------------------------------------
def place_planes(op, pad=0, off=0, poison_pad=True):
    """ops.Planes of the operand on the device, each plane the column slice [:, off : off + extent] of its own
    [rows, off + extent + pad] bf16 allocation (row pitch > extent; the other columns hold NaN). off = 8 k keeps the base 16-byte
    aligned; off = 4 puts it 8 bytes off."""
    from advmil_amd import ops

    def one(p):
        rows, ext = p.shape
        wide = torch.full((rows, off + ext + pad), float("nan") if poison_pad else 0.0, dtype=torch.bfloat16)
        wide[:, off:off + ext] = p.to(torch.bfloat16)
        v = wide.to(DEV)[:, off:off + ext]
        assert v.stride(0) == off + ext + pad and v.data_ptr() % 16 == (2 * off) % 16
        return v
    return ops.Planes(one(op.hi), None if op.lo is None else one(op.lo))


def place_image(op, pitch, nan):
    """The fp32 image on the device with the planes' row pitch; nan: NaN in every element (the launch must not read it)."""
    rows, ext = op.hi.shape
    wide = torch.full((rows, pitch), float("nan"), dtype=torch.float32)
    if not nan:
        wide[:, :ext] = op.image()
    v = wide.to(DEV)[:, :ext]
    assert v.stride(0) == pitch and v.data_ptr() % 16 == 0
    return v


def place_out(M, N, pad, c0=None, off_float=0, fill=77.0):
    """An [M, N] fp32 output view: columns [:N] of an [M, N + pad] buffer (pad columns hold `fill`), or, off_float = 1, a dense view
    one float into its buffer (4 bytes off 16-byte alignment). -> (view, whole buffer)."""
    if off_float:
        assert not pad
        buf = torch.full((M * N + 8,), fill).to(DEV)
        v = buf[off_float:off_float + M * N].view(M, N)
        assert v.data_ptr() % 16 == 4 * off_float
    else:
        buf = torch.full((M, N + pad), fill).to(DEV)
        v = buf[:, :N]
        assert v.data_ptr() % 16 == 0
    if c0 is not None:
        v.copy_(c0.to(DEV))
    return v, buf


def relerr(got, want):
    got = got.detach().cpu().double(); want = want.detach().cpu().double()
    return float((got - want).abs().max() / (want.abs().max() + 1e-30))
