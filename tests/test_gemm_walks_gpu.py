"""GPU: every walk of the plane-fed contraction kernels (csrc/gemm_host.hip, gemm_nt_planes.hip, gemm_tn_planes.hip, the register-staged
planes of gemm_f32.hip, gemm_core.h) against an oracle that shares nothing with them (tests/gemm_ref.py).

The exact cases fill all four operand planes with independent small integers: every product and partial sum of
`al bh + ah bl + ah bh` is then an integer below 2^24, exact in fp32 in any order, and the result must be EQUAL (torch.equal) to the
float64 evaluation of that formula and of an epilogue kept exact (alpha 1 / 0.5, integer bias / rank-1 / accumulate data, ReLU,
mask_scale 2, p = 0.5). A dropped product, a swapped plane, a mis-swizzled 16-byte unit, a stale ring slot or a tile written twice
shows at full magnitude. Where the host mirror says an operand is read from its planes, the launch is handed an fp32 image full of NaN
(ops.gemm(None, ...), B=None or Planes.fp32_stale); where it says the planes are not usable, the expected value is the on-the-fly split
of the fp32 image, which with integer planes is a different number (it gains `al bl`).

Each case names its walk and ASSERTS IT ON THE HOST, before the launch, with the plain-Python mirrors below (`plan`): planes_usable,
the PRE dispatch of advmil_launch_generic, the NT tile table, tile_of and the persistent grid, the TN split / group arithmetic and which
reduce runs. tests/test_gemm_walks_plan_cpu.py pins the mirrors' constants to the source text and to the library's host-only
arithmetic. `test_every_walk_is_reached` fails if the parametrisation loses a walk.

Walks (tags of `plan`):
  plane-fed NT  tile 82 / 83 / 85 / 86 x A two-plane | single-plane (EPI_IN_SLOT false on every single-plane form); K / 32 = 2 .. 5;
                one tile per workgroup at mtiles < 8, mtiles % 8 == 0, mtiles = 9 (the `rem` branch of tile_of); 1 / 2 and 2 / 3 tiles
                per workgroup (sized from the device's CU count), one with a negative dB; pitch > K, ldc > N; the streaming, the plain
                streaming and the generic epilogue -- the last also inside a multi-tile walk (act_split % 32 != 0, an output 4 bytes off
                alignment, rowv + accumulate); the two-layer form with and without fp32 C. Tile 84: the gate score, within tolerance.
  plane-fed TN  tile 91 / 92 / 93 x B two-plane | single-plane; chunks per split (3), (4, 3), (3, 3, 1), (3, 3, 2); by_m true / false;
                one and two rounds of eight groups; pitch > M, > N; direct epilogue, reduce kernel, merge queue.
  register-staged planes  tiles 22 / 12 / 11 x PRE 1 / 2 / 3 x NT / NN / TN / TT, two- and single-plane, ragged shapes, splits 1 / 3;
                tile 43 PRE 1 (NN, TN); tiles 34 / 24 PRE 2 / 3 (TN), with the predicated tail of the 192-row tile; and the dispatch
                holes, where the fp32 image is read although planes were given: tile 43 with both planes, tile 23, an extent that is
                no multiple of 8, a plane base off 16 bytes.

Random-valued cases (true splits of randn), one per family: error against the float64 of the planes formula, bound 4 e32 (e32 = the
same restatement evaluated in float32 on the host against its float64 self; 4 for the summation order), and the project's 2e-5 of
max|want| against the true product. Never a figure taken from the kernels.

Measured on an MI355X (256 CUs) when this file was written: all 248 integer-valued cases pass (240 under torch.equal, the 8 dropout
cases under their rule: dropped entries 0, kept entries within 2^-23 of 2 v); the whole file runs in 6 s (257 tests, the largest --
131 840 rows, 2 / 3 tiles per workgroup -- 0.5 s). Random-valued cases, error / bound in force (every case
prints its figures; `test_every_walk_is_reached` prints the worst of each family):
  plane-fed NT            against the planes formula 2.90e-7 of 4 e32 = 9.9e-7 (0.29; tile 83, K = 160) and 1.70e-7 of 7.4e-7 (0.23; tile
                          86, single-plane A); against the true product 4.5e-6 / 2.7e-6 of 2e-5 (0.23)
  plane-fed TN            1.51e-7 of 6.9e-7 (0.22; tile 93, three splits) and 1.64e-7 of 8.5e-7 (0.19; tile 91, single-plane B); true
                          product 4.5e-6 / 2.7e-6 of 2e-5 (0.23)
  register-staged planes  1.48e-7 of 4.7e-7 (0.32; tile 22 NN) and 1.54e-7 of 7.1e-7 (0.22; tile 34, three splits); true product
                          5.1e-6 / 4.1e-6 of 2e-5 (0.26)
  gate score, tile 84     2.2e-6 and 4.9e-6 of 2e-5 absolute (0.25)
(The distance to the true product is the 2^-17 of the dropped `al bl` terms, not rounding: the float64 restatement of the planes formula
is as far from it, 2.7e-6 .. 5.0e-6 on the same cases.)

Value-only, in-bounds mutants of a scratch copy of the kernels, each run once against this file:
  the `al bh` MFMA of gemm_nt_planes_kernel dropped        all 67 two-plane cases of test_plane_fed_nt_walks and both cases of
                                                           test_plane_fed_gate_score_tile fail; the 65 single-plane cases, whose
                                                           instantiation never had that product, pass
  the a_lo pieces of the TN kernel's `dma` read a_hi       all 28 cases of test_plane_fed_tn_walks fail
  `^ (krow & 3)` dropped from the TN source swizzle        all 28 cases of test_plane_fed_tn_walks fail

Found by this file:
  * ops.gemm moved a launch whose B planes carry `fp32_stale` off the plane-fed NT tiles 82 .. 86 onto tile 22 (its list of kernels
    that read B from its planes named 91 .. 93 and the register-staged forms only). The values are the same, so nothing noticed: the
    cases here handed tile 83 a stale B, the mirror said "plane-fed NT kernel", and the launch was refused for its column sums, which
    tile 22 cannot give at N = 192. ops.gemm now leaves a two-plane stale B on 82 .. 86, as it leaves B=None there, and every case
    asserts the name of the kernel ops.gemm actually launched (ops.KERNEL_PROFILE) against the mirror.
  * The two-layer form (c2 / n_split, tiles 85 / 86) is routed by the plain STREAMING epilogue only; the generic fallback knows nothing
    of c2 and would store the second layer's columns into C behind column n_split, past the end of its last row. The host accepted such
    a launch with an output off 16-byte alignment, ldc % 4 != 0, a bias off alignment or emitted planes off 8 bytes. Found while writing
    the mirror (no case was built to run it); advmil_gemm_f32_tiled now refuses these, and tests/test_gemm_walks_plan_cpu.py asks it to.
"""
import collections
import ctypes
import itertools

import pytest
import torch

from tests import gemm_ref as R
from tests.gemm_ref import Epi

pytestmark = pytest.mark.gpu
DEV = R.DEV

# ------------------------------------------------------------------------------------------------------------------------------
# constants copied from csrc/ (tests/test_gemm_walks_plan_cpu.py pins them to the source text)
# ------------------------------------------------------------------------------------------------------------------------------
BK, PITCH_KC = 32, 36
NT_MIN_K = 64                                        # the three-slot ring prefetches two chunks ahead
TN_MIN_CHUNKS = 3
# tile -> (TN, NBUF, EPI) of gemm_nt_planes_kernel (WR = 4, BKT = 32); ALO = 0 instantiations exist for NT_SINGLE
NT_TABLE = {84: (4, 2, 1), 85: (4, 2, 2), 86: (2, 3, 2), 83: (3, 2, 0), 82: (2, 3, 0)}
NT_SINGLE = (85, 86, 83, 82)
# tile -> (TM, TN, WR, WC, NBUF) of gemm_tn_planes_kernel, both BLO forms
TN_TABLE = {91: (2, 2, 2, 4, 3), 92: (2, 2, 4, 2, 3), 93: (2, 4, 4, 2, 2)}
PLANES_TILES = (22, 12, 11)                          # launch_tile<.., PLANES = true>: every PRE in every layout
GENERIC_GEOM = {23: (2, 3, 2, 2), 22: (2, 2, 2, 2), 13: (1, 3, 2, 2), 12: (1, 2, 2, 2), 11: (1, 1, 2, 2), 43: (2, 3, 4, 2),
                42: (2, 2, 4, 2), 34: (3, 2, 2, 4), 24: (2, 2, 2, 4)}      # tile -> (TM, TN, WR, WC)
NOMINAL_CUS = 256


def device_cus():
    return torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else NOMINAL_CUS


def ceil_div(a, b):
    return -(-a // b)


def epi_wave_floats(tm, tn):
    return 32 * PITCH_KC + 32 * (tn + 2 * tm) + 32 * tm * tn


def planes_usable(nplanes, base_off, ld, extent):
    """csrc/gemm_host.hip::planes_usable: hi given, both bases 16-byte aligned, pitch and contiguous extent multiples of 8 halfwords.
    base_off: halfwords from a 16-byte boundary to the planes' first element."""
    return nplanes > 0 and (2 * base_off) % 16 == 0 and ld % 8 == 0 and extent % 8 == 0


def generic_pre(tile, a_kc, b_kc, pre):
    """Which of the usable planes advmil_launch_generic's instantiation for this tile and layout actually stages (bit 1: A, bit 2: B)."""
    if tile in PLANES_TILES:
        return pre
    if tile == 43:
        return 1 if pre == 1 and not b_kc else 0
    if tile in (34, 24):
        return pre if pre in (2, 3) and not a_kc and not b_kc else 0
    return 0


def tile_of(v, mtiles, ntiles):
    """The persistent NT kernel's tile order -> (mt, nt, took the `rem` branch)."""
    per_group, full = 8 * ntiles, (mtiles // 8) * 8 * ntiles
    if v < full:
        r = v % per_group
        return (v // per_group) * 8 + (r & 7), r >> 3, False
    rem, r = mtiles - (mtiles // 8) * 8, v - full
    return (mtiles // 8) * 8 + r % rem, r // rem, True


def nt_walk(mtiles, ntiles, ncu):
    """grid = min(ntile, CUs); per workgroup the tiles v, v + grid, ...: how many, and the sign of the row deltas between them."""
    ntile = mtiles * ntiles
    grid = min(ntile, ncu)
    counts, neg_db, neg_da, rem = set(), False, False, False
    for v0 in range(grid):
        seq = [tile_of(v, mtiles, ntiles) for v in range(v0, ntile, grid)]
        counts.add(len(seq))
        rem |= any(t[2] for t in seq)
        for (m0, n0, _), (m1, n1, _) in zip(seq, seq[1:]):
            neg_db |= n1 < n0
            neg_da |= m1 < m0
    assert sorted((m, n) for v in range(ntile) for m, n, _ in [tile_of(v, mtiles, ntiles)]) == sorted(itertools.product(range(mtiles), range(ntiles)))
    return grid, frozenset(counts), neg_db, neg_da, rem


def tn_split(K, splits):
    """advmil_gemm_f32_tiled's split arithmetic -> (splits, k_chunk, chunks per split)."""
    kchunks = ceil_div(K, BK)
    splits = max(1, min(splits, kchunks))
    k_chunk = ceil_div(kchunks, splits) * BK
    splits = ceil_div(K, k_chunk)
    return splits, k_chunk, tuple((min(K, (z + 1) * k_chunk) - z * k_chunk) // BK for z in range(splits))


def tn_groups(tile, M, N, splits):
    """(gs, og, grid, by_m, rounds of eight groups) of the plane-fed TN launch."""
    bm, bn = (128 if tile == 91 else 256), (128 if tile == 92 else 256)
    mt, nt = M // bm, N // bn
    by_m = M >= N
    gs, og = (nt, mt) if by_m else (mt, nt)
    return gs, og, 8 * ceil_div(splits * og, 8) * gs, by_m, ceil_div(splits * og, 8)


def reduce_kind(splits, e, ldc, N, c_aligned=True):
    """direct epilogue | the merge queue (the trivial accumulate) | gemm_splitk_reduce_kernel."""
    if splits == 1:
        return "direct"
    plain = (e.accumulate and e.alpha == 1.0 and not e.bias and not e.rowv and not e.maskref and e.act0 == 0 and not e.act1 and not e.drop
             and e.cplanes == "no" and ldc == N and N % 4 == 0 and c_aligned and splits <= 64)
    return "merge" if plain else "kernel"


def nt_epilogue(tile, e, ldc, c_aligned):
    """Which epilogue the persistent kernel takes: `stream` (EPI 0), `plain` (EPI 2) or the `generic` fallback. M and N are whole
    tiles and every side vector is 16-byte aligned in these tests, so what is left of gemm_epilogue's `stream` test is:"""
    nmode = 1 if (e.rowv and e.maskref and not e.accumulate) else int(e.rowv) + int(e.maskref) + int(e.accumulate)
    split = (1 << 30) if e.act_split is None else e.act_split
    stream = ldc % 4 == 0 and c_aligned and split % 32 == 0 and nmode <= 1
    if NT_TABLE[tile][2] == 1:
        return "generic"
    if not stream:
        return "generic"
    return "plain" if NT_TABLE[tile][2] == 2 else "stream"


Case = collections.namedtuple("Case", "fam tile lay M N K a b a_pad b_pad a_off ldc_pad c_off splits epi vals feed want")
Case.__new__.__defaults__ = (0, 0, 0, 0, 0, 1, Epi(), "int", "none", ())
Plan = collections.namedtuple("Plan", "kernel a_src b_src tags")


def pitches(c):
    a_kc, b_kc = R.LAYOUTS[c.lay]
    a_ext, b_ext = (c.K if a_kc else c.M), (c.K if b_kc else c.N)
    return a_ext, b_ext, c.a_off + a_ext + c.a_pad, b_ext + c.b_pad


def plan(c, ncu=NOMINAL_CUS):
    """The host dispatch of advmil_gemm_f32_tiled in bf16x3 mode, mirrored: which kernel runs, which operands it reads from their
    planes, and the tags of the walk. None where the host refuses the launch."""
    a_kc, b_kc = R.LAYOUTS[c.lay]
    e = c.epi
    a_ext, b_ext, lda, ldb = pitches(c)
    n_out = e.n_split or c.N
    ldc = n_out + c.ldc_pad
    if lda % 4 or ldb % 4 or a_ext % 4 or b_ext % 4:
        return None
    splits, k_chunk, chunks = tn_split(c.K, c.splits)
    if splits > 1 and c.N % 4:
        return None
    pre = (1 if planes_usable(c.a, c.a_off, lda, a_ext) else 0) | (2 if planes_usable(c.b, 0, ldb, b_ext) else 0)
    tags = set()
    if 82 <= c.tile <= 86:
        tn_, nbuf, epi_kind = NT_TABLE[c.tile]
        plain = epi_kind == 2
        if c.tile == 84 and c.fam != "gate":
            return None
        if plain and (e.rowv or e.maskref or e.accumulate or e.drop or e.maskbits or e.colsum):
            return None
        if e.n_split and (not plain or e.n_split >= c.N or e.n_split % 32 or e.act_split != e.n_split):
            return None
        if e.n_split and (ldc % 4 or c.c_off):         # the second layer is routed by the plain streaming epilogue only
            return None
        if not (a_kc and b_kc) or pre != 3 or splits != 1 or c.M % 256 or c.K % 32 or c.N % (64 * tn_) or c.K < NT_MIN_K:
            return None
        if c.M * lda * 2 >= 1 << 32 or c.N * ldb * 2 >= 1 << 32 or c.b != 2 or (c.a == 1 and c.tile not in NT_SINGLE):
            return None
        alo = 1 if c.a == 2 else 0
        buf_hw = ((1 + alo) * 256 + 2 * 64 * tn_) * 32
        in_slot = 8 * epi_wave_floats(2, tn_) <= buf_hw // 2
        assert in_slot or alo == 0
        mtiles, ntiles = c.M // 256, c.N // (64 * tn_)
        grid, counts, neg_db, neg_da, rem = nt_walk(mtiles, ntiles, ncu)
        ep = nt_epilogue(c.tile, e, ldc, c.c_off == 0)
        tags |= {("nt", c.tile, c.a), ("nt_in_slot", in_slot), ("nt_chunks", c.K // 32), ("nt_per_wg", counts), ("nt_nbuf", nbuf),
                 ("nt_epilogue", c.tile, ep), ("nt_ntiles", c.tile, ntiles)}
        if max(counts) > 1:
            tags.add(("nt_multi_epilogue", "plain" if plain else "full", ep,
                      "-" if ep != "generic" else ("act_split" if (e.act_split or 0) % 32 else "c_off" if c.c_off else "rowv+acc")))
        if neg_db:
            tags.add(("nt_dB<0",))
        if rem:
            tags.add(("nt_rem",))
        tags.add(("nt_mtiles", "<8" if mtiles < 8 else "%8" if mtiles % 8 == 0 else "9" if mtiles == 9 else "other"))
        if lda > c.K and ldb > c.K:
            tags.add(("nt_pitch>K",))
        if c.ldc_pad:
            tags.add(("nt_ldc>N",))
        if e.n_split:
            tags.add(("nt_two_layers", c.tile, e.cplanes))
        tags |= epi_tags("nt", c.tile, e)
        return Plan("nt", "planes", "planes", tags)
    if 91 <= c.tile <= 93:
        tm, tn_, wr, wc, nbuf = TN_TABLE[c.tile]
        bm, bn = 32 * tm * wr, 32 * tn_ * wc
        if a_kc or b_kc or pre != 3 or c.M % bm or c.N % bn or c.K % 32 or k_chunk // 32 < TN_MIN_CHUNKS or e.n_split or c.a != 2:
            return None
        if 32 * lda * 2 + c.M * 2 >= 1 << 32 or 32 * ldb * 2 + c.N * 2 >= 1 << 32:
            return None
        gs, og, grid, by_m, rounds = tn_groups(c.tile, c.M, c.N, splits)
        red = reduce_kind(splits, e, ldc, c.N, c.c_off == 0)
        tags |= {("tn", c.tile, c.b), ("tn_chunks", c.tile, chunks), ("tn_by_m", by_m), ("tn_rounds", rounds), ("tn_reduce", red),
                 ("tn_groups", splits * og), ("tn_nbuf", nbuf)}
        if min(chunks) < nbuf:
            tags.add(("tn_short_split", nbuf, min(chunks)))
        if lda > c.M and ldb > c.N:
            tags.add(("tn_pitch",))
        return Plan("tn", "planes", "planes", tags)
    if c.tile not in GENERIC_GEOM:
        return None
    eff = generic_pre(c.tile, a_kc, b_kc, pre)
    tm, tn_, wr, wc = GENERIC_GEOM[c.tile]
    nthreads = 64 * wr * wc
    tags.add(("pre", c.tile, c.lay, eff))
    if eff & 1:
        tags.add(("pre_planes", c.tile, "A", c.a))
        tags.add(("pre_full", (32 * tm * wr * 4) % nthreads == 0))
    if eff & 2:
        tags.add(("pre_planes", c.tile, "B", c.b))
        tags.add(("pre_full", (32 * tn_ * wc * 4) % nthreads == 0))
    if eff:
        tags.add(("pre_splits", c.tile, splits))
        if c.M % (32 * tm * wr) or c.N % (32 * tn_ * wc) or c.K % 32:
            tags.add(("pre_ragged", c.tile))
        else:
            tags.add(("pre_whole", c.tile))
    if (c.a or c.b) and not eff:                     # planes were given and none is read: a dispatch hole
        why = ("base%16" if c.a and c.a_off % 8 else "ext%8" if (c.a and a_ext % 8) or (c.b and b_ext % 8) else
               "43both" if c.tile == 43 and pre == 3 else str(c.tile))
        tags.add(("hole", why))
    return Plan("generic", "planes" if eff & 1 else "fp32", "planes" if eff & 2 else "fp32", tags)


def epi_tags(fam, tile, e):
    t = set()
    for name in ("accumulate", "maskref", "rowv", "rowseg", "maskbits", "colsum", "drop"):
        if getattr(e, name):
            t.add((fam + "_epi", tile, name))
    if e.rowv and e.maskref:
        t.add((fam + "_epi", tile, "rowv+maskref"))
    if e.rowv and e.maskbits:
        t.add((fam + "_epi", tile, "rowv+maskbits"))
    if e.cplanes != "no":
        t.add((fam + "_epi", tile, "cplanes_" + e.cplanes))
    if e.alpha != 1.0:
        t.add((fam + "_epi", tile, "alpha"))
    if e.act_split is not None and not e.n_split:
        t.add((fam + "_epi", tile, "act_split"))
    return t


# ------------------------------------------------------------------------------------------------------------------------------
# the cases
# ------------------------------------------------------------------------------------------------------------------------------
RELU = R.ACT_RELU
E_NONE = Epi()
E_BIAS = Epi(alpha=0.5, bias=True, act0=RELU)
E_SPLIT = Epi(bias=True, act0=RELU, act1=0, act_split=64)
E_CPL = Epi(bias=True, act0=RELU, cplanes="yes")
E_CONLY = Epi(alpha=0.5, bias=True, cplanes="only")
PLAIN_FORMS = (E_NONE, E_BIAS, E_SPLIT, E_CPL, E_CONLY)
FULL_FORMS = (Epi(accumulate=True, bias=True), Epi(maskref=True, bias=True, act0=RELU), Epi(rowv=True), Epi(rowv=True, rowseg=True, alpha=0.5, bias=True),
              Epi(rowv=True, rowseg=True, maskref=True), Epi(maskbits=True, bias=True, act0=RELU), Epi(rowv=True, rowseg=True, maskbits=True),
              Epi(colsum=True, bias=True, act0=RELU), Epi(rowv=True, rowseg=True, maskbits=True, colsum=True), Epi(drop=True, bias=True, act0=RELU),
              Epi(drop=True), Epi(accumulate=True, cplanes="yes"))
E_OFFSPLIT = Epi(bias=True, act0=RELU, act1=0, act_split=48)          # act_split % 32 != 0: the generic epilogue
E_ROWACC = Epi(rowv=True, rowseg=True, accumulate=True)                # two per-element operands: the generic epilogue
NT_WIDTH = {82: 128, 83: 192, 85: 256, 86: 128}


def two_layers(N, cplanes):
    n1 = 96 if N >= 256 else 64
    return Epi(bias=True, bias2=True, act0=RELU, act1=0, act_split=n1, n_split=n1, cplanes=cplanes)


def find_mtiles(ncu, ntiles, per_wg, need_neg_db=False):
    """The smallest mtiles from ntile = (max(per_wg) - 1) CUs + 3 on whose persistent walk has exactly these tile counts per workgroup
    (and a negative dB)."""
    for mtiles in range(ceil_div((max(per_wg) - 1) * ncu + 3, ntiles), 4 * ncu):
        _, counts, neg_db, _, _ = nt_walk(mtiles, ntiles, ncu)
        if counts == frozenset(per_wg) and (neg_db or not need_neg_db):
            return mtiles
    raise AssertionError((ncu, ntiles, per_wg, need_neg_db))


def nt_cases(ncu):
    out = []
    Ms, Ks, cols = itertools.cycle((256, 768, 2048, 2304)), itertools.cycle((64, 96, 128, 160)), itertools.cycle((1, 2, 3))
    pads, ldcs, feeds = itertools.cycle(((0, 0), (8, 24), (24, 8))), itertools.cycle((0, 4)), itertools.cycle(("none", "stale"))
    for tile in (82, 83, 85, 86):
        for a in (2, 1):
            forms = list(PLAIN_FORMS) + (list(FULL_FORMS) if tile in (82, 83) else [])
            forms += [E_OFFSPLIT] + ([E_ROWACC] if tile in (82, 83) else [])
            for e in forms:
                ap, bp = next(pads)
                out.append(Case("nt", tile, "NT", next(Ms), NT_WIDTH[tile] * next(cols), next(Ks), a, 2, ap, bp,
                                ldc_pad=0 if e.cplanes == "only" else next(ldcs), epi=e, feed=next(feeds)))
            if tile in (85, 86):
                for cpl in ("no", "yes", "only"):
                    ap, bp = next(pads)
                    N = NT_WIDTH[tile] * (2 if tile == 86 else next(cols))
                    out.append(Case("nt", tile, "NT", next(Ms), N, next(Ks), a, 2, ap, bp, ldc_pad=next(ldcs), epi=two_layers(N, cpl), feed=next(feeds)))
            # an output 4 bytes off 16-byte alignment: the generic epilogue (dense pitch)
            out.append(Case("nt", tile, "NT", 768, NT_WIDTH[tile], 96, a, 2, c_off=1, epi=E_BIAS))
    # one tile per workgroup at mtiles 1, 3 (< 8), 8 (% 8 == 0) and 9 is covered by the cycle above; the multi-tile walks, sized from the CUs:
    m12 = find_mtiles(ncu, 1, (1, 2))
    out.append(Case("nt", 82, "NT", 256 * m12, 128, 96, 2, 2, 8, 24, ldc_pad=4, epi=E_BIAS, want=(("nt_per_wg", frozenset((1, 2))),)))
    m12n = find_mtiles(ncu, 3, (1, 2), need_neg_db=True)
    out.append(Case("nt", 82, "NT", 256 * m12n, 384, 64, 1, 2, 24, 8, epi=E_CPL, feed="stale", want=(("nt_dB<0",), ("nt_per_wg", frozenset((1, 2))))))
    m12b = find_mtiles(ncu, 2, (1, 2))
    out.append(Case("nt", 83, "NT", 256 * m12b, 384, 160, 2, 2, epi=Epi(rowv=True, rowseg=True, alpha=0.5, bias=True), want=(("nt_per_wg", frozenset((1, 2))),)))
    m23 = find_mtiles(ncu, 1, (2, 3))
    out.append(Case("nt", 86, "NT", 256 * m23, 128, 64, 2, 2, 8, 24, epi=two_layers(128, "yes"), want=(("nt_per_wg", frozenset((2, 3))),)))
    out.append(Case("nt", 82, "NT", 256 * m23, 128, 64, 1, 2, epi=E_ROWACC, feed="stale",
                    want=(("nt_per_wg", frozenset((2, 3))), ("nt_multi_epilogue", "full", "generic", "rowv+acc"))))
    # the generic epilogue inside a multi-tile walk
    out.append(Case("nt", 83, "NT", 256 * m12, 192, 96, 2, 2, epi=E_OFFSPLIT, want=(("nt_multi_epilogue", "full", "generic", "act_split"),)))
    out.append(Case("nt", 85, "NT", 256 * m12, 256, 64, 2, 2, 8, 24, epi=E_OFFSPLIT, feed="stale", want=(("nt_multi_epilogue", "plain", "generic", "act_split"),)))
    out.append(Case("nt", 82, "NT", 256 * m12, 128, 128, 2, 2, c_off=1, epi=E_BIAS, want=(("nt_multi_epilogue", "full", "generic", "c_off"),)))
    out.append(Case("nt", 83, "NT", 256 * m12, 192, 64, 1, 2, epi=E_ROWACC, want=(("nt_multi_epilogue", "full", "generic", "rowv+acc"),)))
    out.append(Case("nt", 85, "NT", 256 * m12b, 512, 96, 1, 2, epi=two_layers(512, "only"), want=(("nt_per_wg", frozenset((1, 2))), ("nt_multi_epilogue", "plain", "plain", "-"))))
    return out


TN_SHAPES = {91: ((128, 256), (512, 256)), 92: ((256, 128), (512, 128)), 93: ((256, 256), (256, 512))}
TN_KSPLITS = ((96, 1), (224, 2), (224, 3), (256, 3))
E_ACC = Epi(accumulate=True)


def tn_cases():
    out = []
    ks = itertools.cycle(TN_KSPLITS)
    pads = itertools.cycle(((0, 0), (8, 24)))
    multi = itertools.cycle((("kernel", E_BIAS._replace(alpha=1.0), 0), ("merge", E_ACC, 0), ("kernel", E_ACC, 4)))
    direct = itertools.cycle((E_CPL, E_ACC, E_NONE))
    for tile in (91, 92, 93):
        for b in (2, 1):
            for (M, N) in TN_SHAPES[tile]:
                for _ in range(2):
                    K, sp = next(ks)
                    ap, bp = next(pads)
                    if sp == 1:
                        out.append(Case("tn", tile, "TN", M, N, K, 2, b, ap, bp, splits=1, epi=next(direct)))
                    else:
                        red, e, lp = next(multi)
                        out.append(Case("tn", tile, "TN", M, N, K, 2, b, ap, bp, ldc_pad=lp, splits=sp, epi=e, want=(("tn_reduce", red),)))
            next(ks)                                    # (shift the rotation: every tile meets every (K, splits))
    # splits x og = 8 exactly, and 10: two rounds of eight groups
    out.append(Case("tn", 91, "TN", 512, 256, 224, 2, 2, 8, 24, splits=2, epi=E_ACC, want=(("tn_groups", 8), ("tn_rounds", 1))))
    out.append(Case("tn", 91, "TN", 640, 256, 224, 2, 1, splits=2, epi=E_BIAS._replace(alpha=1.0), want=(("tn_groups", 10), ("tn_rounds", 2))))
    return out


RAGGED = ((200, 136, 72), (260, 196, 40))


def pre_cases():
    out = []
    n = 0
    for tile in PLANES_TILES:
        for lay in ("NT", "NN", "TN", "TT"):
            for pre in (1, 2, 3):
                for k in range(2):
                    M, N, K = RAGGED[(n + k) % 2]
                    single = (n // 2 + k) % 2 == 1
                    a = 0 if not pre & 1 else (1 if single and (pre != 3 or n % 4 < 2) else 2)
                    b = 0 if not pre & 2 else (1 if single and (pre != 3 or n % 4 >= 2) else 2)
                    e = (E_NONE, E_BIAS, E_ACC)[n % 3]
                    out.append(Case("pre", tile, lay, M, N, K, a, b, splits=(1, 3)[(n // 3 + k) % 2], epi=e, feed=("none", "stale")[n % 2]))
                n += 1
    for lay in ("NN", "TN"):                            # tile 43: A from planes only, B from its fp32 image
        out.append(Case("pre", 43, lay, 256, 192, 64, 2, 0, epi=E_BIAS, want=(("pre", 43, lay, 1),)))
        out.append(Case("pre", 43, lay, 264, 200, 72, 2, 0, a_pad=8, epi=E_NONE, feed="stale", want=(("pre", 43, lay, 1), ("pre_ragged", 43))))
    for tile, whole in ((34, (192, 256, 64)), (24, (128, 256, 64))):
        for pre in (2, 3):
            a = 2 if pre == 3 else 0
            out.append(Case("pre", tile, "TN", *whole, a, 2, epi=E_BIAS, want=(("pre", tile, "TN", pre), ("pre_whole", tile))))
            out.append(Case("pre", tile, "TN", 192, 264, 264, a, 2, b_pad=8, epi=E_ACC, feed="stale", want=(("pre", tile, "TN", pre), ("pre_ragged", tile))))
            out.append(Case("pre", tile, "TN", 192, 264, 264, a, 1, splits=3, epi=E_NONE, want=(("pre", tile, "TN", pre), ("pre_planes", tile, "B", 1))))
    # the dispatch holes: planes are given, the fp32 image is read (the expected value gains al bl)
    out.append(Case("pre", 43, "NN", 256, 192, 64, 2, 2, epi=E_NONE, want=(("hole", "43both"),)))
    out.append(Case("pre", 23, "NT", 200, 192, 72, 2, 2, epi=E_NONE, want=(("hole", "23"),)))
    out.append(Case("pre", 22, "NT", 200, 136, 36, 2, 2, a_pad=4, b_pad=4, epi=E_NONE, want=(("hole", "ext%8"),)))
    out.append(Case("pre", 22, "NN", 200, 136, 72, 2, 0, a_off=4, a_pad=4, epi=E_NONE, want=(("hole", "base%16"),)))
    return out


def random_cases():
    return [Case("nt", 83, "NT", 768, 384, 160, 2, 2, 8, 24, epi=E_NONE, vals="randn"),
            Case("nt", 86, "NT", 512, 256, 96, 1, 2, epi=E_NONE, vals="randn", feed="stale"),
            Case("tn", 93, "TN", 256, 256, 256, 2, 2, 8, 24, splits=3, epi=E_NONE, vals="randn"),
            Case("tn", 91, "TN", 128, 256, 96, 2, 1, splits=1, epi=E_NONE, vals="randn"),
            Case("pre", 22, "NN", 200, 136, 72, 2, 2, epi=E_NONE, vals="randn"),
            Case("pre", 34, "TN", 192, 264, 264, 2, 2, splits=3, epi=E_NONE, vals="randn", feed="stale")]


def all_cases(ncu):
    return nt_cases(ncu) + tn_cases() + pre_cases() + random_cases()


def case_id(c):
    e = c.epi
    bits = [n for n in ("bias", "accumulate", "maskref", "rowv", "rowseg", "maskbits", "colsum", "drop") if getattr(e, n)]
    bits += ["relu"] * (e.act0 == RELU) + ["half"] * (e.alpha != 1.0)
    if e.n_split:
        bits.append(f"two{e.n_split}")
    if e.cplanes != "no":
        bits.append("cpl_" + e.cplanes)
    if e.act_split is not None and not e.n_split:
        bits.append(f"split{e.act_split}")
    return (f"{c.fam}{c.tile}-{c.lay}-{c.M}x{c.N}x{c.K}-a{c.a}b{c.b}-p{c.a_pad}.{c.b_pad}.{c.a_off}-c{c.ldc_pad}.{c.c_off}-s{c.splits}-"
            f"{'+'.join(bits) or 'plain'}-{c.vals}-{c.feed}")


NCU = device_cus()
CASES = all_cases(NCU)
assert len({case_id(c) for c in CASES}) == len(CASES), "case ids must be unique"


# ------------------------------------------------------------------------------------------------------------------------------
# launch and compare
# ------------------------------------------------------------------------------------------------------------------------------
_INPUTS, _REFS = {}, {}
WORST = {}                                             # family -> (error / bound, case, figure)


def _ops():
    from advmil_amd import _lib, ops
    _lib.lib()
    return ops


class bf16x3:
    def __enter__(self):
        self.ops = _ops()
        self.prev = self.ops.get_gemm_mode()
        self.ops.set_gemm_mode("bf16x3")
        return self.ops

    def __exit__(self, *exc):
        self.ops.set_gemm_mode(self.prev)
        return False


def inputs(c):
    key = (c.fam, c.lay, c.M, c.N, c.K, c.a, c.b, c.vals, c.epi)
    if key not in _INPUTS:
        a_ext, b_ext, _, _ = pitches(c)
        a_kc, b_kc = R.LAYOUTS[c.lay]
        a_rows, b_rows = (c.M if a_kc else c.K), (c.N if b_kc else c.K)
        make = R.int_operand if c.vals == "int" else R.split_operand
        # (an operand handed over without planes still has two integer planes' worth of value: its image is hi + lo)
        _INPUTS[key] = dict(a=make(a_rows, a_ext, c.a == 1, 11), b=make(b_rows, b_ext, c.b == 1, 12), d=R.epi_data(c.M, c.N, c.epi, c.K))
    return _INPUTS[key]


def reference(c, p):
    key = (case_id(c), p.a_src, p.b_src)
    if key not in _REFS:
        inp = inputs(c)
        fa, fb = p.a_src == "planes", p.b_src == "planes"
        acc = R.contract(inp["a"], inp["b"], c.lay, fa, fb)
        ref = R.apply_epilogue(acc, inp["d"], c.epi)
        if c.vals == "randn":
            ref["e32"] = R.relerr(R.contract(inp["a"], inp["b"], c.lay, fa, fb, torch.float32), acc)
            ref["true"] = R.true_product(inp["a"], inp["b"], c.lay)
        _REFS[key] = ref
    return _REFS[key]


def launch(c):
    """One launch of the case -> dict of everything it wrote (the whole output buffer, pad columns included)."""
    p = plan(c, NCU)
    assert p is not None, c
    inp, e = inputs(c), c.epi
    a_kc, b_kc = R.LAYOUTS[c.lay]
    a_ext, b_ext, lda, ldb = pitches(c)
    with bf16x3() as ops:
        apl = R.place_planes(inp["a"], c.a_pad, c.a_off) if c.a else None
        bpl = R.place_planes(inp["b"], c.b_pad) if c.b else None
        # an operand the mirror says is read from its planes travels with NO usable fp32 image: None, or NaN under fp32_stale
        A = R.place_image(inp["a"], lda, nan=p.a_src == "planes")
        B = R.place_image(inp["b"], ldb, nan=p.b_src == "planes")
        if p.a_src == "planes":
            if c.feed == "none":
                A = None
            else:
                apl.fp32_stale = True
        if p.b_src == "planes":
            if c.feed == "none" and p.kernel != "generic" and c.b == 2:
                B = None
            else:
                bpl.fp32_stale = True
        d = {k: v.to(DEV) for k, v in inp["d"].items() if k != "keep"}
        n_out = e.n_split or c.N
        out = buf = cpl = None
        res = {}
        if e.cplanes != "only":
            out, buf = R.place_out(c.M, n_out, c.ldc_pad, d.get("C0", None) if e.accumulate and not e.n_split else None, c.c_off)
            res["C"] = buf
        if e.cplanes != "no":
            ldc = n_out + c.ldc_pad
            wide = [torch.full((c.M, ldc), 55.0, dtype=torch.bfloat16).to(DEV) for _ in range(2)]
            cpl = ops.Planes(wide[0][:, :n_out], wide[1][:, :n_out])
            res["c_hi"], res["c_lo"] = wide
        if e.n_split:
            res["c2"] = two_layer_launch(ops, c, A if A is not None else apl.hi, B if B is not None else bpl.hi, apl, bpl, out, cpl, d)
            return res
        kw = {}
        if e.bias:
            kw["bias"] = d["bias"]
        if e.rowv:
            kw.update(rowv=d["rowv"], colv=d["colv"], rowseg=d.get("rowseg"))
        if e.maskref:
            kw["maskref"] = d["maskref"]
        if e.maskbits:
            kw["maskbits"] = d["maskbits"]
        if e.maskref or e.maskbits:
            kw["mask_scale"] = R.MASK_SCALE
        if e.colsum:
            rows = _lib().advmil_gemm_f32_colsum_rows(c.tile, c.M, c.N)
            assert rows == c.M // 64, rows
            res["colsum"] = kw["colsum"] = torch.full((rows, c.N), 33.0).to(DEV)
        if e.drop:
            rng = ops.DeviceRng(DEV, seed=R.DROP_SEED)
            kw.update(drop_p=R.DROP_P, seed=rng.seed, stream_id=R.DROP_SID)
        prof, ops.KERNEL_PROFILE = ops.KERNEL_PROFILE, []
        try:
            got = ops.gemm(A, B, a_kc, b_kc, c.M, c.N, c.K, out=out, ldc=None if out is None else out.stride(0), act0=e.act0, act1=e.act1,
                           act_split=e.act_split, accumulate=e.accumulate, alpha=e.alpha, splits=c.splits, tile=c.tile, a_planes=apl, b_planes=bpl,
                           c_planes=cpl, c_planes_only=e.cplanes == "only", **kw)
            launched = [rec[0] for rec in ops.KERNEL_PROFILE]
        finally:
            ops.KERNEL_PROFILE = prof
        assert got is out
        assert launched == [kernel_name(c, p)], (launched, kernel_name(c, p))      # ops.gemm kept the tile the mirror was asked about
    return res


def kernel_name(c, p):
    """The name ops.gemm records for the kernel it launches (after its own re-routing of tiles)."""
    if p.kernel == "nt":
        return {82: "gemm_nt_planes_kernel<2>", 83: "gemm_nt_planes_kernel<3>", 84: "gemm_nt_planes_kernel<4>", 85: "gemm_nt_planes_kernel<4,plain>",
                86: "gemm_nt_planes_kernel<2,plain>"}[c.tile]
    if p.kernel == "tn":
        return "gemm_tn_planes_kernel<%d>" % c.tile
    a_kc, b_kc = R.LAYOUTS[c.lay]
    return "gemm_f32_kernel<%d,%d,%d,%d>" % (a_kc, b_kc, c.tile // 10, c.tile % 10)


def _lib():
    from advmil_amd import _lib as L
    return L.lib()


def two_layer_launch(ops, c, A, B, apl, bpl, out, cpl, d):
    """advmil_epilogue_t's two-layer form has no wrapper of its own shape in ops (ops.gemm_two_layers stacks two weights): the raw call."""
    from advmil_amd import _lib as L
    e = c.epi
    n1, n2 = e.n_split, c.N - e.n_split
    c2 = torch.full((c.M, n2 + 4), 44.0).to(DEV)
    ep = L.Epilogue()
    ep.bias, ep.bias2 = d["bias"].data_ptr(), d["bias"][n1:].data_ptr()
    ep.act0, ep.act1, ep.act_split, ep.alpha = e.act0, e.act1, n1, e.alpha
    ep.a_hi, ep.a_lo, ep.b_hi, ep.b_lo = apl.hi.data_ptr(), apl.lo_ptr(), bpl.hi.data_ptr(), bpl.lo_ptr()
    if cpl is not None:
        ep.c_hi, ep.c_lo = cpl.hi.data_ptr(), cpl.lo.data_ptr()
    ep.c2, ep.ldc2, ep.n_split = c2.data_ptr(), n2 + 4, n1
    ldc = n1 + c.ldc_pad
    L.check(L.lib().advmil_gemm_f32_tiled(1, 1, c.M, c.N, c.K, ops._p(A), A.stride(0), ops._p(B), B.stride(0), ops._p(out), ldc, ctypes.byref(ep), 1, c.tile,
                                          None, 0, ops._stream()), "two-layer launch")
    return c2


def judge(family, case, err, bound):
    line = " ".join(f"{k} {err[k]:.2e}/{bound[k]:.1e}" for k in err)
    print(f"[{family}] {case}: {line}")
    for k in err:
        r = err[k] / bound[k]
        if r > WORST.get(family, (0.0,))[0]:
            WORST[family] = (r, case, k)
    for k in err:
        assert err[k] < bound[k], (family, case, k, err[k], bound[k])


def body(c):
    """Assert the walk on the host, launch, compare with the oracle."""
    p = plan(c, NCU)
    assert p is not None, c
    for t in c.want:
        assert t in p.tags, (t, sorted(p.tags, key=str))
    got = {k: v.detach().cpu() for k, v in launch(c).items()}
    ref, e = reference(c, p), c.epi
    n_out = e.n_split or c.N
    if "C" in got:
        Cbuf = got["C"]
        if c.c_off:
            assert bool((Cbuf[:c.c_off] == 77.0).all()) and bool((Cbuf[c.c_off + c.M * n_out:] == 77.0).all())
            C = Cbuf[c.c_off:c.c_off + c.M * n_out].view(c.M, n_out)
        else:
            assert bool((Cbuf[:, n_out:] == 77.0).all()), "pad columns of the output were written"
            C = Cbuf[:, :n_out]
        want = ref["C"][:, :n_out]
        if c.vals == "randn":
            judge(c.fam, case_id(c), dict(planes=R.relerr(C, want), true=float((C.double() - ref["true"]).abs().max() / ref["true"].abs().max())),
                  dict(planes=4 * ref["e32"], true=2e-5))
        elif e.drop:
            keep = ref["keep"]
            assert bool((C[~keep] == 0).all()), "dropped entries must be exactly 0"
            assert bool(((C.double() - want).abs() <= 2.0 ** -23 * want.abs())[keep].all()), "kept entries: one ulp of 2 v"
        else:
            assert torch.equal(C.double(), want), (case_id(c), int((C.double() != want).sum()), float((C.double() - want).abs().max()))
    if e.n_split:
        assert bool((got["c2"][:, c.N - n_out:] == 44.0).all())
        assert torch.equal(got["c2"][:, :c.N - n_out].double(), ref["C"][:, n_out:]), case_id(c)
    if e.cplanes != "no":
        for k in ("c_hi", "c_lo"):
            assert bool((got[k][:, n_out:].float() == 55.0).all())
            assert torch.equal(got[k][:, :n_out].double(), ref[k]), (case_id(c), k)
    if e.colsum:
        assert torch.equal(got["colsum"].double(), ref["colsum"]), case_id(c)


@pytest.mark.parametrize("c", [c for c in CASES if c.fam == "nt"], ids=case_id)
def test_plane_fed_nt_walks(c):
    body(c)


@pytest.mark.parametrize("c", [c for c in CASES if c.fam == "tn"], ids=case_id)
def test_plane_fed_tn_walks(c):
    body(c)


@pytest.mark.parametrize("c", [c for c in CASES if c.fam == "pre"], ids=case_id)
def test_register_staged_plane_walks(c):
    body(c)


# ------------------------------------------------------------------------------------------------------------------------------
# tile 84: the fused gate score, two-plane (tanh / sigmoid are not exact: the tolerance and float64 of test_gemm_fused_gate_score)
# ------------------------------------------------------------------------------------------------------------------------------
GateCase = collections.namedtuple("GateCase", "M D pad")
GATE_CASES = (GateCase(768, 128, 0), GateCase(2304, 256, 8))


def launch_gate(c):
    g = R._gen(5, c.M, c.D)
    h = R.Operand(*R.split_bf16(torch.randn(c.M, c.D, generator=g)))
    Wa, Wb = 0.05 * torch.randn(c.D, c.D, generator=g), 0.05 * torch.randn(c.D, c.D, generator=g)
    ba, bb, wc, bc = 0.1 * torch.randn(c.D, generator=g), 0.1 * torch.randn(c.D, generator=g), 0.1 * torch.randn(c.D, generator=g), torch.randn(1, generator=g)
    Wi = R.Operand(*R.split_bf16(torch.stack((Wa, Wb), dim=1).reshape(2 * c.D, c.D)))
    bi = torch.stack((ba, bb), dim=1).reshape(2 * c.D)
    with bf16x3() as ops:
        hp, wp = R.place_planes(h, c.pad), R.place_planes(Wi, c.pad)
        part = ops.gemm(None, None, True, True, c.M, 2 * c.D, c.D, bias=bi.to(DEV), gate_wc=wc.to(DEV), tile=84, splits=1, a_planes=hp, b_planes=wp)
    h64, W64 = h.hi + h.lo, Wi.hi + Wi.lo                                      # the planes ARE the operands
    a64 = torch.tanh(h64 @ W64[0::2].t() + ba.double())
    b64 = torch.sigmoid(h64 @ W64[1::2].t() + bb.double())
    return dict(score=part.sum(dim=1).cpu() + bc), (a64 * b64) @ wc.double() + bc.double()


@pytest.mark.parametrize("c", GATE_CASES, ids=lambda c: f"M{c.M}-D{c.D}-pad{c.pad}")
def test_plane_fed_gate_score_tile(c):
    assert plan(Case("gate", 84, "NT", c.M, 2 * c.D, c.D, 2, 2, c.pad, c.pad), NCU).kernel == "nt"
    got, want = launch_gate(c)
    judge("gate", f"M{c.M}-D{c.D}", dict(score=float((got["score"].double() - want).abs().max())), dict(score=2e-5))


# ------------------------------------------------------------------------------------------------------------------------------
# the parametrisation reaches every walk the mirrors name
# ------------------------------------------------------------------------------------------------------------------------------
def walks_reached(ncu=None):
    """Worked out on the host from the case lists alone (tests/test_gemm_walks_plan_cpu.py calls this for a nominal 256-CU device)."""
    ncu = NCU if ncu is None else ncu
    got = set()
    for c in (CASES if ncu == NCU else all_cases(ncu)):
        p = plan(c, ncu)
        assert p is not None, c
        for t in c.want:
            assert t in p.tags, (c, t)
        got |= p.tags
    for c in GATE_CASES:
        got |= plan(Case("gate", 84, "NT", c.M, 2 * c.D, c.D, 2, 2, c.pad, c.pad), ncu).tags
    return got


def _wanted():
    w = set()
    for t in (82, 83, 85, 86):
        w |= {("nt", t, 2), ("nt", t, 1), ("nt_epilogue", t, "generic"), ("nt_epilogue", t, "plain" if t >= 85 else "stream")}
        w |= {("nt_ntiles", t, n) for n in ((1, 2, 3) if t != 86 else (1, 2))}
        w |= {("nt_epi", t, f) for f in ("alpha", "act_split", "cplanes_yes", "cplanes_only")}
    for t in (82, 83):
        w |= {("nt_epi", t, f) for f in ("accumulate", "maskref", "rowv", "rowseg", "maskbits", "colsum", "drop", "rowv+maskref", "rowv+maskbits")}
    for t in (85, 86):
        w |= {("nt_two_layers", t, cp) for cp in ("no", "yes", "only")}
    w |= {("nt", 84, 2), ("nt_in_slot", True), ("nt_in_slot", False), ("nt_nbuf", 2), ("nt_nbuf", 3)}
    w |= {("nt_chunks", n) for n in (2, 3, 4, 5)} | {("nt_mtiles", m) for m in ("<8", "%8", "9")}
    w |= {("nt_per_wg", frozenset(s)) for s in ((1,), (1, 2), (2, 3))} | {("nt_dB<0",), ("nt_rem",), ("nt_pitch>K",), ("nt_ldc>N",)}
    w |= {("nt_multi_epilogue", "full", "generic", r) for r in ("act_split", "c_off", "rowv+acc")}
    w |= {("nt_multi_epilogue", "plain", "generic", "act_split"), ("nt_multi_epilogue", "plain", "plain", "-"), ("nt_multi_epilogue", "full", "stream", "-")}
    for t in (91, 92, 93):
        w |= {("tn", t, 2), ("tn", t, 1)} | {("tn_chunks", t, ch) for ch in ((3,), (4, 3), (3, 3, 1), (3, 3, 2))}
    w |= {("tn_by_m", True), ("tn_by_m", False), ("tn_rounds", 1), ("tn_rounds", 2), ("tn_groups", 8), ("tn_groups", 10), ("tn_pitch",),
          ("tn_short_split", 3, 1), ("tn_short_split", 3, 2), ("tn_short_split", 2, 1), ("tn_nbuf", 2), ("tn_nbuf", 3)}
    w |= {("tn_reduce", r) for r in ("direct", "kernel", "merge")}
    for t in PLANES_TILES:
        w |= {("pre", t, lay, p) for lay in R.LAYOUTS for p in (1, 2, 3)} | {("pre_planes", t, o, n) for o in "AB" for n in (1, 2)}
        w |= {("pre_splits", t, 1), ("pre_splits", t, 3), ("pre_ragged", t)}
    w |= {("pre", 43, "NN", 1), ("pre", 43, "TN", 1), ("pre_ragged", 43)}
    for t in (34, 24):
        w |= {("pre", t, "TN", 2), ("pre", t, "TN", 3), ("pre_ragged", t), ("pre_whole", t), ("pre_planes", t, "B", 1)}
    w |= {("pre_full", False), ("pre_full", True)} | {("hole", h) for h in ("43both", "23", "ext%8", "base%16")}
    return w


WALKS_WANTED = _wanted()


def test_every_walk_is_reached():
    """Every tile and plane count of the three families, every ring depth and chunk count, every tile count per workgroup, the `rem`
    branch, a negative dB, every epilogue route (also inside a multi-tile walk), every TN split shape, group round and reduce, every PRE
    form and every dispatch hole: each is asserted by at least one case above."""
    missing = WALKS_WANTED - walks_reached()
    assert not missing, sorted(missing, key=str)
    for fam, (r, case, k) in sorted(WORST.items()):
        print(f"worst of {fam}: {r:.3f} of its bound ({k}, {case})")
