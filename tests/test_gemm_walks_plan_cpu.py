"""CPU: what aims the contraction-walk tests is itself pinned. tests/test_gemm_walks_gpu.py works out on the host which kernel a launch
lands on, which operands are read from their planes, how the persistent NT kernel walks its tiles and how the TN kernel splits and
groups its work, from constants and expressions copied out of csrc/gemm_host.hip, gemm_f32.hip, gemm_nt_planes.hip, gemm_tn_planes.hip
and gemm_core.h. A retune of the kernels must break these tests instead of silently un-aiming the others: the constants are pinned to
the source text, the mirrors to the library's own host-only arithmetic, and the refusals of advmil_gemm_f32_tiled that the mirrors
predict are asked of the library itself (they return before any launch, so no GPU is needed)."""
import ctypes
import os
import re

import pytest

from tests import test_gemm_walks_gpu as TG
from tests.gemm_ref import Epi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "advmil_amd", "csrc")
FILES = ("gemm_host.hip", "gemm_f32.hip", "gemm_nt_planes.hip", "gemm_tn_planes.hip", "gemm_core.h")
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


def read_sources():
    return {f: open(os.path.join(CSRC, f)).read() for f in FILES}


def check_source(src):
    """Every constant and expression the mirrors copy, where the sources state it. Raises AssertionError on the first that moved."""
    host, f32, ntp, tnp, core = (src[f] for f in FILES)
    one = lambda text, pat: re.findall(pat, text, flags=re.M)   # noqa: E731
    has = lambda text, line: text.count(line)                   # noqa: E731
    # chunking and the epilogue's per-wave LDS area
    assert one(core, r"^#define BK (\d+)\b") == [str(TG.BK)] and one(core, r"^#define PITCH_KC (\d+)\b") == [str(TG.PITCH_KC)]
    assert has(core, "#define EPI_WAVE_FLOATS(TM, TN) (32 * PITCH_KC + 32 * ((TN) + 2 * (TM)) + 32 * (TM) * (TN))") == 1
    # planes_usable and where it is asked
    assert has(host, "return hi && !((uintptr_t)hi & 15) && !((uintptr_t)lo & 15) && !(ld & 7) && !(contiguous_extent & 7);") == 1
    assert has(host, "if (planes_usable(epi->a_hi, epi->a_lo, lda, a_kc ? K : M)) pre |= 1;") == 1
    assert has(host, "if (planes_usable(epi->b_hi, epi->b_lo, ldb, b_kc ? K : N)) pre |= 2;") == 1
    # the split arithmetic
    assert has(host, "g.k_chunk = ((kchunks + splits - 1) / splits) * BK;") == 1 and has(host, "splits = (int)((K + g.k_chunk - 1) / g.k_chunk);") == 1
    # plane-fed NT: what the host asks, the persistent grid, the launch table, the ring and tile_of
    assert has(host, "if (K < %d) return ADVMIL_EINVAL;" % TG.NT_MIN_K) == 1
    assert has(host, "if (g_gemm_mode != 1 || !a_kc || !b_kc || pre != 3 || splits != 1 || (M % bm) || (K % bkt) || (N % (64 * tnp))) return ADVMIL_EINVAL;") == 1
    assert has(host, "const int tnp = tile == 85 ? 4 : tile == 86 ? 2 : tile % 10, bm = 256, bkt = 32;") == 1
    assert has(host, "dim3 pgrid(ntile_all < ncu ? ntile_all : ncu);") == 1
    assert has(host, "if (!epi->b_lo) return ADVMIL_EINVAL;") == 1
    assert has(host, "if ((ldc & 3) || (((uintptr_t)C) & 15) || (((uintptr_t)epi->bias) & 15) ||") == 1          # the two-layer form: streaming only
    table = one(ntp, r"case (\d+): hipLaunchKernelGGL\(\(gemm_nt_planes_kernel<(\d), (\d), 4, 32(?:, (\d))?(?:, (\d))?>\)")
    single = [(t, tn, nb, ep, alo) for t, tn, nb, ep, alo in table if alo == "0"]
    double = [(t, tn, nb, ep or "0") for t, tn, nb, ep, alo in table if alo != "0"]
    assert sorted(single) == sorted((str(t),) + tuple(str(v) for v in TG.NT_TABLE[t]) + ("0",) for t in TG.NT_SINGLE), single
    assert sorted(double) == sorted((str(t),) + tuple(str(v) for v in TG.NT_TABLE[t]) for t in TG.NT_TABLE), double
    assert has(ntp, "constexpr int AROWS = (1 + ALO) * BM_;") == 1 and has(ntp, "constexpr int ROWS_ALL = AROWS + 2 * BN_;") == 1
    assert has(ntp, "constexpr int BUF_HW = ROWS_ALL * BKT;") == 1 and has(ntp, "constexpr int PATCH_FLOATS = NW * EPI_WAVE_FLOATS(TM, TN);") == 1
    assert has(ntp, "constexpr bool EPI_IN_SLOT = PATCH_FLOATS <= BUF_HW / 2;") == 1
    for line in ("const int inner = g.ntiles, outer = g.mtiles;", "const int per_group = 8 * inner, full = (outer / 8) * per_group;",
                 "mt = (v / per_group) * 8 + (r & 7);", "nt = r >> 3;", "const int rem = outer - (outer / 8) * 8, r = v - full;",
                 "mt = (outer / 8) * 8 + r % rem;", "nt = r / rem;", "for (; v < ntile; v += G) {", "const bool has_next = v + G < ntile;"):
        assert has(ntp, line) == 1, line
    # the epilogue route inside the kernels
    assert has(core, "const bool stream = direct && !gate_mode && vec_ok && (g.N % (32 * TN * WC)) == 0 && (g.M % (32 * TM * WR)) == 0 && (e.act_split & 31) == 0 &&") == 1
    assert has(core, "nmode <= 1 && !(e.rowv && e.seed && e.rng_row)") == 1
    assert has(core, "const int nmode = (e.rowv && e.maskref && !e.accumulate) ? 1 : (e.rowv ? 1 : 0) + (e.maskref ? 1 : 0) + (e.accumulate ? 1 : 0);") == 1
    assert has(core, "const bool vec_ok = ((ldo & 3) == 0) && (((uintptr_t)out & 15) == 0);") == 1
    # plane-fed TN
    assert has(host, "if (g.k_chunk / 32 < %d || epi->gate_wc || epi->c2) return ADVMIL_EINVAL;" % TG.TN_MIN_CHUNKS) == 1
    assert has(host, "const int bm = tile == 91 ? 128 : 256, bn = tile == 92 ? 128 : 256;") == 1
    assert has(host, "const int gs = M >= N ? g.ntiles : g.mtiles, og = M >= N ? g.mtiles : g.ntiles;") == 1
    assert has(host, "const dim3 tgrid((unsigned)(8 * ((splits * og + 7) / 8) * gs));") == 1
    assert has(host, "if (!epi->a_lo) return ADVMIL_EINVAL;") == 1
    ttab = one(tnp, r"(case \d+|default): hipLaunchKernelGGL\(\(gemm_tn_planes_kernel<(\d), (\d), (\d), (\d), (\d)(?:, (\d))?>\)")
    want_t = {"case 91": TG.TN_TABLE[91], "case 92": TG.TN_TABLE[92], "default": TG.TN_TABLE[93]}
    assert sorted(ttab) == sorted((k,) + tuple(str(x) for x in v) + (blo,) for k, v in want_t.items() for blo in ("", "0")), ttab
    assert has(tnp, "const int q = bid >> 3, G = (bid & 7) + 8 * (q / gs), mem = q % gs;") == 1 and has(tnp, "const bool by_m = g.M >= g.N;") == 1
    assert has(tnp, "if (G >= g.splits * og) return;") == 1
    # which reduce
    assert has(f32, "const bool plain = e.accumulate && e.alpha == 1.0f && !e.bias && !e.rowv && !e.maskref && e.act0 == 0 && e.act1 == 0 &&") == 1
    assert has(f32, "!(e.seed && e.drop_p > 0.0f) && !e.c_hi && !e.gate_wc && g.ldc == g.N && (g.N & 3) == 0 &&") == 1
    assert has(f32, "(((uintptr_t)g.C) & 15) == 0 && g.splits <= 64;") == 1
    # the generic kernels' PRE dispatch
    gtab = one(f32, r"case (\d+): launch_tile<(\d), (\d), (true|false)>")
    assert gtab == [("23", "2", "3", "false"), ("22", "2", "2", "true"), ("13", "1", "3", "false"), ("12", "1", "2", "true"), ("11", "1", "1", "true")]
    assert sorted(int(t) for t, _, _, pl in gtab if pl == "true") == sorted(TG.PLANES_TILES)
    assert one(f32, r"case (\d): launch_tile_m<TM, TN, true, (\d), 2, 2>") == [("1", "1"), ("2", "2"), ("3", "3")]
    assert has(f32, "if (pre == 1 && a_kc && !b_kc) hipLaunchKernelGGL((gemm_f32_kernel<true, false, 2, 3, true, 1, 32, 4, 2>)") == 1
    assert has(f32, "else if (pre == 1 && !a_kc && !b_kc) hipLaunchKernelGGL((gemm_f32_kernel<false, false, 2, 3, true, 1, 32, 4, 2>)") == 1
    assert has(f32, "else launch_tile_m<2, 3, true, 0, 4, 2>(a_kc, b_kc, grid, stream, g);") == 1
    for tm, tn in ((3, 2), (2, 2)):
        assert has(f32, f"if (pre == 2 && !a_kc && !b_kc) hipLaunchKernelGGL((gemm_f32_kernel<false, false, {tm}, {tn}, true, 2, 32, 2, 4>)") == 1
        assert has(f32, f"else if (pre == 3 && !a_kc && !b_kc) hipLaunchKernelGGL((gemm_f32_kernel<false, false, {tm}, {tn}, true, 3, 32, 2, 4>)") == 1
        assert has(f32, f"else launch_tile_m<{tm}, {tn}, true, 0, 2, 4>(a_kc, b_kc, grid, stream, g);") == 1
    assert has(f32, "case 42: launch_tile_m<2, 2, true, 0, 4, 2>(a_kc, b_kc, grid, stream, g); break;") == 1
    assert has(core, "static constexpr bool FULL = NPIECE % NT == 0;") == 1 and has(core, "static constexpr int NPIECE = ROWS * BKT / 8;") == 1


BITES = {
    "gemm_core.h": (("#define PITCH_KC 36", "#define PITCH_KC 40"), ("32 * ((TN) + 2 * (TM))", "32 * ((TN) + 4 * (TM))"), ("(e.act_split & 31) == 0 &&", "(e.act_split & 15) == 0 &&"),
                    ("nmode <= 1 && !(e.rowv", "nmode <= 2 && !(e.rowv"), ("FULL = NPIECE % NT == 0;", "FULL = true;")),
    "gemm_host.hip": (("!(ld & 7) && !(contiguous_extent & 7);", "!(ld & 3) && !(contiguous_extent & 3);"), ("if (K < 64) return ADVMIL_EINVAL;", "if (K < 96) return ADVMIL_EINVAL;"),
                      ("if (g.k_chunk / 32 < 3 ||", "if (g.k_chunk / 32 < 2 ||"), ("(8 * ((splits * og + 7) / 8) * gs)", "(splits * og * gs)"),
                      ("dim3 pgrid(ntile_all < ncu ? ntile_all : ncu);", "dim3 pgrid(ntile_all < 2 * ncu ? ntile_all : 2 * ncu);"),
                      ("lda, a_kc ? K : M)) pre |= 1;", "lda, K)) pre |= 1;"), ("const int gs = M >= N ? g.ntiles", "const int gs = M > N ? g.ntiles"),
                      ("tile == 85 ? 4 : tile == 86 ? 2 : tile % 10", "tile == 85 ? 4 : tile == 86 ? 3 : tile % 10")),
    "gemm_nt_planes.hip": (("case 82: hipLaunchKernelGGL((gemm_nt_planes_kernel<2, 3, 4, 32>)", "case 82: hipLaunchKernelGGL((gemm_nt_planes_kernel<2, 2, 4, 32>)"),
                           ("case 83: hipLaunchKernelGGL((gemm_nt_planes_kernel<3, 2, 4, 32, 0, 0>)", "case 83: hipLaunchKernelGGL((gemm_nt_planes_kernel<3, 3, 4, 32, 0, 0>)"),
                           ("PATCH_FLOATS <= BUF_HW / 2;", "PATCH_FLOATS <= BUF_HW;"), ("const int per_group = 8 * inner,", "const int per_group = 4 * inner,"),
                           ("mt = (outer / 8) * 8 + r % rem;", "mt = (outer / 8) * 8 + r / ((r / rem) + 1);"), ("nt = r >> 3;", "nt = r >> 2;")),
    "gemm_tn_planes.hip": (("case 91: hipLaunchKernelGGL((gemm_tn_planes_kernel<2, 2, 2, 4, 3>)", "case 91: hipLaunchKernelGGL((gemm_tn_planes_kernel<2, 2, 2, 4, 2>)"),
                           ("default: hipLaunchKernelGGL((gemm_tn_planes_kernel<2, 4, 4, 2, 2, 0>)", "default: hipLaunchKernelGGL((gemm_tn_planes_kernel<2, 4, 4, 2, 3, 0>)"),
                           ("G = (bid & 7) + 8 * (q / gs)", "G = (bid & 3) + 4 * (q / gs)"), ("const bool by_m = g.M >= g.N;", "const bool by_m = g.M > g.N;")),
    "gemm_f32.hip": (("case 12: launch_tile<1, 2, true>", "case 12: launch_tile<1, 2, false>"), ("case 23: launch_tile<2, 3, false>", "case 23: launch_tile<2, 3, true>"),
                     ("if (pre == 1 && a_kc && !b_kc) hipLaunchKernelGGL", "if ((pre & 1) && a_kc && !b_kc) hipLaunchKernelGGL"),
                     ("else if (pre == 3 && !a_kc && !b_kc) hipLaunchKernelGGL((gemm_f32_kernel<false, false, 3, 2, true, 3,", "else if (pre == 3 && !b_kc) hipLaunchKernelGGL((gemm_f32_kernel<false, false, 3, 2, true, 3,"),
                     ("g.ldc == g.N && (g.N & 3) == 0 &&", "(g.N & 3) == 0 &&"), ("g.splits <= 64;", "g.splits <= 32;")),
}


def test_walk_constants_match_the_kernel_sources():
    src = read_sources()
    check_source(src)
    # and the check bites: each copied constant or expression, changed in a copy of the text, fails it
    for f, pairs in BITES.items():
        for old, new in pairs:
            assert old in src[f], (f, old)
            with pytest.raises(AssertionError):
                check_source(dict(src, **{f: src[f].replace(old, new)}))


def test_the_host_side_mirrors():
    assert [TG.planes_usable(*a) for a in ((2, 0, 72, 72), (1, 0, 72, 72), (0, 0, 72, 72), (2, 4, 80, 72), (2, 8, 80, 72), (2, 0, 76, 72), (2, 0, 40, 36))] \
        == [True, True, False, False, True, False, False]
    assert [TG.generic_pre(t, a, b, p) for t, a, b, p in ((22, 1, 1, 3), (11, 0, 1, 2), (23, 1, 1, 3), (43, 1, 0, 1), (43, 0, 0, 1), (43, 1, 1, 1), (43, 1, 0, 3),
                                                         (34, 0, 0, 2), (34, 0, 0, 3), (34, 0, 0, 1), (24, 1, 0, 3), (42, 0, 0, 3))] == [3, 2, 0, 1, 1, 0, 0, 2, 3, 0, 0, 0]
    assert [TG.tile_of(v, 9, 2)[:2] for v in (0, 7, 8, 15, 16, 17)] == [(0, 0), (7, 0), (0, 1), (7, 1), (8, 0), (8, 1)]
    assert [TG.tile_of(v, 3, 2) for v in range(6)] == [(0, 0, True), (1, 0, True), (2, 0, True), (0, 1, True), (1, 1, True), (2, 1, True)]
    assert TG.nt_walk(257, 1, 256)[:2] == (256, frozenset((1, 2))) and TG.nt_walk(3, 2, 256)[:2] == (6, frozenset((1,)))
    assert TG.nt_walk(89, 3, 256)[2] is True and TG.nt_walk(130, 2, 256)[2] is False          # (three column tiles: dB goes negative)
    assert [TG.tn_split(K, s) for K, s in ((96, 1), (224, 2), (224, 3), (256, 3), (64, 1), (8288, 4))] == [
        (1, 96, (3,)), (2, 128, (4, 3)), (3, 96, (3, 3, 1)), (3, 96, (3, 3, 2)), (1, 64, (2,)), (4, 2080, (65, 65, 65, 64))]
    assert TG.tn_groups(91, 512, 256, 2) == (1, 4, 8, True, 1) and TG.tn_groups(91, 640, 256, 2) == (1, 5, 16, True, 2)
    assert TG.tn_groups(93, 256, 512, 3) == (1, 2, 8, False, 1) and TG.tn_groups(92, 512, 128, 3) == (1, 2, 8, True, 1)
    assert TG.tn_groups(91, 128, 512, 3) == (1, 2, 8, False, 1) and TG.tn_groups(93, 512, 512, 2) == (2, 2, 16, True, 1)
    E = Epi
    assert [TG.reduce_kind(s, e, ldc, 256) for s, e, ldc in ((1, E(accumulate=True), 256), (3, E(accumulate=True), 256), (3, E(accumulate=True), 260),
                                                              (3, E(bias=True, act0=1), 256), (3, E(accumulate=True, alpha=0.5), 256))] \
        == ["direct", "merge", "kernel", "kernel", "kernel"]
    assert [TG.nt_epilogue(t, e, ldc, al) for t, e, ldc, al in ((82, E(), 128, True), (85, E(), 256, True), (82, E(act_split=48), 128, True), (86, E(), 128, False),
                                                                (83, E(rowv=True, accumulate=True), 192, True), (83, E(rowv=True, maskref=True), 192, True),
                                                                (84, E(), 256, True))] == ["stream", "plain", "generic", "generic", "generic", "stream", "generic"]
    # EPI_IN_SLOT: every two-plane form, no single-plane one
    for t in TG.NT_SINGLE:
        tags2 = TG.plan(TG.Case("nt", t, "NT", 256, TG.NT_WIDTH[t], 64, 2, 2)).tags
        tags1 = TG.plan(TG.Case("nt", t, "NT", 256, TG.NT_WIDTH[t], 64, 1, 2)).tags
        assert ("nt_in_slot", True) in tags2 and ("nt_in_slot", False) in tags1, t


def test_mirrors_against_the_librarys_host_arithmetic(L):
    lib = L.lib()
    t, s = ctypes.c_int(0), ctypes.c_int(0)
    # the plan of the plane-fed NT kernel never picks what the mirror refuses, and refuses what the mirror names
    for M in (4096, 16384, 65536, 65536 + 128):
        for N in (128, 192, 256, 384, 768, 100):
            for K in (32, 64, 96, 100):
                assert lib.advmil_gemm_f32_plan_planes(1, 1, M, N, K, ctypes.byref(t)) == 0
                if t.value:
                    assert t.value in (82, 83) and TG.plan(TG.Case("nt", t.value, "NT", M, N, K, 2, 2)) is not None, (M, N, K, t.value)
                if K < TG.NT_MIN_K or K % 32 or M % 256 or N % 128:
                    assert t.value == 0, (M, N, K)
    assert lib.advmil_gemm_f32_plan_planes(1, 1, 65536, 128, 64, ctypes.byref(t)) == 0 and t.value == 82
    assert lib.advmil_gemm_f32_plan_planes(1, 0, 65536, 128, 64, ctypes.byref(t)) == 0 and t.value == 0
    # ... and so the plan of the TN kernel: tile by divisibility, every split at least a ring deep, no XCD above its 32 CUs
    for M, N in ((128, 256), (512, 256), (256, 128), (512, 128), (256, 256), (256, 512), (768, 384), (384, 1024), (128, 128)):
        for K in (8192, 8192 + 96, 16384, 65536, 4096):
            assert lib.advmil_gemm_f32_plan_tn_planes(M, N, K, ctypes.byref(t), ctypes.byref(s)) == 0
            if not t.value:
                continue
            tm, tn, wr, wc, _ = TG.TN_TABLE[t.value]
            assert M % (32 * tm * wr) == 0 and N % (32 * tn * wc) == 0 and K >= 8192
            splits, k_chunk, chunks = TG.tn_split(K, s.value)
            assert splits == s.value and min(chunks) >= 1 and k_chunk // 32 >= TG.TN_MIN_CHUNKS
            assert TG.plan(TG.Case("tn", t.value, "TN", M, N, K, 2, 2, splits=s.value)) is not None
            assert TG.tn_groups(t.value, M, N, splits)[2] <= 256
            assert lib.advmil_gemm_f32_workspace_bytes(M, N, splits) == (4 * splits * M * N if splits > 1 else 0)
    # gate partial columns and column-sum partial rows from the tile geometry
    for N in (256, 512, 768):
        for tile, (tn, _, _) in TG.NT_TABLE.items():
            if N % (64 * tn) == 0:
                assert lib.advmil_gemm_f32_gate_blocks(tile, N) == N // (64 * tn) * 2, (tile, N)
        for tile, (tm, tn, wr, wc) in TG.GENERIC_GEOM.items():
            assert lib.advmil_gemm_f32_gate_blocks(tile, N) == TG.ceil_div(N, 32 * tn * wc) * wc, (tile, N)
    for tile in (82, 83):
        assert lib.advmil_gemm_f32_colsum_rows(tile, 2304, 384) == 2304 // 64 and lib.advmil_gemm_f32_colsum_rows(tile, 2304 + 64, 384) == 0
    for tile, (tm, tn, wr, wc) in TG.GENERIC_GEOM.items():
        M, N = 32 * tm * wr * 3, 32 * tn * wc * 2
        assert lib.advmil_gemm_f32_colsum_rows(tile, M, N) == (3 * wr if tm * tn >= 4 else 0), tile
    assert lib.advmil_gemm_f32_colsum_rows(85, 2304, 512) == 0                                  # (the plain tiles have no column sums)


def _tiled(lib, L, c, splits=None, ws=False):
    """advmil_gemm_f32_tiled for a Case, on fake addresses laid out as tests/test_gemm_walks_gpu.py lays the real ones out."""
    a_kc, b_kc = TG.R.LAYOUTS[c.lay]
    a_ext, b_ext, lda, ldb = TG.pitches(c)
    e = L.Epilogue()
    e.alpha, e.act_split = 1.0, (1 << 30) if c.epi.act_split is None else c.epi.act_split
    pa, pb = A16 + (1 << 36), A16 + (2 << 36)
    if c.a:
        e.a_hi, e.a_lo = pa + 2 * c.a_off, (pa + (1 << 34) + 2 * c.a_off) if c.a == 2 else None
    if c.b:
        e.b_hi, e.b_lo = pb, (pb + (1 << 34)) if c.b == 2 else None
    n_out = c.epi.n_split or c.N
    if c.epi.n_split:
        e.c2, e.ldc2, e.n_split = A16 + (5 << 36), c.N - n_out, n_out
    e.accumulate = 1 if c.epi.accumulate else 0
    sp = c.splits if splits is None else splits
    wsb = lib.advmil_gemm_f32_workspace_bytes(c.M, c.N, sp)
    return lib.advmil_gemm_f32_tiled(1 if a_kc else 0, 1 if b_kc else 0, c.M, c.N, c.K, ctypes.c_void_p(A16), lda, ctypes.c_void_p(A16 + (3 << 36)), ldb,
                                     ctypes.c_void_p(A16 + (4 << 36) + 4 * c.c_off), n_out + c.ldc_pad, ctypes.byref(e), sp, c.tile,
                                     ctypes.c_void_p(A16 + (6 << 36)) if (ws or wsb) else None, wsb, None)


REFUSED = [
    TG.Case("nt", 82, "NT", 256, 128, 32, 2, 2),                         # K < 64: the ring prefetches two chunks ahead
    TG.Case("nt", 83, "NT", 256, 192, 48, 2, 2),
    TG.Case("nt", 85, "NT", 384, 256, 64, 2, 2),                         # M % 256
    TG.Case("nt", 82, "NT", 256, 192, 64, 2, 2),                         # N no multiple of the tile width
    TG.Case("nt", 83, "NT", 256, 128, 64, 2, 2),
    TG.Case("nt", 85, "NT", 256, 128, 64, 2, 2),
    TG.Case("nt", 86, "NT", 256, 192, 64, 2, 2),
    TG.Case("nt", 82, "NT", 1 << 20, 128, 2048, 2, 2),                   # A's planes span 2^32 bytes
    TG.Case("nt", 82, "NT", 256, 1 << 20, 2048, 2, 2),                   # ... B's
    TG.Case("nt", 82, "NT", 256, 128, 128, 2, 2, splits=2),              # split-K: none for NT
    TG.Case("nt", 82, "NT", 256, 128, 64, 2, 1),                         # a single-plane B has no instantiation
    TG.Case("nt", 82, "NN", 256, 128, 64, 2, 2),                         # NT only
    TG.Case("nt", 82, "NT", 256, 128, 64, 2, 2, a_off=4, a_pad=4),       # planes off 16 bytes: pre != 3
    TG.Case("nt", 82, "NT", 256, 128, 64, 2, 2, a_pad=4),                # pitch % 8
    TG.Case("nt", 85, "NT", 256, 256, 64, 2, 2, epi=Epi(accumulate=True)),                     # the plain tiles: bias + activation only
    TG.Case("nt", 86, "NT", 256, 256, 64, 2, 2, c_off=1, epi=TG.two_layers(256, "no")),        # two layers: the streaming epilogue's alignment
    TG.Case("nt", 86, "NT", 256, 256, 64, 2, 2, ldc_pad=2, epi=TG.two_layers(256, "no")),
    TG.Case("nt", 83, "NT", 256, 384, 64, 2, 2, epi=TG.two_layers(384, "no")),                 # ... and the plain tiles only
    TG.Case("tn", 91, "TN", 128, 256, 64, 2, 2),                         # k_chunk / 32 < 3
    TG.Case("tn", 92, "TN", 256, 128, 128, 2, 2, splits=2),              # ... chunks (2, 2)
    TG.Case("tn", 91, "TN", 128, 256, 96, 1, 2),                         # a single-plane A
    TG.Case("tn", 92, "TN", 128, 128, 96, 2, 2),                         # M % 256
    TG.Case("tn", 91, "TN", 128, 128, 96, 2, 2),                         # N % 256
    TG.Case("tn", 93, "NT", 256, 256, 96, 2, 2),                         # TN only
    TG.Case("tn", 93, "TN", 256, 256, 96, 2, 0),                         # B without planes
]


@pytest.mark.parametrize("c", REFUSED, ids=TG.case_id)
def test_refusals_before_any_launch(L, c):
    """The mirror says `refused`; the library answers ADVMIL_EINVAL (a positive return would be a hipError_t: the call got to a launch)."""
    assert TG.plan(c) is None, c
    assert _tiled(L.lib(), L, c, ws=True) == EINVAL, c


def test_reach_for_a_nominal_device():
    """The same host-side collection tests/test_gemm_walks_gpu.py ends with, here where no GPU is needed to learn that a case went."""
    for ncu in (TG.NOMINAL_CUS, 304, 64):
        assert not TG.WALKS_WANTED - TG.walks_reached(ncu), ncu
    assert all(TG.plan(c, TG.NOMINAL_CUS) is not None for c in TG.all_cases(TG.NOMINAL_CUS))
