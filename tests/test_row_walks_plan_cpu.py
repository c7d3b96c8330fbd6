"""CPU: what aims the row-kernel tests is itself pinned. tests/test_row_walks_gpu.py works out on the host which walk of csrc/pool.hip
a shape takes (rows per block, the online / statistics forms of the pooling call, the backward's row walks, the gate score's three
walks, the LayerNorm kernel families, direct or merged column sums) from constants copied out of the kernel source. A retune of the
kernels must break these tests instead of silently un-aiming the others: the constants are pinned to the source text, and the mirrors
to the library's own workspace arithmetic, which needs no GPU."""
import os
import re

import pytest

from tests import test_row_walks_gpu as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POOL_HIP = os.path.join(ROOT, "advmil_amd", "csrc", "pool.hip")
MAX_LENS = (1, 32, 33, 32768, 32769, 491520, 491521, 1048576, 1048577, 1049089)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from advmil_amd import _lib
    return _lib.lib()


def check_source(src):
    """Every constant the mirrors copy, where pool.hip states it. Raises AssertionError on the first that moved."""
    one = lambda pat: re.findall(pat, src, flags=re.M)   # noqa: E731
    # rows_per_block(): ceil(rows / 1024), up to a multiple of 32, clamped to [ROWS_PER_BLOCK, 512]
    assert one(r"^#define ROWS_PER_BLOCK (\d+)$") == [str(TR.ROWS_PER_BLOCK)]
    assert one(r"^\s*int64_t r = \(rows \+ (\d+)\) / (\d+);$") == [(str(TR.RPB_DIV - 1), str(TR.RPB_DIV))]
    assert one(r"^\s*r = \(r \+ (\d+)\) / (\d+) \* (\d+);$") == [("31", "32", "32")]
    assert len(one(r"^\s*if \(r < ROWS_PER_BLOCK\) r = ROWS_PER_BLOCK;$")) == 1
    assert one(r"^\s*if \(r > (\d+)\) r = (\d+);$") == [(str(TR.RPB_CAP), str(TR.RPB_CAP))]
    assert one(r"__shared__ float wts\[(\d+)\];") == [str(TR.RPB_CAP)]
    # the pooling call: which form
    assert one(r"^#define POOL_ONLINE_MAX_NBLK (\d+)$") == [str(TR.POOL_ONLINE_MAX_NBLK)]
    assert len(one(r"if \(\(D & 7\) == 0 && D >= 16 && nblk <= POOL_ONLINE_MAX_NBLK\) \{")) == 1
    assert len(one(r"^\s*if \(mean \|\| hlo\) return ADVMIL_EINVAL;")) == 1
    assert len(one(r"^\s*if \(\(D & 7\) == 0 && D >= 16\)\n\s*hipLaunchKernelGGL\(pool_partial8_kernel,")) == 1
    assert len(one(r"\(D & 3\) \|\| D > 1024 \|\| \(ldh & 3\)\) return ADVMIL_EINVAL;")) == 1
    assert one(r"__shared__ float sc\[(\w+)\];") == ["POOL_ONLINE_MAX_NBLK"]
    # its backward
    assert one(r"^#define PBD_ROWS (\d+)$") == [str(TR.PBD_ROWS)]
    assert len(one(r"const int nwg = \(int\)\(\(max_len \+ 4 \* PBD_ROWS - 1\) / \(4 \* PBD_ROWS\)\);")) == 1
    assert len(one(r"if \(\(D & 3\) == 0 && \(ldh & 3\) == 0\) \{")) == 1
    assert len(one(r"if \(hlo && \(\(\(uintptr_t\)hlo & 15\) \|\| \(D & 7\) \|\| \(ldh & 7\) \|\| \(\(\(uintptr_t\)dpooled\) & 15\)\)\) return ADVMIL_EINVAL;")) == 1
    # the gate score
    assert one(r"int64_t blocks = \(N \+ 3\) / 4;\n\s*if \(blocks > (\d+)\) blocks = (\d+);") == [(str(TR.GATE_SCORE_MAXBLK),) * 2]
    assert one(r"if \(\(D & 3\) == 0 && D4 == (\d+)\) \{") == [str(TR.GATE_PAIR_D4)]
    assert one(r"if \(\(D & 3\) == 0 && D4 <= (\d+)\) \{") == [str(TR.GATE_F4_MAX_D4)]
    # LayerNorm: the generic kernels by width, the 16-byte kernels by d / 128
    assert one(r"if \(\(d\) <= (\d+)\) hipLaunchKernelGGL\(\(kernel<(\d+)>\)") == [(str(lim), str(q)) for lim, q in TR.LN_QT_STEPS[:3]]
    assert one(r"^\s*else hipLaunchKernelGGL\(\(kernel<(\d+)>\)") == [str(TR.LN_QT_STEPS[3][1])]
    assert one(r"switch \(\(int\)\(\(d\) / (\d+)\)\)") == ["128"]
    assert one(r"case (\d): hipLaunchKernelGGL\(\(kernel<(\d)>\)") == [("1", "1"), ("2", "2"), ("3", "3")]
    assert one(r"default: hipLaunchKernelGGL\(\(kernel<(\d)>\)") == ["4"]
    assert len(one(r"if \(g_ln4 && \(d & 127\) == 0 && ")) == 2
    assert one(r"d <= 0 \|\|\s+d > (\d+)") == ["512"] * 6
    assert one(r"^#define LN_BWD_MAXBLK (\d+)$") == [str(TR.LN_BWD_MAXBLK)]
    # column sums: 1024-column chunks, direct when one block sees every row and the destination is aligned
    assert one(r"for \(int64_t c0 = 0; c0 < N; c0 \+= (\d+)\) \{") == [str(TR.COLSUM_CHUNK)] * 2
    assert one(r"const int64_t W = \(N - c0 < (\d+)\) \? \(N - c0\) : (\d+);") == [(str(TR.COLSUM_CHUNK),) * 2] * 2
    assert len(one(r"const bool direct = nblk == 1 && \(\(\(uintptr_t\)out\) & 15\) == 0;")) == 1
    assert len(one(r"const bool direct = dbias && nblk == 1 && \(\(\(uintptr_t\)dbias\) & 15\) == 0;")) == 1


def test_walk_constants_match_the_kernel_source():
    src = open(POOL_HIP).read()
    check_source(src)
    # and the check bites: each copied constant, changed in a copy of the text, fails it
    for old, new in (("#define ROWS_PER_BLOCK 32", "#define ROWS_PER_BLOCK 64"), ("(rows + 1023) / 1024", "(rows + 2047) / 2048"),
                     ("if (r > 512) r = 512;", "if (r > 256) r = 256;"), ("#define POOL_ONLINE_MAX_NBLK 2048", "#define POOL_ONLINE_MAX_NBLK 1024"),
                     ("#define PBD_ROWS 4", "#define PBD_ROWS 8"), ("#define LN_BWD_MAXBLK 2048", "#define LN_BWD_MAXBLK 4096"),
                     ("if (blocks > 8192) blocks = 8192;          // grid-stride over rows", "if (blocks > 4096) blocks = 4096;"),
                     ("D4 == 96", "D4 == 64"), ("D4 <= 128", "D4 <= 256"), ("c0 < N; c0 += 1024", "c0 < N; c0 += 512"),
                     ("if ((d) <= 128) hipLaunchKernelGGL((kernel<2>)", "if ((d) <= 64) hipLaunchKernelGGL((kernel<2>)"),
                     ("case 3: hipLaunchKernelGGL((kernel<3>)", "case 3: hipLaunchKernelGGL((kernel<4>)"),
                     ("D >= 16 && nblk <= POOL_ONLINE_MAX_NBLK", "D >= 32 && nblk <= POOL_ONLINE_MAX_NBLK")):
        assert old in src, old
        with pytest.raises(AssertionError):
            check_source(src.replace(old, new))


def test_the_host_side_mirrors():
    assert [TR.rows_per_block(n) for n in (1, 32768, 32769, 65536, 65537, 491520, 491521, 1 << 24)] == [32, 32, 64, 64, 96, 480, 512, 512]
    assert TR.pool_walk(513, 384) == TR.PoolWalk("online", 32, 17)
    assert TR.pool_walk(500000, 16) == TR.PoolWalk("online", 512, 977)
    assert TR.pool_walk(1048576, 16) == TR.PoolWalk("online", 512, 2048) and TR.pool_walk(1048577, 16) == TR.PoolWalk("stats8", 512, 2049)
    assert TR.pool_walk(1049089, 16) == TR.PoolWalk("stats8", 512, 2050)
    assert TR.pool_walk(1049089, 16, mean=True) is None and TR.pool_walk(1049089, 16, planes=True) is None
    assert [TR.pool_walk(513, D).form for D in (4, 8, 12, 16, 20, 24, 1020, 1024)] == ["stats4", "stats4", "stats4", "online", "stats4", "online", "stats4", "online"]
    assert TR.pool_walk(513, 8, mean=True) is None and TR.pool_walk(513, 8, planes=True) is None and TR.pool_walk(513, 6) is None
    assert [TR.pool_bwd_walk(D, ldh, pl) for D, ldh, pl in ((384, 384, True), (24, 28, True), (260, 264, False), (6, 8, False), (130, 132, False), (6, 6, False))] \
        == ["planes", None, "float4", "scalar", "scalar", None]
    assert [TR.gate_score_walk(D) for D in (4, 6, 20, 256, 260, 384, 512, 516)] == ["float4", "scalar", "float4", "float4", "float4", "pair", "float4", "scalar"]
    assert [TR.gate_score_blocks(N) for N in (1, 5, 32768, 32771, 65539)] == [1, 2, 8192, 8192, 8192]
    assert [TR.ln_walk(d, True) for d in (4, 128, 129, 256, 320, 384, 385, 512)] == [
        ("generic", 2), ("ln4", 1), ("generic", 4), ("ln4", 2), ("generic", 6), ("ln4", 3), ("generic", 8), ("ln4", 4)]
    assert [TR.ln_walk(d, False) for d in (128, 256, 384, 512)] == [("generic", 2), ("generic", 4), ("generic", 6), ("generic", 8)]
    assert TR.ln_walk(128, False, planes=True) is None and TR.ln_walk(200, True, dup=2) is None and TR.ln_walk(513, True) is None
    assert TR.colsum_walk(32, 260, True) == TR.ColsumWalk("direct", 1, 32, 1) and TR.colsum_walk(32, 260, False).form == "merged"
    assert TR.colsum_walk(33, 2052, True) == TR.ColsumWalk("merged", 3, 32, 2) and TR.colsum_walk(32801, 4, True) == TR.ColsumWalk("merged", 1, 64, 513)


@pytest.mark.parametrize("max_len", MAX_LENS)
def test_mirrors_against_the_librarys_workspace_arithmetic(lib, max_len):
    """advmil_softmax_pool_workspace_bytes = 4 max(4 nseg + nseg nblk (D + 2), 4 + nseg ceil(max_len / 4)): at D = 1024 the first term
    wins for every max_len and yields nblk; the colsum and gate-backward workspaces yield their block counts the same way."""
    ws = lib.advmil_softmax_pool_workspace_bytes
    for D, nseg in ((1024, 1), (16, 1), (4, 3), (384, 16)):
        w = TR.pool_walk(max_len, D)
        assert ws(max_len, D, nseg) == 4 * max(4 * nseg + nseg * w.nblk * (D + 2), 4 + nseg * TR.ceil_div(max_len, 4)), (D, nseg)
    nblk = (ws(max_len, 1024, 1) // 4 - 4) // 1026
    assert (ws(max_len, 1024, 1) // 4 - 4) % 1026 == 0 and nblk == TR.pool_walk(max_len, 1024).nblk == TR.ceil_div(max_len, TR.rows_per_block(max_len))
    assert lib.advmil_softmax_pool_mean_workspace_bytes(max_len, 16, 2) == (ws(max_len, 16, 2) + 15) // 16 * 16 + 4 * 2 * nblk * 16
    assert lib.advmil_colsum_workspace_bytes(max_len, 4) == 4 * 4 * TR.colsum_walk(max_len, 4, True).nblk == 16 * nblk
    assert lib.advmil_gate_bwd_workspace_bytes(max_len, 4) == 4 * nblk * (3 * 4 + 4)
    assert TR.pool_bwd_partials(max_len) <= TR.ceil_div(max_len, 4)          # the backward's partials fit the second term


def test_ln_backward_workspace_is_capped_at_its_block_limit(lib):
    for nreg in (1, 2047, 2048, 2049, 2051):
        assert lib.advmil_ln_relu_mean16_bwd_workspace_bytes(16 * nreg, 128) == 4 * TR.ln_bwd_blocks(nreg) * 3 * 128
        assert lib.advmil_ln_relu_bwd_workspace_bytes(16 * nreg - 15, 200) == 4 * TR.ln_bwd_blocks(nreg) * 3 * 200


def test_the_parametrisation_reaches_every_walk():
    """The same host-side collection tests/test_row_walks_gpu.py ends with, here where no GPU is needed to learn that a case went."""
    assert not TR.WALKS_WANTED - TR.walks_reached()
