"""CPU: what aims the attention walk tests is itself pinned. tests/test_attn_walks_gpu.py works out on the host which walk of
csrc/attn.hip / attn_bwd1.hip a launch takes (tests/attn_ref.py::walk_facts) from constants copied out of the kernel sources. A retune
of the kernels must break these tests instead of silently un-aiming the others: the constants are pinned to the source text, and the
mirror to the library's own workspace arithmetic, which needs no GPU."""
import os
import re

import numpy as np
import pytest

from advmil_amd import synth
from tests import attn_ref as AR
from tests import test_attn_walks_gpu as TW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "advmil_amd", "csrc")
FILES = ("attn_core.h", "attn.hip", "attn_bwd1.hip")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from advmil_amd import _lib
    return _lib.lib()


def sources():
    return {f: open(os.path.join(CSRC, f)).read() for f in FILES}


def check_source(src):
    """Every constant the mirror copies, where the three files state it. Raises AssertionError on the first that moved."""
    core, attn, bwd1 = (src[f] for f in FILES)
    one = lambda pat, s: re.findall(pat, s, flags=re.M)   # noqa: E731
    # tiles: 256 stationary rows per workgroup, 64 streamed rows per tile, 32 streamed queries per trip of the single pass
    assert one(r"^#define AT_QB (\d+)\b", core) == [str(AR.AT_QB)]
    assert one(r"^#define AT_KT (\d+)\b", core) == [str(AR.AT_KT)]
    assert one(r"^#define B1_QT (\d+)\b", bwd1) == [str(AR.B1_QT)]
    assert one(r"const int64_t ntile = \(max_len \+ AT_QB - 1\) / AT_QB;", core) == ["const int64_t ntile = (max_len + AT_QB - 1) / AT_QB;"]
    assert len(one(r"const int T = \(int\)\(\(Lg \+ AT_KT - 1\) / AT_KT\);", attn)) == 3          # forward, dQ, dK/dV
    assert len(one(r"const int T = \(int\)\(\(Lg \+ B1_QT - 1\) / B1_QT\);", bwd1)) == 1
    # the workgroups of a raised grid return
    assert len(one(r"if \(\(int64_t\)qt \* AT_QB >= Lg\) return;", attn)) == 2
    assert len(one(r"if \(\(int64_t\)kt \* AT_QB >= Lg\) return;", attn)) == 1
    assert len(one(r"if \(\(int64_t\)kt \* AT_QB >= Lg\) return;", bwd1)) == 1
    # the forward's ring start: two slots, the second issue and the counted wait only with a second tile
    assert len(one(r"if \(T > 1\) dma\.issue\(smem, wave, 1, AT_KT,", attn)) == 3
    assert len(one(r"if \(T > 1\) at_wait_vmcnt<AT_PPW>\(\); else at_wait_vmcnt<0>\(\);", attn)) == 1
    assert one(r"unsigned char smem\[(\d) \* AT_SLOT_B", attn) == ["2", "3", "3"]
    # the reduce: 32 rows per workgroup, the bags on grid y, key blocks by four plus remainder
    assert one(r"const int rows_per_wg = (\d+);", bwd1) == [str(AR.REDUCE_ROWS)]
    assert len(one(r"const dim3 rgrid\(\(unsigned\)\(\(max_len \+ rows_per_wg - 1\) / rows_per_wg\), \(unsigned\)nseg\);", bwd1)) == 1
    assert len(one(r"if \(rb >= Lg\) return;", bwd1)) == 1
    assert one(r"for \(; kb \+ (\d) <= nkb; kb \+= (\d)\) \{", bwd1) == [(str(AR.REDUCE_UNROLL),) * 2]
    assert len(one(r"for \(; kb < nkb; \+\+kb\) \{", bwd1)) == 1
    assert len(one(r"const int nkb = \(int\)\(\(Lg \+ AT_QB - 1\) / AT_QB\);", bwd1)) == 1
    # the prep kernel's blocks
    assert one(r"const int pbt = head_dim == (\d+) \? (\d+) : (\d+);", attn) == [("48", "192", "256")]
    assert len(one(r"const int64_t png = pbt / \(head_dim / 4\);", attn)) == 1
    assert one(r"constexpr int BT = HD == (\d+) \? (\d+) : (\d+), G = HD / 4, NG = BT / G;", attn) == [("48", "192", "256")]
    assert (AR.prep_threads(48), AR.prep_threads(16)) == (192, 256)
    # the head dims that are built, KS / DT / pad units
    assert one(r"if \(head_dim != (\d+) && head_dim != (\d+) && head_dim != (\d+) && head_dim != (\d+)\) return ADVMIL_EINVAL;", core) \
        == [tuple(str(h) for h in AR.HEAD_DIMS)]
    assert len(one(r"constexpr int KS = HD / 16, DT = \(HD \+ 31\) / 32, UN = HD / 8;", attn)) == 3
    assert len(one(r"constexpr int UN = HD / 8, UP = 4 \* \(\(HD \+ 31\) / 32\) - UN;", core)) == 1
    # the dropout threshold and scale
    assert len(one(r"a\.drop_thr = drop \? \(uint32_t\)\(\(double\)drop_p \* 256\.0\) : 0u;", core)) == 1
    assert len(one(r"a\.inv_keep = drop \? 256\.0f / \(256\.0f - \(float\)a\.drop_thr\) : 1\.0f;", core)) == 1
    # head and row key for any head count
    assert len(one(r"const int h = blockIdx\.x % H;", attn)) == 3 and len(one(r"const int h = blockIdx\.x % H;", bwd1)) == 1


MUTATIONS = (
    ("attn_core.h", "#define AT_QB 256 ", "#define AT_QB 128 "), ("attn_core.h", "#define AT_KT 64 ", "#define AT_KT 32 "),
    ("attn_bwd1.hip", "#define B1_QT 32 ", "#define B1_QT 64 "), ("attn_bwd1.hip", "const int rows_per_wg = 32;", "const int rows_per_wg = 64;"),
    ("attn_bwd1.hip", "for (; kb + 4 <= nkb; kb += 4) {", "for (; kb + 2 <= nkb; kb += 2) {"),
    ("attn_bwd1.hip", "for (; kb < nkb; ++kb) {", "for (; kb + 1 < nkb; ++kb) {"),
    ("attn.hip", "const int pbt = head_dim == 48 ? 192 : 256;", "const int pbt = head_dim == 48 ? 192 : 128;"),
    ("attn.hip", "const int64_t png = pbt / (head_dim / 4);", "const int64_t png = pbt / (head_dim / 8);"),
    ("attn.hip", "if ((int64_t)qt * AT_QB >= Lg) return;", "if ((int64_t)qt * AT_QB > Lg) return;"),
    ("attn_bwd1.hip", "if ((int64_t)kt * AT_QB >= Lg) return;", "if ((int64_t)kt * AT_QB > Lg) return;"),
    ("attn_bwd1.hip", "if (rb >= Lg) return;", "if (rb > Lg) return;"),
    ("attn_core.h", "head_dim != 48 && head_dim != 64", "head_dim != 48 && head_dim != 96"),
    ("attn_core.h", "(uint32_t)((double)drop_p * 256.0)", "(uint32_t)((double)drop_p * 256.0 + 0.5)"),
    ("attn_core.h", "256.0f / (256.0f - (float)a.drop_thr)", "1.0f / (1.0f - drop_p)"),
    ("attn.hip", "if (T > 1) at_wait_vmcnt<AT_PPW>(); else at_wait_vmcnt<0>();", "at_wait_vmcnt<0>();"),
    ("attn.hip", "constexpr int KS = HD / 16, DT = (HD + 31) / 32, UN = HD / 8;", "constexpr int KS = HD / 16, DT = (HD + 15) / 16, UN = HD / 8;"),
)


def test_walk_constants_match_the_kernel_sources():
    src = sources()
    check_source(src)
    # and the check bites: each copied constant, changed in a copy of the text, fails it
    for f, old, new in MUTATIONS:
        assert old in src[f], (f, old)
        with pytest.raises(AssertionError):
            check_source({**src, f: src[f].replace(old, new, 1)})


def test_the_mirror():
    w = AR.walk_facts([1, 64, 65, 257, 1025], 48, 8)
    assert [b.key_tiles for b in w.bags] == [1, 1, 2, 5, 17] and [b.last_fill for b in w.bags] == [1, 64, 1, 1, 1]
    assert [b.last_half for b in AR.walk_facts([32, 33], 16, 8).bags] == ["first", "second"]
    assert [(b.q_tiles, b.last_q_valid, b.idle_waves) for b in w.bags] == [(1, 1, 7), (1, 64, 6), (1, 65, 5), (2, 1, 7), (5, 1, 7)]
    assert [(b.trips, b.last_trip_parity) for b in w.bags] == [(1, 0), (2, 1), (3, 0), (9, 0), (33, 0)]
    assert [(b.nkb, b.nkb_groups, b.nkb_rem) for b in w.bags] == [(1, 0, 1), (1, 0, 1), (1, 0, 1), (2, 0, 2), (5, 1, 1)]
    assert [(b.reduce_wgs, b.reduce_idle) for b in w.bags] == [(33, 32), (33, 31), (33, 30), (33, 24), (33, 0)]
    assert [(b.main_wgs, b.main_idle) for b in w.bags] == [(5, 4), (5, 4), (5, 4), (5, 3), (5, 0)]
    assert (w.max_len, w.L_total, w.prep_blocks, w.prep_partial) == (1025, 1412, 706, False)
    assert [AR.prep_pairs(h) for h in AR.HEAD_DIMS] == [64, 32, 16, 16]
    assert [(x.KS, x.DT, x.pad_units) for x in (AR.walk_facts([1], h, 8) for h in AR.HEAD_DIMS)] == [(1, 1, 2), (2, 1, 0), (3, 2, 2), (4, 2, 0)]
    w = AR.walk_facts([65, 257], 48, 8, max_len=600)
    assert [(b.main_wgs, b.main_idle, b.reduce_wgs, b.reduce_idle) for b in w.bags] == [(3, 2, 19, 16), (3, 1, 19, 10)]
    assert AR.walk_facts([1, 2], 16, 8).prep_partial and not AR.walk_facts([8], 16, 8).prep_partial
    with pytest.raises(AssertionError):
        AR.walk_facts([65, 257], 48, 8, max_len=256)
    with pytest.raises(AssertionError):
        AR.walk_facts([65], 40, 8)


def test_dropout_threshold_and_scale():
    for p, thr in ((1 / 256, 1), (0.1, 25), (0.25, 64), (0.5, 128), (255 / 256, 255)):
        assert AR.drop_thr(p) == thr and AR.inv_keep(p) == 256.0 / (256 - thr) == synth.attn_dropout_scale(p)
        keep = synth.attn_dropout_keep(3, 1, np.arange(64), 8, 0, 1024, p)
        assert abs(keep.mean() - (1 - thr / 256)) < 8e-3


@pytest.mark.parametrize("lens,max_len", [((1,), None), ((1, 2), None), ((5, 32), None), ((65, 257), None), ((65, 257), 600),
                                          ((65, 257), 322), ((1025,), None), ((700, 257, 33, 1025, 1), None)])
def test_mirror_against_the_librarys_workspace_arithmetic(lib, lens, max_len):
    """advmil_mha_bwd_workspace_bytes = D | dO hi | dO lo, advmil_mha_bwd1_workspace_bytes the same + ceil(max_len / 256) partial slabs:
    the slab count is the mirror's workgroups per (bag, head) of the main grids."""
    for hd in AR.HEAD_DIMS:
        for nhead in (1, 3, 8, 16):
            w = AR.walk_facts(lens, hd, nhead, max_len)
            Lt = w.L_total
            two = lib.advmil_mha_bwd_workspace_bytes(Lt, nhead, hd)
            one = lib.advmil_mha_bwd1_workspace_bytes(Lt, nhead, hd, w.max_len)
            assert two == AR.bwd_workspace_bytes(Lt, nhead, hd) and one == AR.bwd1_workspace_bytes(Lt, nhead, hd, w.max_len)
            assert (one - two) % (4 * Lt * nhead * hd) == 0 and (one - two) // (4 * Lt * nhead * hd) == w.bags[0].main_wgs
            assert two >= 4 * Lt * nhead          # D lies first: what ops.MhaFn.keep_dsum copies out


def test_the_parametrisation_reaches_every_walk():
    """The same host-side collection tests/test_attn_walks_gpu.py ends with, here where no GPU is needed to learn that a case went:
    walk_facts over every case's arguments."""
    assert not TW.WALKS_WANTED - TW.walks_reached()
    # and the collection can miss: without the single-bag and query-tile cases some walks are not reached
    got = set()
    for c in TW.RING[:8]:
        got |= AR.walk_tags(TW.facts(c), c.hd, c.nhead, c.p)
    assert TW.WALKS_WANTED - got
