"""CPU: what aims the region-network tests is itself pinned. tests/test_region_walks_gpu.py sizes its cases (rows around the 64-row tile,
segment ends inside a tile, the workspace's tile count and the pad columns of a partial row) from constants copied out of
csrc/region.hip. A retune of the kernels must break these tests instead of silently un-aiming the others: the constants are pinned to the
source text and to the library's own workspace arithmetic, which needs no GPU; and the covering set of cases is checked here too, where
no GPU is needed to learn that a walk went."""
import os
import re

import pytest

from tests import test_region_walks_gpu as TRW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REGION_HIP = os.path.join(ROOT, "advmil_amd", "csrc", "region.hip")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from advmil_amd import _lib
    return _lib.lib()


def check_source(src):
    """Every constant the GPU file copies, where region.hip states it. Raises AssertionError on the first that moved."""
    one = lambda pat: re.findall(pat, src, flags=re.M)   # noqa: E731
    assert one(r"^#define RC_ROWS (\d+)$") == [str(TRW.RC_ROWS)]
    assert one(r"^#define RC_D (\d+)$") == [str(TRW.RC_D)]
    assert one(r"^#define RC_H (\d+)$") == [str(TRW.RC_H)]
    # a partial row: dwc 128 | dba 128 | dbb 128 | dbc 1 + 3 pad | db2 128 | db1 64
    assert one(r"^#define RC_PART \((\d+) \* RC_D \+ (\d+) \+ RC_D \+ RC_H\)") == [("3", "4")]
    assert TRW.RC_PART == 3 * TRW.RC_D + 4 + TRW.RC_D + TRW.RC_H == 580 and TRW.RC_PART_PAD == (3 * TRW.RC_D + 1, 3 * TRW.RC_D + 4)
    # who writes and who reads a partial row: dbc at column 3 D, db2 from 3 D + 4, db1 behind it; the merges skip the pad
    assert len(one(r"^\s*prow\[3 \* RC_D\] = t;$")) == 1
    assert len(one(r"prow \+ 3 \* RC_D \+ 4 \+ col\)")) == 1 and len(one(r"prow\[3 \* RC_D \+ 4 \+ RC_D \+ tid\]")) == 1
    assert len(one(r"advmil_sumq\(stream, \(const float\*\)ws, nblk, RC_PART, 3 \* RC_D \+ 1, dwc, 1, dbab, RC_D, dbc, 3 \* RC_D\);")) == 1
    assert len(one(r"advmil_sumq\(stream, \(const float\*\)ws \+ 3 \* RC_D \+ 4, nblk, RC_PART, RC_D \+ RC_H, db2, 1, db1, RC_D\);")) == 1
    # one workgroup per RC_ROWS rows, each way, and the workspace sized by the same count
    assert len(one(r"dim3\(\(unsigned\)\(\(R \+ RC_ROWS - 1\) / RC_ROWS\)\)")) == 1
    assert len(one(r"const int nblk = \(int\)\(\(R \+ RC_ROWS - 1\) / RC_ROWS\);")) == 1
    assert len(one(r"return \(size_t\)\(\(R \+ RC_ROWS - 1\) / RC_ROWS\) \* RC_PART \* sizeof\(float\);")) == 1
    # the dropout draws' flat indices: width RC_H for dx_fc1, RC_D for the gates, each way
    assert len(one(r"\(uint64_t\)\(grow \* RC_H \+ col\)")) == 1 and len(one(r"\(uint64_t\)\(grow \* RC_D \+ col\)")) == 1
    assert len(one(r"\(uint64_t\)\(\(g\.rng_row \? g\.rng_row\[n\] : n\) \* RC_D \+ j\)")) == 1
    # one rule for the seed, each way
    assert len(one(r"const bool d1 = g\.seed && g\.p1 > 0\.f, dg = g\.seed && g\.pg > 0\.f;")) == 1
    assert len(one(r"const bool dg = g\.seed && g\.pg > 0\.f;")) == 1
    assert len(one(r"const float inv1 = \(g\.seed && g\.p1 > 0\.f\) \? hw_rcp\(1\.f - g\.p1\) : 1\.f;")) == 1


def test_walk_constants_match_the_kernel_source():
    src = open(REGION_HIP).read()
    check_source(src)
    # and the check bites: each copied constant, changed in a copy of the text, fails it
    for old, new in (("#define RC_ROWS 64", "#define RC_ROWS 128"), ("#define RC_D 128", "#define RC_D 256"), ("#define RC_H 64", "#define RC_H 128"),
                     ("#define RC_PART (3 * RC_D + 4 + RC_D + RC_H)", "#define RC_PART (3 * RC_D + 8 + RC_D + RC_H)"),
                     ("prow[3 * RC_D] = t;", "prow[3 * RC_D + 1] = t;"),
                     ("(const float*)ws + 3 * RC_D + 4, nblk", "(const float*)ws + 3 * RC_D + 1, nblk"),
                     ("nblk, RC_PART, 3 * RC_D + 1, dwc", "nblk, RC_PART, 3 * RC_D + 4, dwc"),
                     ("(uint64_t)(grow * RC_H + col)", "(uint64_t)(grow * RC_D + col)"),
                     ("const float inv1 = (g.seed && g.p1 > 0.f) ?", "const float inv1 = g.p1 > 0.f ?"),
                     ("dim3((unsigned)((R + RC_ROWS - 1) / RC_ROWS))", "dim3((unsigned)((R + 2 * RC_ROWS - 1) / (2 * RC_ROWS)))")):
        assert old in src, old
        with pytest.raises(AssertionError):
            check_source(src.replace(old, new))


@pytest.mark.parametrize("R", [1, 64, 65, 4097])
def test_workspace_is_one_partial_row_per_tile(lib, R):
    assert lib.advmil_dx_chain_bwd_workspace_bytes(R, 128) == TRW.ceil_div(R, TRW.RC_ROWS) * TRW.RC_PART * 4 == TRW.tiles(R) * 580 * 4


def test_the_parametrisation_reaches_every_walk():
    """The same host-side collection tests/test_region_walks_gpu.py ends with."""
    assert not TRW.WALKS_WANTED - TRW.walks_reached()
    # ... and it bites: without its [1, 300] cases no backward launch spans five tiles, without its noseed cases no pair with that mode
    keep = TRW.BWD_CASES
    try:
        TRW.BWD_CASES = [c for c in keep if c.lens != (1, 300)]
        assert ("bwd", "tiles", 5) in TRW.WALKS_WANTED - TRW.walks_reached()
        TRW.BWD_CASES = [c for c in keep if c.mode != "noseed"]
        assert {("bwd", "pair", "noseed", False), ("bwd", "pair", "noseed", True)} <= TRW.WALKS_WANTED - TRW.walks_reached()
    finally:
        TRW.BWD_CASES = keep


def test_the_case_tables_hold_what_the_issue_lists():
    assert sorted({c.R for c in TRW.FWD_CASES}) == [1, 63, 64, 65, 127, 193]
    assert {c.lens for c in TRW.BWD_CASES} == {(1,), (63,), (64,), (65,), (200,), (1, 300), (30, 1, 20, 77, 64)}
    assert max(max(c.R for c in TRW.FWD_CASES), max(sum(c.lens) for c in TRW.BWD_CASES), sum(TRW.WRAP_LENS)) <= 322
    assert all(c.seg or len(c.lens) == 1 for c in TRW.BWD_CASES)
    assert TRW.WRAP_LENS == (130, 1, 61) and TRW.POISON_CASE.lens == (30, 1, 20, 77, 64) and TRW.POISON_CASE.mode == "both"
