"""CPU: what aims the GENConv tests is itself pinned. tests/test_genconv_gpu.py and tools/probe/graph_fuzz.py work out on the host which
walk of csrc/graph.hip a graph takes (tile size, staged or unstaged edge indices) from three constants copied out of the kernel
source; a retune of the kernels must break these tests instead of silently un-aiming the others. And the fuzz's fixed-seed run of the
suite must reach every walk: checked here, without a GPU, through its --plan mode."""
import importlib.util
import os
import re
import subprocess
import sys

import torch

from tests import test_genconv_gpu as TG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUZZ = os.path.join(ROOT, "tools", "probe", "graph_fuzz.py")


def _fuzz_module():
    spec = importlib.util.spec_from_file_location("graph_fuzz", FUZZ)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_walk_constants_match_the_kernel_source():
    src = open(os.path.join(ROOT, "advmil_amd", "csrc", "graph.hip")).read()
    one = lambda pat: re.findall(pat, src, flags=re.M)
    assert one(r"^constexpr int GT_EDGES = (\d+);") == ["2048"]
    assert one(r"^constexpr int GT_MAXS = (\d+);") == ["16"]
    assert one(r"^\s*int64_t s = N / \((\d+) \* (\d+)\);") == [("8", "512")]
    assert one(r"^\s*s = s < 1 \? 1 : \(s > GT_MAXS \? GT_MAXS : s\);\n\s*return \(int\)\((\d+) \* s\);") == ["8"]
    assert one(r"^#define GENCONV_BWD_CH (\d+)") == ["4"]
    assert one(r"staged\(int nt\) const \{ return rp\[nt\] - rp\[0\] (\S+) GT_EDGES; \}") == ["<="]
    assert len(one(r"node_chunk<8>\(te, h, nt\)")) == 1 and len(one(r"node_chunk<CH>\(te, h, nt\)")) == 1
    fz = _fuzz_module()
    for mod in (TG, fz):
        assert (mod.GT_EDGES, mod.GT_MAXS, mod.TILE_DIV) == (2048, 16, 8 * 512), mod.__name__
    assert (TG.FWD_CH, TG.BWD_CH) == (8, 4)


def test_the_host_side_mirror_of_the_tiling():
    assert [TG.tile_nodes_for(n) for n in (1, 4095, 8191, 8192, 12301, 65535, 65536, 65549, 1 << 20)] == [8, 8, 8, 16, 24, 120, 128, 128, 128]
    # 20 nodes, tiles of 8: degrees 3 x 8 | 0 x 8 | 5 x 4
    deg = torch.tensor([3] * 8 + [0] * 8 + [5] * 4)
    key = torch.repeat_interleave(torch.arange(20), deg)
    f = TG.walk_facts(TG.rowptr_of(key, 20), 20)
    assert f == TG.Facts(1, 24, 5, [24, 0, 20])
    fz = _fuzz_module()
    assert fz.tile_facts(key, 20) == (1, 24)
    for name in ("ladder_s2", "unstaged_forward", "unstaged_backward"):      # the shared graphs are where they claim to be
        ei, N = TG.named_graph(name)
        assert fz.tile_facts(ei[1], N) == (TG.facts_of(ei, N)[0].S, TG.facts_of(ei, N)[0].tile_max)


def test_the_suites_fuzz_arguments_reach_every_walk():
    """tests/test_fuzz_gpu.py runs `graph_fuzz.py 40 104`: the same draws must hold a C == 128 case with S > 1, with an unstaged
    forward tile, with an unstaged backward tile and with t < 0."""
    r = subprocess.run([sys.executable, FUZZ, "40", "104", "--plan"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 41 and all(re.match(r"case \d+: \w+ graph N \d+ E \d+ C \d+ t -?[\d.]+: S \d+ forward tile \d+ backward tile \d+ sign [-+]$", ln)
                                    for ln in lines[:-1]), r.stdout[-2000:]
    m = re.match(r"plan; 40 cases; C == 128 cases with S > 1: (\d+); forward unstaged: (\d+); backward unstaged: (\d+); t < 0: (\d+)$", lines[-1])
    assert m and all(int(v) > 0 for v in m.groups()), lines[-1]
    # the counts are those of the printed cases
    wide = [ln for ln in lines[:-1] if " C 128 " in ln]
    num = lambda ln, pat: int(re.search(pat, ln).group(1))
    assert int(m.group(1)) == sum(num(ln, r": S (\d+)") > 1 for ln in wide)
    assert int(m.group(2)) == sum(num(ln, r"forward tile (\d+)") > 2048 for ln in wide)
    assert int(m.group(3)) == sum(num(ln, r"backward tile (\d+)") > 2048 for ln in wide)
    assert int(m.group(4)) == sum(ln.endswith("sign -") for ln in wide)
