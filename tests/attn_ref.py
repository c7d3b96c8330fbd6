"""No GPU: what tests/test_attn_walks_gpu.py judges the attention core (csrc/attn.hip, attn_bwd1.hip, attn_core.h) with.

  oracle        float64 softmax(Q K^T / sqrt(hd)) (o mask) V per (bag, head) on the packed rows, any nhead / head_dim, with the stored
                statistics (log2-domain log-sum-exp, D = rowsum(dO o O)) and the gradients from autograd on the float64 graph;
  block_errors  per tensor part (O; dQ, dK, dV; lse; D) the worst ratio over (bag, head) blocks of max|got - ref| to THAT block's
                max|ref| -- a long bag's rows are not judged against a short bag's scale;
  model         the kernels' arithmetic in float32 on the host (operands as hi + lo bf16 planes, lo.lo left out; probabilities and dS
                split in two bf16; exp2(float32(s c - m)); fp32 sums): its distance to the oracle on the same inputs is e_model;
  walk_facts    plain-Python mirror of which walk of the kernels a (lens, hd, nhead, max_len) launch takes. What it copies from the
                source is pinned to the source text by tests/test_attn_walks_plan_cpu.py.
"""
import math
from collections import namedtuple

import numpy as np
import torch

from advmil_amd import synth

# ---- copied from csrc/attn_core.h / attn.hip / attn_bwd1.hip (pinned by tests/test_attn_walks_plan_cpu.py)
AT_QB = 256            # stationary rows per workgroup
AT_KT = 64             # streamed rows per LDS tile (forward, two-launch backward)
B1_QT = 32             # streamed queries per trip of the single-pass backward
REDUCE_ROWS = 32       # rows_per_wg of attn_dq_reduce_kernel
REDUCE_UNROLL = 4      # `kb + 4 <= nkb`
HEAD_DIMS = (16, 32, 48, 64)
PROJECT_BOUND = {"O": 1e-5, "lse": 1e-5, "D": 1e-5, "dQ": 5e-5, "dK": 5e-5, "dV": 5e-5}
PARTS = ("O", "lse", "dQ", "dK", "dV", "D")
FP32_TINY = 2.0 ** -126


def ceil_div(a, b):
    return -(-int(a) // int(b))


def prep_threads(hd):
    return 192 if hd == 48 else 256


def prep_pairs(hd):
    """(row, head) pairs per block of attn_bwd_prep_kernel: 64 / 32 / 16 / 16 at head_dim 16 / 32 / 48 / 64."""
    return prep_threads(hd) // (hd // 4)


def drop_thr(p):
    """floor(256 p) of the float the ABI receives."""
    return int(float(np.float32(p)) * 256.0) if p > 0 else 0


def inv_keep(p):
    return 256.0 / (256.0 - drop_thr(p))


# ---------------------------------------------------------------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------------------------------------------------------------
def host_masks(seed, sid, lens, p, nhead=8, rowoff=None, scale=None):
    """Per bag float64 [nhead, L, L]: keep(i, j) * scale from the kernels' counter hash (synth.attn_dropout_keep). `scale` defaults to
    the kernels' own 256 / (256 - floor(256 p)) (synth.attn_dropout_scale; equal to 1 / (1 - p) where p is a multiple of 1/256)."""
    sc = synth.attn_dropout_scale(p) if scale is None else scale
    out, r0 = [], 0
    for b, L in enumerate(lens):
        rows = np.arange(L) + r0 + (0 if rowoff is None else int(rowoff[b]))
        m = np.stack([synth.attn_dropout_keep(seed, sid, rows, nhead, h, L, p) for h in range(nhead)])
        out.append(torch.from_numpy(m.astype(np.float64) * sc))
        r0 += L
    return out


def _heads(blk, nhead, hd):
    L = blk.shape[0]
    return tuple(t.reshape(L, nhead, hd).transpose(0, 1) for t in blk.split(nhead * hd, dim=1))


def ref_attention(qkv, lens, masks=None, nhead=8, hd=48, want_lse=False):
    """float64: per bag and head softmax(q k^T / sqrt(hd)) (* mask) v on the packed [L_total, 3 * nhead * hd] rows; with want_lse also
    the log2-domain log-sum-exp [L_total, nhead] of the scaled scores (no mask: the kernels' row sum is taken before the dropout)."""
    outs, lses, r0 = [], [], 0
    d = nhead * hd
    for b, L in enumerate(lens):
        q, k, v = _heads(qkv[r0:r0 + L], nhead, hd)
        s = q @ k.transpose(-1, -2) / hd ** 0.5
        pr = torch.softmax(s, dim=-1)
        if masks is not None:
            pr = pr * masks[b]
        outs.append((pr @ v).transpose(0, 1).reshape(L, d))
        if want_lse:
            lses.append((torch.logsumexp(s, dim=-1) / math.log(2.0)).transpose(0, 1))
        r0 += L
    o = torch.cat(outs, dim=0)
    return (o, torch.cat(lses, dim=0)) if want_lse else o


def oracle(qkv, go, lens, nhead, hd, masks=None):
    """-> dict of float64 tensors: O [L, d], lse [L, nhead], D [L, nhead], dQ / dK / dV [L, d] (autograd of sum(O * go)), and the
    inputs themselves (`qkv`, `dO`), which block_errors needs for the blocks whose dQ / dK are identically zero."""
    d = nhead * hd
    r = qkv.detach().double().clone().requires_grad_(True)
    g = go.detach().double()
    o, lse = ref_attention(r, lens, masks, nhead, hd, want_lse=True)
    (o * g).sum().backward()
    o = o.detach()
    D = (o * g).reshape(-1, nhead, hd).sum(-1)
    return {"O": o, "lse": lse.detach(), "D": D, "dQ": r.grad[:, :d], "dK": r.grad[:, d:2 * d], "dV": r.grad[:, 2 * d:],
            "qkv": r.detach(), "dO": g}


# ---------------------------------------------------------------------------------------------------------------------------------
# the error measure
# ---------------------------------------------------------------------------------------------------------------------------------
def block_errors(got, ref, lens, nhead, hd, degenerate=()):
    """Per part present in both `got` and `ref`: (worst ratio, (bag, head)) over the (bag, head) blocks of max|got - ref| over that
    block's own max|ref|. A block whose reference is all zero, or below the smallest normal fp32 number throughout (probabilities that
    underflow in fp32 and not in float64), must be all zero (ratio inf otherwise).

    dQ and dK of a one-row bag are identically zero in float64 (softmax over one key is constant); what the kernel leaves there is the
    round-off of dO.v against D. Those blocks -- and those of the bags listed in `degenerate`, whose probabilities are one-hot or whose
    dP is constant along the keys, so that dS vanishes the same way -- are measured against the float64 value
    max_row |D| * max|k| / sqrt(hd) (resp. max|q|) of that bag and head instead (|D| = |dO . O| is |dO.v| times the dropout factor)."""
    d = nhead * hd
    out = {}
    for part in PARTS:
        if part not in got or part not in ref:
            continue
        g_, r_ = got[part].detach().cpu().double(), ref[part]
        assert g_.shape == r_.shape, (part, g_.shape, r_.shape)
        w = 1 if part in ("lse", "D") else hd
        worst, where, r0 = 0.0, None, 0
        for b, L in enumerate(lens):
            for h in range(nhead):
                gb, rb = g_[r0:r0 + L, h * w:(h + 1) * w], r_[r0:r0 + L, h * w:(h + 1) * w]
                err = float((gb - rb).abs().max())
                if part in ("dQ", "dK") and (L == 1 or b in degenerate):
                    other = ref["qkv"][r0:r0 + L, (d if part == "dQ" else 0) + h * hd:(d if part == "dQ" else 0) + (h + 1) * hd]
                    den = float(ref["D"][r0:r0 + L, h].abs().max() * other.abs().max()) / hd ** 0.5 + float(rb.abs().max())
                else:
                    den = float(rb.abs().max())
                if den < FP32_TINY:             # no fp32 result can hold such a reference: the block must be exact zeros
                    ratio = 0.0 if float(gb.abs().max()) == 0.0 else math.inf
                else:
                    ratio = err / den
                if not ratio <= worst:          # (NaN counts as the worst)
                    worst, where = (ratio if ratio == ratio else math.inf), (b, h)
            r0 += L
        out[part] = (worst, where)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the float32 host model of the kernels' arithmetic
# ---------------------------------------------------------------------------------------------------------------------------------
def split32(x):
    """fp32 -> (hi, lo): the two bf16 planes, as fp32 (round to nearest even both times, as advmil_split_planes)."""
    x = x.float()
    hi = x.bfloat16().float()
    return hi, (x - hi).bfloat16().float()


def mm3(ah, al, bh, bl):
    """The kernels' product of two split operands: lo.hi + hi.lo + hi.hi, fp32 sums (lo.lo left out)."""
    return al @ bh + ah @ bl + ah @ bh


def _fma(a, b, c):
    return (a.double() * b.double() + c.double()).float()


def model(qkv, go, lens, nhead, hd, keeps=None, ik=1.0, lse_in=None, backward=True):
    """The kernels' arithmetic in float32 on the host. `keeps`: per bag bool [nhead, L, L] (None = no dropout), `ik` the kept
    probabilities' scale. `lse_in` [L_total, nhead]: the advmil_mha_fwd_lse form (probabilities exp2(s c - lse), no row sum).
    -> the same parts as `oracle` (fp32)."""
    d = nhead * hd
    c = np.float32(np.float32(1.0 / np.sqrt(np.float32(hd))) * np.float32(1.44269504088896340736))
    sc = np.float32(1.0) / np.sqrt(np.float32(hd))
    ik32 = torch.tensor(float(np.float32(ik)), dtype=torch.float32)
    c_t = torch.tensor(float(c), dtype=torch.float32)
    res = {k: [] for k in PARTS}
    r0 = 0
    for b, L in enumerate(lens):
        q, k, v = _heads(qkv[r0:r0 + L].float(), nhead, hd)
        (qh, ql), (kh, kl), (vh, vl) = split32(q), split32(k), split32(v)
        s = mm3(qh, ql, kh.transpose(-1, -2), kl.transpose(-1, -2))
        keep = None if keeps is None else keeps[b].float()
        if lse_in is None:
            m = s.max(dim=-1, keepdim=True).values
            e = torch.exp2(_fma(s, c_t, -(m * c_t)))
            l = e.sum(dim=-1, keepdim=True)
            lse = m * c_t + torch.log2(l)
            inv = ik32 / l
        else:
            lse = lse_in[r0:r0 + L].float().transpose(0, 1).unsqueeze(-1)
            e = torch.exp2(_fma(s, c_t, -lse))
            inv = ik32
        pm = e if keep is None else e * keep
        ph, pl = split32(pm)
        o = mm3(ph, pl, vh, vl) * inv
        res["O"].append(o.transpose(0, 1).reshape(L, d))
        res["lse"].append(lse.squeeze(-1).transpose(0, 1))
        if backward:
            g = go[r0:r0 + L].float().reshape(L, nhead, hd).transpose(0, 1)
            gh, gl = split32(g)
            D = (g * o).sum(-1, keepdim=True)
            pb = torch.exp2(_fma(s, c_t, -lse))
            dp = mm3(gh, gl, vh.transpose(-1, -2), vl.transpose(-1, -2))
            kf = ik32 if keep is None else keep * ik32
            ds = pb * _fma(dp, kf, -D)
            dsh, dsl = split32(ds)
            pdh, pdl = split32(pb * kf)
            dq = mm3(dsh, dsl, kh, kl) * sc
            dk = mm3(dsh.transpose(-1, -2), dsl.transpose(-1, -2), qh, ql) * sc
            dv = mm3(pdh.transpose(-1, -2), pdl.transpose(-1, -2), gh, gl)
            for name, t in (("dQ", dq), ("dK", dk), ("dV", dv)):
                res[name].append(t.transpose(0, 1).reshape(L, d))
            res["D"].append(D.squeeze(-1).transpose(0, 1))
        r0 += L
    return {k_: torch.cat(v_, dim=0) for k_, v_ in res.items() if v_}


# ---------------------------------------------------------------------------------------------------------------------------------
# the walk mirror
# ---------------------------------------------------------------------------------------------------------------------------------
BagWalk = namedtuple("BagWalk", "L key_tiles last_fill last_half q_tiles last_q_valid idle_waves trips last_trip_parity nkb nkb_groups "
                                "nkb_rem reduce_wgs reduce_idle main_wgs main_idle")
Walk = namedtuple("Walk", "bags max_len L_total prep_blocks prep_partial KS DT pad_units")


def walk_facts(lens, hd, nhead, max_len=None):
    """Which walk of the attention kernels a launch over bags `lens` takes. Per bag: key tiles T = ceil(L / 64), the fill of the last
    one and the 32-key half it ends in; query tiles ceil(L / 256), the valid queries of the last and its waves without a valid row;
    the single-pass backward's 32-query trips and the parity of the last (the wave quartets alternate per trip); key blocks nkb of the
    reduce with its groups of four and remainder; the reduce grid's workgroups ceil(max_len / 32) and how many return idle; the main
    grids' workgroups per (bag, head) ceil(max_len / 256) and how many return. Per launch: the prep kernel's blocks and whether the last
    is partial; KS / DT / pad units of the head dim."""
    assert hd in HEAD_DIMS, hd
    lens = [int(v) for v in lens]
    ml = max(lens) if max_len is None else int(max_len)
    assert ml >= max(lens)
    bags = []
    for L in lens:
        T = ceil_div(L, AT_KT)
        fill = L - (T - 1) * AT_KT
        qt = ceil_div(L, AT_QB)
        lq = L - (qt - 1) * AT_QB
        trips = ceil_div(L, B1_QT)
        nkb = ceil_div(L, AT_QB)
        rw = ceil_div(ml, REDUCE_ROWS)
        mw = ceil_div(ml, AT_QB)
        bags.append(BagWalk(L, T, fill, "first" if fill <= 32 else "second", qt, lq, 8 - ceil_div(lq, 32), trips, (trips - 1) & 1, nkb,
                            nkb // REDUCE_UNROLL, nkb % REDUCE_UNROLL, rw, rw - ceil_div(L, REDUCE_ROWS), mw, mw - qt))
    n = sum(lens) * nhead
    un = hd // 8
    return Walk(tuple(bags), ml, sum(lens), ceil_div(n, prep_pairs(hd)), n % prep_pairs(hd) != 0, hd // 16, (hd + 31) // 32,
                4 * ((hd + 31) // 32) - un)


def bwd_workspace_bytes(L_total, nhead, hd):
    """advmil_mha_bwd_workspace_bytes: D [L, nhead] fp32 | dO hi | dO lo, each part rounded up to 16 bytes."""
    r16 = lambda v: (v + 15) // 16 * 16          # noqa: E731
    return r16(4 * L_total * nhead) + 2 * r16(2 * L_total * nhead * hd)


def bwd1_workspace_bytes(L_total, nhead, hd, max_len):
    """advmil_mha_bwd1_workspace_bytes: the same, then ceil(max_len / 256) partial slabs [L, nhead * hd] fp32."""
    return bwd_workspace_bytes(L_total, nhead, hd) + ceil_div(max_len, AT_QB) * L_total * nhead * hd * 4


def walk_tags(w, hd, nhead, p=0.0, forms=("two", "one")):
    """The walks a launch reaches, as the tags tests/test_attn_walks_gpu.py::WALKS_WANTED names."""
    tags = set()
    for b in w.bags:
        tags.add(f"hd{hd}:T{min(b.key_tiles, 4)}")
        if b.last_fill in (1, 31, 32, 33, 63, 64):
            tags.add(f"hd{hd}:fill{b.last_fill}")
        if b.q_tiles == 2:
            tags.add(f"hd{hd}:q2:{'one' if b.last_q_valid == 1 else 'more'}")
        if b.L == 255:
            tags.add(f"hd{hd}:q1:255")
        if b.L == 256:
            tags.add(f"hd{hd}:q1:full")
        if b.L % AT_KT == 1 and b.L > AT_QB:
            tags.add(f"hd{hd}:keyblock2:one")
        if "one" in forms:
            if b.trips <= 3:
                tags.add(f"trips{b.trips}")
            tags.add(f"hd{hd}:parity{b.last_trip_parity}")
            if b.nkb <= 5:
                tags.add(f"hd{hd}:nkb{b.nkb}")
            if b.reduce_idle:
                tags.add("reduce_idle")
        if b.main_idle:
            tags.add("main_idle")
        if p > 0 and b.L % 4 and b.L > AT_KT:
            tags.add(f"keys%4={b.L % 4}")
    if w.prep_partial:
        tags.add(f"hd{hd}:prep_partial")
    if w.L_total % 2:
        tags.add(f"hd{hd}:Lodd")
    if nhead != 8:
        tags.add(f"hd{hd}:nhead{nhead}")
    if p > 0:
        tags.add(f"thr{drop_thr(p)}")
    return tags
