"""CPU: PatchGCN at full depth -- what can be checked without a device.
 * tests/gcn_ref.py::patch_gcn_deep at L = 1 is the committed oracle's patch_gcn (pins the new restatement to the old one);
 * state_dict keys and shapes of PatchGCN(num_layers = 3) are the reference's;
 * the argument errors of PatchGCN, load_backbone and the two handlers come before any device is needed;
 * advmil_gcn_res_fwd / _bwd exist in the header, the ctypes table and the library, the workspace query is a pure host function and
   every refusal of the header's contract answers ADVMIL_EINVAL without a launch."""
import ctypes

import pytest
import torch

from advmil_amd import synth
from advmil_amd.config import default_baseline_cfg, default_cfg
from oracle import advmil_oracle as O
from tests import gcn_ref as R
from tests import helpers as H
from tests.test_abi_cpu import header_symbols

EINVAL, EWORKSPACE = -1, -2
A16 = 0x7F0000001000          # a fake 16-byte aligned "device address": never dereferenced when validation does its job
NEW = ("advmil_gcn_res_fwd", "advmil_gcn_res_bwd_workspace_bytes", "advmil_gcn_res_bwd")
DIMS = [1024, 128, 128]


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from advmil_amd import _lib
    return _lib


def synth_params(module, prefix):
    return {k: torch.as_tensor(synth.param(H.PARAM_SEED, prefix + k, tuple(v.shape))).double() for k, v in module.state_dict().items()}


def test_restatement_at_depth_one_is_the_oracle():
    from advmil_amd.model.backbone import PatchGCN
    N = 37
    P = synth_params(PatchGCN(DIMS, num_layers=1), "gcn-deep:")
    x = torch.as_tensor(synth.bag(3, 0, 64))[0, :N].double()
    ei = torch.as_tensor(synth.grid_knn_graph(N, 8))
    g = torch.Generator().manual_seed(5)
    masks = {k: (torch.rand(N, 128, generator=g) >= 0.25).double() / 0.75 for k in ("fc", "phi", "att_a", "att_b")}
    for m in (None, masks):
        want, wantA = O.patch_gcn(P, x, ei, m)
        got, gotA = R.patch_gcn_deep(P, x, ei, 1, m)
        assert float((got - want).abs().max()) <= 1e-12 and float((gotA - wantA).abs().max()) <= 1e-12


def test_state_dict_of_three_layers_is_the_references():
    from advmil_amd.model.backbone import PatchGCN
    sd = {k: tuple(v.shape) for k, v in PatchGCN(DIMS, num_layers=3).state_dict().items()}
    want = {"fc.0.weight": (128, 1024), "fc.0.bias": (128,), "path_phi.0.weight": (128, 512), "path_phi.0.bias": (128,)}
    for l in range(3):
        p = f"layers.{l}."
        want.update({p + "conv.t": (1,), p + "conv.mlp.0.weight": (256, 128), p + "conv.mlp.0.bias": (256,), p + "conv.mlp.1.weight": (256,),
                     p + "conv.mlp.1.bias": (256,), p + "conv.mlp.4.weight": (128, 256), p + "conv.mlp.4.bias": (128,),
                     p + "norm.weight": (128,), p + "norm.bias": (128,)})
    for br in ("attention_a.0", "attention_b.0"):
        want.update({f"path_attention_head.{br}.weight": (128, 128), f"path_attention_head.{br}.bias": (128,)})
    want.update({"path_attention_head.attention_c.weight": (1, 128), "path_attention_head.attention_c.bias": (1,)})
    assert sd == want


def test_argument_errors_come_before_any_device():
    from advmil_amd.model import BaselineHandler, MyHandler, load_backbone
    from advmil_amd.model.backbone import PatchGCN
    with pytest.raises(ValueError, match="num_layers = 0"):
        PatchGCN(DIMS, num_layers=0)
    with pytest.raises(ValueError, match="edge_agg = 'x'"):
        PatchGCN(DIMS, edge_agg="x")
    with pytest.raises(TypeError, match="num_layers"):
        load_backbone("abmil", DIMS, num_layers=2)
    with pytest.raises(TypeError, match="dropout"):
        load_backbone("graph", DIMS, dropout=0.5)
    assert load_backbone("graph", DIMS).num_layers == 1 and load_backbone("graph", DIMS).edge_agg == "spatial"
    deep = load_backbone("graph", DIMS, num_layers=2, edge_agg="latent")
    assert (deep.num_layers, deep.edge_agg, len(deep.layers)) == (2, "latent", 2)
    with pytest.raises(ValueError, match="bcb_gcn_layers"):
        MyHandler(default_cfg(bcb_mode="patch", bcb_gcn_layers=2))
    with pytest.raises(ValueError, match="bcb_gcn_edge_agg"):
        BaselineHandler(default_baseline_cfg(bcb_mode="abmil", bcb_gcn_edge_agg="latent"))
    assert "bcb_gcn_layers" not in default_cfg() and "bcb_gcn_edge_agg" not in default_cfg()      # absent = shipped


def test_site_layout_is_registered():
    from advmil_amd import ops
    assert ops.site_layouts("gcn_res1") == ("patch",) and ops.site_layouts("gcn_res2") == ("patch",)


def test_symbols_in_header_table_and_library(L):
    handle = ctypes.CDLL(L.LIB_PATH)
    for name in NEW:
        assert name in header_symbols() and name in L.SIGNATURES and hasattr(handle, name), name


def test_workspace_query_is_a_pure_host_function(L):
    lib = L.lib()
    # one row of dgamma | dbeta partials per workgroup; a workgroup per 16 rows, at most 2048 of them
    assert lib.advmil_gcn_res_bwd_workspace_bytes(1, 4) == 2 * 4 * 4
    assert lib.advmil_gcn_res_bwd_workspace_bytes(500, 128) == 32 * 2 * 128 * 4
    assert lib.advmil_gcn_res_bwd_workspace_bytes(65536, 384) == 2048 * 2 * 384 * 4
    assert lib.advmil_gcn_res_bwd_workspace_bytes(0, 128) == 0


def _p(k, off=0):
    return ctypes.c_void_p(A16 + (k << 20) + off)


def fwd_args(N=64, d=128, ldx=None, ldo=None, p=0.0, seed=None, rng_row=None, h=None, x=None):
    ldx, ldo = d if ldx is None else ldx, d if ldo is None else ldo
    return (h or _p(0), x or _p(1), ldx, _p(2), _p(3), 1e-5, N, d, p, seed, 7, rng_row, _p(4), ldo, _p(5), _p(6), None)


def bwd_args(N=64, d=128, lddo=None, lddx=None, p=0.0, seed=None, dx=None, ws=_p(12), ws_bytes=1 << 20):
    lddo, lddx = d if lddo is None else lddo, d if lddx is None else lddx
    return (_p(0), lddo, _p(1), _p(2), _p(3), _p(5), _p(6), N, d, p, seed, 7, None, _p(7), dx or _p(8), lddx, 0, _p(9), _p(10), 0,
            ws, ws_bytes, None)


REFUSED = [("d6", dict(d=6)), ("d516", dict(d=516)), ("d0", dict(d=0)), ("N0", dict(N=0)), ("p1", dict(p=1.0, seed=_p(11))),
           ("p-neg", dict(p=-0.1, seed=_p(11))), ("p-without-seed", dict(p=0.1))]


@pytest.mark.parametrize("kw", [k for _, k in REFUSED], ids=[n for n, _ in REFUSED])
def test_both_entry_points_refuse(L, kw):
    lib = L.lib()
    assert lib.advmil_gcn_res_fwd(*fwd_args(**kw)) == EINVAL
    assert lib.advmil_gcn_res_bwd(*bwd_args(**kw)) == EINVAL


def test_pitch_alignment_and_workspace_checks(L):
    lib = L.lib()
    assert lib.advmil_gcn_res_fwd(*fwd_args(ldo=124)) == EINVAL                   # pitch shorter than the row
    assert lib.advmil_gcn_res_fwd(*fwd_args(ldx=124)) == EINVAL
    assert lib.advmil_gcn_res_fwd(*fwd_args(ldx=130)) == EINVAL                   # rows of the block off 16 bytes
    assert lib.advmil_gcn_res_fwd(*fwd_args(ldo=130)) == EINVAL
    assert lib.advmil_gcn_res_fwd(*fwd_args(h=_p(0, 4))) == EINVAL                # a misaligned pointer
    assert lib.advmil_gcn_res_fwd(*fwd_args(x=_p(1, 8))) == EINVAL
    assert lib.advmil_gcn_res_fwd(*fwd_args(p=0.1, seed=_p(11), rng_row=_p(13, 8))) == EINVAL
    assert lib.advmil_gcn_res_bwd(*bwd_args(lddo=124)) == EINVAL
    assert lib.advmil_gcn_res_bwd(*bwd_args(lddx=130)) == EINVAL
    assert lib.advmil_gcn_res_bwd(*bwd_args(dx=_p(8, 4))) == EINVAL
    assert lib.advmil_gcn_res_bwd(*bwd_args(ws=None)) == EINVAL
    need = lib.advmil_gcn_res_bwd_workspace_bytes(64, 128)
    assert lib.advmil_gcn_res_bwd(*bwd_args(ws_bytes=need - 4)) == EWORKSPACE
