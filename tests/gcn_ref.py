"""TEST INFRASTRUCTURE ONLY: float64 restatement of PatchGCN at full depth (reference model/backbone.py:148-168), in torch double with
autograd, built on the oracle's own pieces (genconv, _lin, _drop, attn_net_gated).

PARITY UNPINNED, as oracle.advmil_oracle.patch_gcn is: the block wrapper is torch_geometric's DeepGCNLayer(block='res'), absent and
unversioned. Restated from its published semantics: conv -> norm -> act -> x + h -> dropout; layer 0 runs its conv only.

Masks are multiplicative (keep / (1 - p), or None): `fc`, `phi`, `att_a`, `att_b` as in the oracle, `res1 .. res{L-1}` for the blocks."""
import torch
import torch.nn.functional as F

from oracle import advmil_oracle as O


def layer_norm(h, gamma, beta, eps=1e-5):
    return F.layer_norm(h, (h.shape[-1],), gamma, beta, eps)


def res_block(h, x, gamma, beta, keep_scale=None, eps=1e-5):
    """Dropout(x + relu(LayerNorm(h))): h = the layer's GENConv output, x = the previous layer's output."""
    y = x + torch.relu(layer_norm(h, gamma, beta, eps))
    return y if keep_scale is None else y * keep_scale


def patch_gcn_deep(P, x, edge_index, L, masks=None):
    """x[N, dim_in], edge_index[2, E] (the edge set in use) -> (H[1, dim_out], A[1, N])."""
    xs = [O._drop(torch.relu(O._lin(P, "fc.0", x)), masks, "fc")]
    xs.append(O.genconv(O._sub(P, "layers.0.conv."), xs[0], edge_index))
    for l in range(1, L):
        h = O.genconv(O._sub(P, f"layers.{l}.conv."), xs[-1], edge_index)
        keep = None if masks is None else masks.get(f"res{l}")
        xs.append(res_block(h, xs[-1], P[f"layers.{l}.norm.weight"], P[f"layers.{l}.norm.bias"], keep))
    h = torch.cat(xs, dim=1)
    h = O._drop(torch.relu(O._lin(P, "path_phi.0", h)), masks, "phi")
    s = O.attn_net_gated(O._sub(P, "path_attention_head."), h, masks)
    A = torch.softmax(s.t(), dim=1)
    return A @ h, A


def generator_deep(P, x, edge_index, L, noise, masks=None, out_scale="sigmoid", noise_flags=(0, 1)):
    """The oracle's generator with the deep backbone under `backbone.`."""
    H, _ = patch_gcn_deep(O._sub(P, "backbone."), x, edge_index, L, masks)
    return O.generator_head(P, H, list(noise_flags), noise, masks, out_scale)
