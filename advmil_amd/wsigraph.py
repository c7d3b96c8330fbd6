"""WSI patch graphs built on the device: the graph `ext` of `bcb_mode: graph` from patch features and patch coordinates.

The reference gets these graphs from tools/patchgcn_graph_s2.py (nmslib HNSW, approximate; as shipped its latent search queries the
feature index with 2-d coordinates, line 85, so the documented latent edge set cannot be built with it). Here both edge sets are EXACT
k-nearest-neighbour searches with a stated tie rule -- ascending (squared distance, neighbour id), self excluded by index --, one launch
each (ops.knn_spatial: integer coordinates, int64 distances; ops.knn_latent: features, bf16x3 contraction with a selection epilogue),
pinned to a float64 / int64 oracle (tests/knn_ref.py). `radius=9` upstream asks the index for 9 neighbours and drops the first (the
node itself): k = 8.

    g = build_graph(feats, coords)                    # SimpleNamespace(x, edge_index, edge_latent, centroid)
    H = PatchGCN(...)(g)                              # or as the `ext` of a MyHandler / baseline loader sample
    gs = build_graphs(feats_list, coords_list)        # all slides of a patient with one launch per edge set
    g = merge_graphs(gs)                              # patient-level graph, as the reference's dataset concatenates them
"""
from types import SimpleNamespace

import torch

from . import ops


def edges_from_neighbours(nbr):
    """nbr[N, k] (neighbour ids) -> edge_index[2, k*N] int64: row 0 = arange(N).repeat_interleave(k), row 1 = nbr.reshape(-1), the
    layout of tools/patchgcn_graph_s2.py:78-80 that ops.GraphCSR documents."""
    N, k = nbr.shape
    src = torch.arange(N, dtype=torch.int64, device=nbr.device).repeat_interleave(k)
    return torch.stack([src, nbr.reshape(-1).to(torch.int64)])


def _graph(x, coords, nbr_s, nbr_l):
    return SimpleNamespace(x=x, edge_index=edges_from_neighbours(nbr_s),
                           edge_latent=None if nbr_l is None else edges_from_neighbours(nbr_l), centroid=coords)


def build_graph(feats, coords, k=8, latent=True):
    """One slide: feats [N, C] fp32 and coords [N, 2] (int32 / int64 / integer-valued float) on the device, N > k. `edge_latent` is
    None with latent=False."""
    return _graph(feats, coords, ops.knn_spatial(coords, k), ops.knn_latent(feats, k) if latent else None)


def build_graphs(feats_list, coords_list, k=8, latent=True):
    """Several slides at once: the slides' rows form one slab, ONE spatial and ONE latent launch search every slide within its own rows
    (ops.Segments). Returns one graph per slide, bit-identical to build_graph of that slide."""
    if len(feats_list) != len(coords_list) or not feats_list:
        raise ValueError("advmil_amd: build_graphs: one coordinate tensor per feature tensor, at least one slide")
    lens = [int(f.shape[0]) for f in feats_list]
    for b, (n, c) in enumerate(zip(lens, coords_list)):
        if int(c.shape[0]) != n:
            raise ValueError(f"advmil_amd: build_graphs: slide {b} has {n} feature rows and {int(c.shape[0])} coordinates")
    X = torch.cat(list(feats_list), dim=0)
    xy = torch.cat([c.to(coords_list[0].dtype) for c in coords_list], dim=0)
    seg = ops.Segments(lens, X.device)
    nbr_s = ops.knn_spatial(xy, k, seg)
    nbr_l = ops.knn_latent(X, k, seg) if latent else None
    out = []
    for b, f in enumerate(feats_list):
        r0, r1 = seg.offsets[b], seg.offsets[b + 1]
        out.append(_graph(f, coords_list[b], nbr_s[r0:r1], None if nbr_l is None else nbr_l[r0:r1]))
    return out


def merge_graphs(graphs):
    """Patient-level concatenation of slide graphs, what the reference's dataset does with
    GraphBatch.from_data_list(..., update_cat_dims={'edge_latent': 1}) (dataset/PatchWSI.py:96-107): x and centroid along dim 0, both
    edge sets along dim 1 with the slides' node offsets added. Pure torch; works on CPU tensors."""
    graphs = list(graphs)
    if not graphs:
        raise ValueError("advmil_amd: merge_graphs: no graph")
    offs, n = [], 0
    for g in graphs:
        offs.append(n)
        n += int(g.x.shape[0])
    has_latent = [getattr(g, "edge_latent", None) is not None for g in graphs]
    if any(has_latent) and not all(has_latent):
        raise ValueError("advmil_amd: merge_graphs: some graphs carry edge_latent and some do not")
    cat_edges = lambda name: torch.cat([getattr(g, name).to(torch.int64) + o for g, o in zip(graphs, offs)], dim=1)   # noqa: E731
    cents = [getattr(g, "centroid", None) for g in graphs]
    return SimpleNamespace(x=torch.cat([g.x for g in graphs], dim=0), edge_index=cat_edges("edge_index"),
                           edge_latent=cat_edges("edge_latent") if all(has_latent) else None,
                           centroid=None if any(c is None for c in cents) else torch.cat(cents, dim=0))
