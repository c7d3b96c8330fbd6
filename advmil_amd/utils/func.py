"""The five helpers of the reference's utils/func.py that sit on the G+D step path
(SURVEY.md §2 #12): generate_noise (154-164), collect_tensor (112-125), agg_tensor (127-133),
sparse_key / sparse_str (135-152), seed_everything (166-175), and the occlusion test's random_mask_square_instance (14-40).
Same names and argument meaning."""
import random

import numpy as np
import torch

from .. import ops


def generate_noise(*dims, to_device="cuda", distribution="uniform", rng=None):
    """[dims] noise drawn ON the device by the counter RNG (the reference samples on the CPU and copies:
    utils/func.py:154-164). uniform -> U[0,1); gaussian -> N(0,1) by Box-Muller on two uniform draws."""
    assert distribution in ["uniform", "gaussian"]
    rng = rng or ops.default_rng(to_device)
    n = int(np.prod(dims))
    w = int(dims[-1])
    if distribution == "uniform":
        return rng.uniform(n, "noise", width=w).reshape(*dims)
    u1 = rng.uniform(n, "noise_u1", width=w).clamp_min(2.0 ** -24)
    u2 = rng.uniform(n, "noise_u2", width=w)
    return (torch.sqrt(-2.0 * torch.log(u1)) * torch.cos(2.0 * np.pi * u2)).reshape(*dims)


def collect_tensor(collector, real, fake):
    for key, val in (("real", real), ("fake", fake)):
        if val is not None:
            collector[key] = val if collector[key] is None else torch.cat([collector[key], val], dim=0)
    return collector


def agg_tensor(collector, data):
    for k, v in data.items():
        prev = collector.get(k)
        collector[k] = v if prev is None else torch.cat([prev, v], dim=0)
    return collector


def sparse_key(d, prefixes: str = ""):
    """cfg keys starting with `prefixes` + '_' -> dict without the prefix (func.py:135-146)."""
    if prefixes == "":
        return d
    out = {}
    for k, v in d.items():
        if k.startswith(prefixes):
            rest = k.split(prefixes)[1]
            if len(rest) >= 2:
                out[rest[1:]] = v
    return out


def sparse_str(s, sep="-", dtype=int):
    return [s] if not isinstance(s, str) else [dtype(tok) for tok in s.split(sep)]


def seed_everything(seed):
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)
        ops.default_rng(torch.device("cuda", torch.cuda.current_device())).reset(seed)


def dropout_small(x, p, training, rng, tag=""):
    """Dropout for the [1,d]-sized head tensors, drawn from the same counter RNG as the kernels
    (so a parity test can regenerate the mask: advmil_amd.synth.dropout_keep)."""
    if not training or p <= 0.0:
        return x
    return ops.dropout(x, p, rng, tag)


def square_instance_keep(n_rows, mask_ratio, scale=4, rng=None):
    """The draw of the reference's random_mask_square_instance (utils/func.py:14-31) on its own: the sorted int64 indices of the
    `scale` x `scale` square instances (regions of scale^2 consecutive patches) a bag of `n_rows` patches KEEPS, or None where the
    reference hands the bag back unchanged (mask_ratio <= 0 or > 1; no random number is consumed then). The reference's arithmetic to
    the letter -- n_keep = max(1, int(N_scaled * (1 - mask_ratio))), the ratio is not rounded: 10 regions at 0.8 keep ONE, because
    10 * (1 - 0.8) is 1.9999999999999996 -- and one `permutation(N_scaled)` per bag, from `rng` (an np.random.RandomState) or from
    the global np.random as the reference draws it: same seed, same bag order -> the reference's own kept sets."""
    if mask_ratio <= 0 or mask_ratio > 1:
        return None
    n_square = scale * scale
    assert n_rows % n_square == 0, 'bag must consist of square instances.'
    n_scaled = n_rows // n_square
    n_keep = max(1, int(n_scaled * (1 - mask_ratio)))
    idxs = (np.random if rng is None else rng).permutation(n_scaled)
    return np.sort(idxs[:n_keep]).astype(np.int64)


def keep_rows_index(keep, scale=4):
    """Kept region indices -> the row indices of their patches, ascending (int64 numpy)."""
    n_square = scale * scale
    return (np.asarray(keep, dtype=np.int64).reshape(-1, 1) * n_square + np.arange(n_square, dtype=np.int64).reshape(1, -1)).reshape(-1)


def mask_square_rows(bag, keep, scale=4, mask_way='mask_zero'):
    """bag[N, C] (host or device) under a kept-region set of square_instance_keep: 'mask_zero' -> a new bag whose masked rows are
    zero, 'discard' -> the kept rows only. keep None -> the bag itself."""
    if mask_way not in ('discard', 'mask_zero'):
        raise NotImplementedError("Cannot run with mask_way={}.".format(mask_way))
    if keep is None:
        return bag
    rows = torch.from_numpy(keep_rows_index(keep, scale)).to(bag.device)
    if mask_way == 'discard':
        return bag[rows]
    new_bag = torch.zeros_like(bag)
    new_bag[rows] = bag[rows]
    return new_bag


def random_mask_square_instance(bag, mask_ratio, scale=4, mask_way='mask_zero'):
    """Reference utils/func.py:14-40, same signature: zero ('mask_zero') or drop ('discard') a random share of the bag's square
    instances. bag[N, C] on the host or on the device; plain indexing over square_instance_keep (the evaluation's staged path
    applies the same kept set inside the staging launch instead: include/advmil_hip.h::advmil_stage_bag_masked)."""
    if mask_ratio <= 0 or mask_ratio > 1:
        return bag
    keep = square_instance_keep(bag.shape[0], mask_ratio, scale)
    return mask_square_rows(bag, keep, scale, mask_way)


def square_mask_fn(backbone, mask_ratio, rng=None):
    """The per-bag draw of an evaluation under `mask_ratio` (both handlers' test_model): n_rows -> square_instance_keep, or None when
    nothing is to be masked -- a ratio the reference ignores (None, <= 0, > 1: no draw at all), or bags that are no patch grids: the
    reference's dataset masks 'patch'-style bags only (dataset/PatchWSI.py:80-81; cluster and graph bags, 85-107, never), which is
    said once per call."""
    if mask_ratio is None or mask_ratio <= 0 or mask_ratio > 1:
        return None
    if backbone not in ("abmil", "patch"):
        import warnings
        warnings.warn(f"mask_ratio={mask_ratio} is ignored for backbone {backbone!r}: only patch-style bags (abmil, patch) consist of "
                      "square instances; the bags are evaluated unmasked")
        return None
    return lambda n_rows: square_instance_keep(n_rows, mask_ratio, rng=rng)


def keep_bitmap(keep, n_regions):
    """Kept region indices -> the uint32 words advmil_stage_bag_masked reads: bit r & 31 of word r >> 5 = region r is kept."""
    bits = np.zeros((n_regions + 31) // 32 * 32, dtype=np.uint8)
    bits[np.asarray(keep, dtype=np.int64)] = 1
    return np.packbits(bits, bitorder="little").view(np.uint32)
