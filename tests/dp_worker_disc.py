"""One rank of the bag-parallel test of the discrete-time task (tests/test_disc_parallel_gpu.py): MyHandler with task = disc_gansurv
(time_bins = 4) on cuda:0 with the shipped dropout ON, this rank's shard of the global step batches (bag i on rank i mod W), two optimizer
steps through _train_each_epoch; rank 0 saves what the single-process run is compared with. The protocol of tests/dp_worker.py.
usage: python -m tests.dp_worker_disc RANK WORLD PORT OUT KIND"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

BINS = 4
LENS = (256, 128, 64, 192, 320, 96, 160, 224)       # 2 steps x 4 bags (global), ragged, multiples of 16
# `bp8`: 2 steps x 8 bags, for W = 4 (2 bags per rank and step)
LENS_BP8 = (256, 128, 64, 192, 320, 96, 160, 224, 48, 272, 112, 208, 80, 304, 144, 176)
# `wolabel` (mode 'wolabel'): the bags whose label is NOT visible. Step 1 holds bags 0..3: at W = 2 rank 1 (bags 1, 3) has no visible label
# while rank 0 (bags 0, 2) has two; step 2 (bags 4..7) mixes them on both ranks
INVISIBLE = (1, 3, 6)


def bin_label(i):
    from advmil_amd import synth
    from tests import helpers as H
    y = synth.label(H.DATA_SEED, i).copy()
    y[0, 0] = np.floor(BINS * y[0, 0])
    return H.T(y)


def build_loader(idxs, lens):
    from tests import helpers as H
    return [(torch.tensor([[i]], dtype=torch.int), [H.bag(300 + i, 512)[:, :lens[i]].contiguous(), torch.zeros(1, 1)], bin_label(300 + i))
            for i in idxs]


def run(kind, world, rank, dp=None, device="cuda:0"):
    from advmil_amd import ops, synth
    from advmil_amd.config import default_cfg
    from advmil_amd.model import MyHandler
    from advmil_amd.parallel import BagParallel
    from tests import helpers as H
    lens, bp, mode = LENS, 4, "wlabel"
    if kind.endswith("-bp8"):
        kind, lens, bp = kind[:-len("-bp8")], LENS_BP8, 8
    elif kind.endswith("-wolabel"):
        kind, mode = kind[:-len("-wolabel")], "wolabel"
    cfg = default_cfg(task="disc_gansurv", time_format="quantile", time_bins=BINS, gen_dims=f"384-{BINS}", disc_nety_in_dim=BINS,
                      bcb_mode=kind, bp_every_batch=bp)         # the GLOBAL step batch: every rank steps after bp / world of its bags
    mode0 = ops.get_gemm_mode()
    h = MyHandler(cfg, device=device, parallel=dp)
    for net, prefix in ((h.netG, f"G-{kind}:"), (h.netD, "D-prj:")):
        sd = {k: H.T(synth.param(H.PARAM_SEED, prefix + k, tuple(v.shape))) for k, v in net.state_dict().items()}
        net.load_state_dict(sd, strict=True)
    h.rng.reset(4321)
    h.patient_id["train"] = [str(i) for i in range(len(lens))]
    if mode == "wolabel":
        h.patient_id["label_visible"] = [str(i) for i in range(len(lens)) if i not in INVISIBLE]
    idxs = (dp or BagParallel()).shard_epoch(list(range(len(lens))), bp)    # bag i of a global step batch -> rank i mod W
    heads, real = [], ops.ghead
    ops.ghead = lambda *a, **k: (heads.append(int(a[1].W1.shape[0])), real(*a, **k))[1]      # (the fused width-K head ran on this rank)
    try:
        cl = h._train_each_epoch(build_loader(idxs, lens), "train", mode)
    finally:
        ops.ghead = real
        ops.set_gemm_mode(mode0)
    logs = h.pop_logs()
    return {"cl": cl, "logs": logs, "heads": heads, "graphs": dict(h.step_graph_stats),
            "G": {k: v.detach().cpu() for k, v in h.netG.state_dict().items()}, "D": {k: v.detach().cpu() for k, v in h.netD.state_dict().items()}}


def main():
    rank, world, port, out, kind = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4], sys.argv[5]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=port, RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0",
                      HSA_ENABLE_IPC_MODE_LEGACY="0")
    from advmil_amd import parallel
    parallel.init_from_env(backend="gloo")           # the ranks share ONE GPU: RCCL refuses that, the exchange layer is backend agnostic
    res = run(kind, world, rank, parallel.BagParallel(), device="cuda:0")
    if rank == 0:
        torch.save(res, out)
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
