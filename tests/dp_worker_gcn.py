"""One rank of the bag-parallel test of a DEEP PatchGCN (tests/test_gcn_deep_gpu.py): tests/dp_worker.py's graph-mode run with
cfg['bcb_gcn_layers'] set -- that worker builds its cfg itself and takes no extra keys. Same bags, same shard rule, same result tree.
usage: python -m tests.dp_worker_gcn RANK WORLD PORT OUT LAYERS"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def run(layers, world, rank, dp=None, device="cuda:0"):
    from advmil_amd import ops, synth
    from advmil_amd.config import default_cfg
    from advmil_amd.model import MyHandler
    from advmil_amd.parallel import BagParallel
    from tests import dp_worker
    from tests import helpers as H
    lens, bp = dp_worker.LENS, 4
    cfg = default_cfg(bcb_mode="graph", bp_every_batch=bp, bcb_dims="1024-128-128", gen_dims="128-1", bcb_gcn_layers=layers)
    mode0 = ops.get_gemm_mode()
    h = MyHandler(cfg, device=device, parallel=dp)
    assert h.netG.backbone.num_layers == layers
    for net, prefix in ((h.netG, f"G-graph{layers}:"), (h.netD, "D-prj:")):
        sd = {k: H.T(synth.param(H.PARAM_SEED, prefix + k, tuple(v.shape))) for k, v in net.state_dict().items()}
        net.load_state_dict(sd, strict=True)
    h.rng.reset(4321)
    idxs = (dp or BagParallel()).shard_epoch(list(range(len(lens))), bp)    # bag i of a global step batch -> rank i mod W
    try:
        cl = h._train_each_epoch(dp_worker.build_loader("graph", idxs, lens), "train", "wlabel")
    finally:
        ops.set_gemm_mode(mode0)
    return {"cl": cl, "logs": h.pop_logs(), "G": {k: v.detach().cpu() for k, v in h.netG.state_dict().items()},
            "D": {k: v.detach().cpu() for k, v in h.netD.state_dict().items()}}


def main():
    rank, world, port, out, layers = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4], int(sys.argv[5])
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=port, RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0",
                      HSA_ENABLE_IPC_MODE_LEGACY="0")
    from advmil_amd import parallel
    parallel.init_from_env(backend="gloo")               # two ranks on ONE GPU: RCCL refuses that, the exchange layer is backend agnostic
    res = run(layers, world, rank, parallel.BagParallel())
    if rank == 0:
        torch.save(res, out)
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
