#!/usr/bin/env python3
"""Golden vectors of the gated-attention region embedding (disc_netx_backbone: gapool) from the REAL reference, run on the CPU through
the import shims of gen_golden.py, and the pin of the float64 restatement (tests/gapool_ref.py) against the reference module in the
same run.

Runs only in the build container (the reference never travels). Inputs and weights are regenerated from the repo's counter RNG
(advmil_amd/synth.py), so the fixtures hold only outputs: tests/golden/gapool_v1.npz and tests/golden/ORACLE_PIN_gapool.json.
Usage:  python tests/golden/gen_golden_gapool.py

  (a) L_d{128,384}_*: the reference GAPoolPatchEmbedding alone in float64, C = 1024, N = 48: emb, A and the gradient of sum(emb * w)
      with respect to every parameter (matrices above 4096 entries as digests, gapool_ref.grad_digest; the
      pin below compares them whole).
  (b) Dg_{name}_N{64,512}_f: PrjDiscriminator (instance / x, bag / x) and Discriminator (cat) in eval mode with the gapool embedding.
  (c) S_{abmil,patch}_*: two passes of MyHandler._train_each_epoch (each one _update_disc and one _update_gen) over the same 4 bags of
      32, 64, 16 and 48 patches with events 1, 0, 1, 1; disc_netx_backbone: gapool, bp_every_batch 4, every dropout p = 0, injected noise.
"""
import importlib.util
import json
import os
import sys
import tempfile

import numpy as np
import torch
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)

_spec = importlib.util.spec_from_file_location("gen_golden", os.path.join(HERE, "gen_golden.py"))
GG = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(GG)

from advmil_amd import synth  # noqa: E402
from tests import gapool_ref as R  # noqa: E402

T, REF, DATA_SEED, PARAM_SEED, LOG = GG.T, GG.REF, GG.DATA_SEED, GG.PARAM_SEED, GG.LOG
LAYER_PREFIX = "net_pair_one.embedding."
LAYER_N, LAYER_C, LAYER_BAG = 48, 1024, 5
STEP_LENS, STEP_EVENTS = (32, 64, 16, 48), (1.0, 0.0, 1.0, 1.0)
LOG_KEYS_D, LOG_KEYS_G = ("Loss_D", "D_real", "D_fake"), ("Loss_G_fake", "Loss_G_time", "Loss_G_total", "D_fake_avg")


def layer_weight(d):
    """The fixed w of (a): the gradients are those of sum(emb * w)."""
    return synth.normal(synth.stream_key(1, f"gapool_w:{d}"), (LAYER_N // 16) * d).reshape(LAYER_N // 16, d)


def step_label(i):
    y = synth.label(DATA_SEED, i).copy()
    y[0, 1] = STEP_EVENTS[i]
    return T(y)


def gen_a(out, pin):
    from model.backbone_utils import GAPoolPatchEmbedding
    for d in (128, 384):
        m = GAPoolPatchEmbedding(LAYER_C, d, 4, False, 1).double()
        sd = m.state_dict()
        assert {k: tuple(v.shape) for k, v in sd.items()} == R.shapes(LAYER_C, d), {k: tuple(v.shape) for k, v in sd.items()}
        P = {k: synth.param(PARAM_SEED, LAYER_PREFIX + k, tuple(v.shape)) for k, v in sd.items()}
        m.load_state_dict({k: T(v).double() for k, v in P.items()})
        x = synth.bag(DATA_SEED, LAYER_BAG, LAYER_N, LAYER_C)
        w = layer_weight(d)
        cap = {}
        hk = m.pool.fc2.register_forward_hook(lambda mod, i, o: cap.__setitem__("s", o.detach()))
        emb = m(T(x).double())
        hk.remove()
        assert tuple(emb.shape) == (1, LAYER_N // 16, d)
        (emb[0] * T(w).double()).sum().backward()
        A = torch.softmax(cap["s"].reshape(-1, 16), dim=1).reshape(-1)
        out[f"L_d{d}_emb"], out[f"L_d{d}_A"] = emb[0].detach().numpy(), A.numpy()
        grads = {k: p.grad.numpy() for k, p in m.named_parameters()}
        for k, g in grads.items():                # (the large matrices as digests: tests/gapool_ref.py::grad_digest)
            for suf, v in R.grad_digest(k, g).items():
                out[f"L_d{d}_grad_{k}_{suf}"] = v
        f = R.layer_fwd(P, x[0])
        G = R.layer_bwd(P, f, w)
        pin[f"a/d{d}"] = {"emb": float(np.abs(f["emb"] - out[f"L_d{d}_emb"]).max()), "A": float(np.abs(f["A"] - out[f"L_d{d}_A"]).max()),
                          "grad": max(float(np.abs(G[k] - grads[k]).max()) for k in grads)}
    out["L_keys"] = np.array(sorted(R.shapes(LAYER_C, 128)))


def build_disc(disc_type, iprd, prj):
    from types import SimpleNamespace
    from model.GANSurv import Discriminator, PrjDiscriminator
    ax = SimpleNamespace(in_dim=1024, out_dim=128, ksize=1, backbone="gapool", dropout=0.25)
    ay = SimpleNamespace(in_dim=1, hid_dims=[64, 128], norm=False, dropout=0.0)
    return PrjDiscriminator(ax, ay, prj_path=prj, inner_product=iprd) if disc_type == "prj" else Discriminator(ax, ay)


def gen_b(out):
    t = torch.tensor([[0.37]])
    for disc_type, iprd, prj in (("prj", "instance", "x"), ("prj", "bag", "x"), ("cat", "bag", None)):
        d = build_disc(disc_type, iprd, prj).eval()
        GG.load_synth(d, prefix="D-prj:" if disc_type == "prj" else "D-cat:")
        out[f"Dg_{disc_type}-{iprd}-{prj}_keys"] = np.array(sorted(d.state_dict()))
        for N in (64, 512):
            with torch.no_grad():
                f = d(T(synth.bag(DATA_SEED, 3, N)), t)
            out[f"Dg_{disc_type}-{iprd}-{prj}_N{N}_f"] = f.numpy()


def gen_c(out, tmp):
    import utils.func
    import model.GANSurv as GS
    from model.model_handler import MyHandler
    cfg0 = yaml.load(open(os.path.join(REF, "config/cfg_nlst.yaml")), Loader=yaml.FullLoader)
    nq = GG.NoiseQueue()
    old = (utils.func.generate_noise, GS.generate_noise)
    utils.func.generate_noise = nq
    GS.generate_noise = nq
    try:
        for kind in ("abmil", "patch"):
            cfg = dict(cfg0)
            cfg.update(bcb_mode=kind, data_split_seed=0, save_path=os.path.join(tmp, f"save_{kind}"), wandb_dir=tmp, num_workers=0,
                       bp_every_batch=4, disc_netx_backbone="gapool")
            h = MyHandler(cfg)
            assert type(h.netD.net_pair_one.embedding).__name__ == "GAPoolPatchEmbedding"
            PG = GG.load_synth(h.netG, prefix=f"G-{kind}:")
            PD = GG.load_synth(h.netD, prefix="D-prj:")
            GG.zero_dropout(h.netG); GG.zero_dropout(h.netD)
            nb = len(STEP_LENS)
            h.patient_id["label_visible"] = h.patient_id["train"] = [str(i) for i in range(nb)]
            loader = [(torch.tensor([[i]], dtype=torch.int), [T(synth.bag(DATA_SEED, i, STEP_LENS[i])), torch.zeros(1, 1)], step_label(i))
                      for i in range(nb)]
            name = f"S_{kind}"
            LOG.clear()
            ys, fs = [], []
            for ep in range(2):
                nq.q.extend(GG.noise_tensor(f"GP{ep}d:{kind}", i, 192) for i in range(nb))
                nq.q.extend(GG.noise_tensor(f"GP{ep}g:{kind}", i, 192) for i in range(nb))
                cl = h._train_each_epoch(loader, "train")
                assert not nq.q
                ys.append(cl["y_hat"].numpy()); fs.append(cl["f_fake"].numpy())
            logs = [{k.split("/")[-1]: v for k, v in d.items()} for d in LOG]
            assert len(logs) == 4
            out[f"{name}_logs"] = np.array([[logs[2 * s][k] for k in LOG_KEYS_D] + [logs[2 * s + 1][k] for k in LOG_KEYS_G] for s in range(2)],
                                           dtype=np.float64)
            out[f"{name}_y_hat"], out[f"{name}_f_fake"], out[f"{name}_y"] = np.stack(ys), np.stack(fs), cl["y"].numpy()
            refG = {k: v.detach() for k, v in h.netG.state_dict().items()}
            refD = {k: v.detach() for k, v in h.netD.state_dict().items()}
            keysG, keysD = sorted(refG), sorted(refD)
            out[f"{name}_keysG"], out[f"{name}_keysD"] = np.array(keysG), np.array(keysD)
            st = GG.tensor_stats
            out[f"{name}_postG_stats"] = np.array([st(refG)[k] for k in keysG])
            out[f"{name}_postD_stats"] = np.array([st(refD)[k] for k in keysD])
            for t_, ref, P0, keys in (("G", refG, PG, keysG), ("D", refD, PD, keysD)):
                out[f"{name}_d{t_}_stats"] = np.array([[float((ref[k].double() - P0[k].double()).sum()),
                                                        float((ref[k].double() - P0[k].double()).norm())] for k in keys])
            gk = [k for k, _ in h.netG.named_parameters()]
            out[f"{name}_gradG2_keys"] = np.array(gk)
            out[f"{name}_gradG2_norm"] = np.array([float(p.grad.double().norm()) for _, p in h.netG.named_parameters()])
    finally:
        utils.func.generate_noise, GS.generate_noise = old


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    GG.install_shims()
    out, pin = {}, {}
    print("[golden-gapool] (a)", flush=True)
    gen_a(out, pin)
    print("[golden-gapool] (b)", flush=True)
    gen_b(out)
    with tempfile.TemporaryDirectory() as tmp:
        print("[golden-gapool] (c)", flush=True)
        gen_c(out, tmp)
    np.savez_compressed(os.path.join(HERE, "gapool_v1.npz"), **out)
    worst = max(v for d in pin.values() for v in d.values())
    meta = {"reference": "liupei101/AdvMIL @ v1", "torch": torch.__version__, "data_seed": DATA_SEED, "param_seed": PARAM_SEED,
            "restatement_vs_reference_maxabs": pin, "worst": worst}
    with open(os.path.join(HERE, "ORACLE_PIN_gapool.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    print(json.dumps(pin, indent=1, sort_keys=True))
    assert worst < 1e-12, worst
    print("size", os.path.getsize(os.path.join(HERE, "gapool_v1.npz")))


if __name__ == "__main__":
    main()
