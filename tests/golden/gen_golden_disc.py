#!/usr/bin/env python3
"""Golden vectors of the discrete-time adversarial task (task: disc_gansurv) from the REAL reference, run on the CPU through the import
shims of gen_golden.py, and the pin of the float64 restatement (tests/disc_ref.py) against the reference's own functions in the same run.

Runs only in the build container (the reference never travels). Inputs and weights are regenerated from the repo's counter RNG
(advmil_amd/synth.py) and from tests/disc_ref.py::loss_cases, so the fixtures hold only outputs: tests/golden/golden_disc_v1.npz and
tests/golden/ORACLE_PIN_disc.json. Usage:  python tests/golden/gen_golden_disc.py

  (a) LM_* / MLE_*: utils.func.get_label_mask over every (t, e) of K in {1, 4, 7}; loss.utils.SurvMLE value and gradient (float64) on
      every case of disc_ref.loss_cases() and on its float64 extreme case.
  (b) D4_{abmil,patch}_*: two optimizer steps of MyHandler._train_each_epoch with task=disc_gansurv, time_bins=4, gen_dims=384-4,
      disc_nety_in_dim=4, dropout zeroed, injected noise, 2 x 16 bags of 512 rows, bin labels floor(4 t) of synth.label.
  (c) D4c_abmil_*: the same in mode='wolabel' with every third bag's label invisible.
  (d) D5_*: MyHandler.test_model on 8 of those bags: test_zero_noise=True, and 3 injected-noise samples.
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
from tests import disc_ref as R  # noqa: E402

T, REF, DATA_SEED, LOG = GG.T, GG.REF, GG.DATA_SEED, GG.LOG
BINS = 4


def bin_label(i):
    y = synth.label(DATA_SEED, i).copy()
    y[0, 0] = np.floor(BINS * y[0, 0])
    return T(y)


def gen_a(out, pin):
    from loss.utils import SurvMLE
    from utils.func import get_label_mask
    d_lm = 0.0
    for K in (1, 4, 7):
        t = np.repeat(np.arange(K, dtype=np.float32), 2).reshape(-1, 1)
        e = np.tile(np.array([0.0, 1.0], dtype=np.float32), K).reshape(-1, 1)
        label, mask = get_label_mask(T(t), T(e), K)
        out[f"LM_K{K}_t"], out[f"LM_K{K}_e"] = t, e
        out[f"LM_K{K}_label"], out[f"LM_K{K}_mask"] = label.numpy(), mask.numpy()
        out[f"LM_K{K}_real"] = (label * mask).numpy()
        rl, rm = R.get_label_mask(t, e, K)
        d_lm = max(d_lm, float(np.abs(rl - label.numpy()).max()), float(np.abs(rm - mask.numpy()).max()),
                   float(np.abs(R.real_rows(t, e, K) - (label * mask).numpy()).max()))
    pin["a/get_label_mask"] = {"max": d_lm}
    dv = dg = 0.0
    for c in R.loss_cases() + [R.extreme_case_f64()]:
        hz = T(c["hz"].astype(np.float64)).requires_grad_(True)
        t, e = T(c["t"].astype(np.float64)).reshape(-1, 1), T(c["e"].astype(np.float64)).reshape(-1, 1)
        loss = SurvMLE(alpha=c["alpha"], eps=c["eps"])(hz, t, e)
        loss.backward()
        out[f"MLE_{c['name']}_value"] = np.array(float(loss), dtype=np.float64)
        out[f"MLE_{c['name']}_grad"] = hz.grad.numpy()
        rv, rg = R.surv_mle(c["hz"], c["t"], c["e"], c["alpha"], c["eps"])
        dv, dg = max(dv, abs(rv - float(loss))), max(dg, float(np.abs(rg - hz.grad.numpy()).max()))
    pin["a/SurvMLE"] = {"value": dv, "grad": dg}


def _patched_noise():
    import utils.func
    import model.GANSurv as GS
    nq = GG.NoiseQueue()
    old = (utils.func.generate_noise, GS.generate_noise)
    utils.func.generate_noise = nq
    GS.generate_noise = nq
    return nq, old


def _restore_noise(old):
    import utils.func
    import model.GANSurv as GS
    utils.func.generate_noise, GS.generate_noise = old


def disc_cfg(kind, tmp):
    cfg = dict(yaml.load(open(os.path.join(REF, "config/cfg_nlst.yaml")), Loader=yaml.FullLoader))
    # (the ctor reads max t from cfg['path_label'] for time_format 'quantile' -- model_handler.py:112-113 -- though the discrete
    # evaluator never uses it: a two-line table stands in)
    table = os.path.join(tmp, "labels.csv")
    with open(table, "w") as f:
        f.write("patient_id,t,e\np0,1.0,1\n")
    cfg.update(task="disc_gansurv", time_format="quantile", time_bins=BINS, gen_dims=f"384-{BINS}", disc_nety_in_dim=BINS, log_plot=False,
               bcb_mode=kind, data_split_seed=0, save_path=os.path.join(tmp, f"save_{kind}"), wandb_dir=tmp, num_workers=0,
               bp_every_batch=16, path_label=table)
    return cfg


def run_steps(out, name, kind, tag, mode, visible, tmp):
    from model.model_handler import MyHandler
    nq, old = _patched_noise()
    try:
        h = MyHandler(disc_cfg(kind, tmp))
        assert h.task == "disc_gansurv" and h.nbins == BINS
        PG = GG.load_synth(h.netG, prefix=f"G-{kind}:")
        PD = GG.load_synth(h.netD, prefix="D-prj:")
        GG.zero_dropout(h.netG); GG.zero_dropout(h.netD)
        nb, N = 32, 512
        h.patient_id["train"] = [str(i) for i in range(nb)]
        h.patient_id["label_visible"] = [str(i) for i in range(nb) if visible(i)]
        loader = [(torch.tensor([[i]], dtype=torch.int), [T(synth.bag(DATA_SEED, i, N)), torch.zeros(1, 1)], bin_label(i)) for i in range(nb)]
        width = h.netG.MLPs[1][0].in_features // 2           # the noise is concatenated at the hidden width get_hop_dims gives
        out[f"{name}_noise_width"] = np.array(width)
        noise_d = [GG.noise_tensor(f"{tag}d:{kind}", i, width) for i in range(nb)]
        noise_g = [GG.noise_tensor(f"{tag}g:{kind}", i, width) for i in range(nb)]
        for s in range(2):
            nq.q.extend(noise_d[16 * s:16 * s + 16])
            nq.q.extend(noise_g[16 * s:16 * s + 16])
        LOG.clear()
        cl = h._train_each_epoch(loader, "train", mode=mode)
        assert not nq.q
        logs = [{k.split("/")[-1]: v for k, v in d.items()} for d in LOG]
        refG = {k: v.detach() for k, v in h.netG.state_dict().items()}
        refD = {k: v.detach() for k, v in h.netD.state_dict().items()}
        out[f"{name}_logs"] = np.array(
            [[logs[2 * s][k] for k in ("Loss_D", "D_real", "D_fake")] +
             [logs[2 * s + 1][k] for k in ("Loss_G_fake", "Loss_G_time", "Loss_G_total", "D_fake_avg")] for s in range(2)], dtype=np.float64)
        out[f"{name}_y_hat"] = cl["y_hat"].numpy()
        out[f"{name}_f_fake"] = cl["f_fake"].numpy()
        out[f"{name}_y"] = cl["y"].numpy()
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
        return cl
    finally:
        _restore_noise(old)


def gen_d(out, tmp):
    from types import SimpleNamespace
    from model.backbone import load_backbone
    from model.GANSurv import Generator, PrjDiscriminator
    from model.model_handler import MyHandler
    nq, old = _patched_noise()
    try:
        kind = "abmil"
        g = Generator(384, BINS, load_backbone(kind, [1024, 384, 384]), SimpleNamespace(noise=[0, 1], hops=1, noise_dist="uniform"),
                      False, 0.6, "sigmoid")
        ax = SimpleNamespace(in_dim=1024, out_dim=128, ksize=1, backbone="avgpool", dropout=0.25)
        ay = SimpleNamespace(in_dim=BINS, hid_dims=[64, 128], norm=False, dropout=0.0)
        d = PrjDiscriminator(ax, ay, prj_path="x", inner_product="instance")
        GG.load_synth(g, prefix=f"G-{kind}:"); GG.load_synth(d, prefix="D-prj:")
        nb, N, S = 8, 512, 3
        loader = [(torch.tensor([[i]], dtype=torch.int), [T(synth.bag(DATA_SEED, i, N)), torch.zeros(1, 1)], bin_label(i)) for i in range(nb)]
        res = MyHandler.test_model(g, d, kind, loader, times_test_sample=1, checkpoints=None, test_zero_noise=True)
        out["D5_zero_y_hat"], out["D5_zero_f_fake"] = res["y_hat"].numpy(), res["f_fake"].numpy()
        for i in range(nb):
            nq.q.extend(GG.noise_tensor(f"D5:{kind}:{i}", k, 192) for k in range(S + 1))
        res = MyHandler.test_model(g, d, kind, loader, times_test_sample=S, checkpoints=None, test_zero_noise=False)
        assert not nq.q
        for k in ("y_hat", "f_fake", "dist_y_hat", "avg_y_hat"):
            out[f"D5_noise_{k}"] = res[k].numpy()
        assert out["D5_noise_dist_y_hat"].shape == (nb, S, BINS) and out["D5_noise_avg_y_hat"].shape == (nb, BINS)
    finally:
        _restore_noise(old)


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    GG.install_shims()
    out, pin = {}, {}
    print("[golden-disc] (a)", flush=True)
    gen_a(out, pin)
    with tempfile.TemporaryDirectory() as tmp:
        for kind in ("abmil", "patch"):
            print("[golden-disc] (b)", kind, flush=True)
            cl = run_steps(out, f"D4_{kind}", kind, "D4", "wlabel", lambda i: True, tmp)
            assert tuple(cl["y_hat"].shape) == (32, BINS) and tuple(cl["f_fake"].shape) == (32,)
        print("[golden-disc] (c)", flush=True)
        run_steps(out, "D4c_abmil", "abmil", "D4c", "wolabel", lambda i: i % 3 != 0, tmp)
        print("[golden-disc] (d)", flush=True)
        gen_d(out, tmp)
    np.savez_compressed(os.path.join(HERE, "golden_disc_v1.npz"), **out)
    worst = max(v for d in pin.values() for v in d.values())
    meta = {"reference": "liupei101/AdvMIL @ v1", "torch": torch.__version__, "data_seed": DATA_SEED, "param_seed": GG.PARAM_SEED,
            "restatement_vs_reference_maxabs": pin, "worst": worst}
    with open(os.path.join(HERE, "ORACLE_PIN_disc.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    print(json.dumps(pin, indent=1, sort_keys=True))
    assert worst < 1e-12, worst


if __name__ == "__main__":
    main()
