"""GPU: the training step, the handler's own epoch loop, the batched evaluation and a baseline step under allocation poisoning
(tests/poison.py; DESIGN.md section 2, "Allocation poisoning"). No oracle here: the plain run is the reference, and every result of a
run whose fresh allocations were filled with 0xFF (NaN / -1) or 0x7F (3.39e38 / 2139062143) must equal it bit for bit -- predictions,
scores, logged statistics, attention, every gradient and weight. What each case computes is pinned to float64 by the module it borrows
its runner from (test_step_dropout_oracle_gpu.py, test_step_graphs_gpu.py, test_eval_batched_gpu.py, test_baseline_gpu.py).

A result that moves with the pattern is a finding: named here with its fix, the case stays. Found so far: none (every case passed when the module was introduced)."""
import pytest
import torch

from advmil_amd.config import default_baseline_cfg
from tests import helpers as H
from tests import poison as P
from tests.test_parity_gpu import DEV, load_synth
from tests.test_step_dropout_oracle_gpu import CASES, gpu_step, make_bags

pytestmark = pytest.mark.gpu

# name: (kind, lens, events, pad to a multiple of, first bag seed); the third: an ESAT step with a ragged last bag (4080 = 255 regions)
STEP_CASES = {"abmil_ragged": CASES["abmil_ragged"][:5], "misl_ragged": CASES["misl_ragged"][:5],
              "esat_ragged": ("patch", (4096, 4096, 4080), (1, 0, 1), 256, 80)}


@pytest.mark.timeout(600)
@pytest.mark.parametrize("name", sorted(STEP_CASES))
def test_slab_step_does_not_move_with_what_its_buffers_held(name):
    """gpu_step: one D backward and one G backward over a staged slab (ragged bags + zero pad rows; the slab itself comes from
    torch.zeros and stays that way), bf16x3, shipped dropout."""
    kind, lens, events, pad_to, seed0 = STEP_CASES[name]
    bags = make_bags(kind, lens, events, seed0)
    nd = [[H.noise_tensor("sd_d", i, 192)] for i in range(len(bags))]
    ng = [[H.noise_tensor("sd_g", i, 192)] for i in range(len(bags))]

    def run():
        G = gpu_step(kind, bags, pad_to, "bf16x3", nd, ng)
        assert G["pad"] == (-sum(lens)) % pad_to and G["pad"] > 0
        return {k: G[k] for k in ("preds_d", "fakes", "pred_g", "A", "gD", "gG", "logs", "n_real")}

    trees = P.three_runs(run)
    P.assert_same_bits(trees)
    for t in trees:
        P.assert_finite(t)
    assert all(float(g.abs().max()) > 0 for g in (trees[0]["gD"]["net_pair_one.embedding.conv.weight"], trees[0]["pred_g"]))


@pytest.mark.timeout(600)
def test_epoch_loop_with_its_stager_graphs_and_bag_cache_does_not_move():
    """The handler's own loop (test_step_graphs_gpu._epochs, graphs on, bag lengths that put the slab pad in play): first-sight eager
    steps, captures and replays, SlabStager's pinned and device slabs (pad rows included), the bag cache, the graphs' private pool."""
    from advmil_amd import ops
    from tests.test_step_graphs_gpu import _epochs
    prev = ops.get_gemm_mode()

    def run():
        h, cls, logs = _epochs(True, odd=True)
        return {"cls": [{k: c[k] for k in ("y", "y_hat", "f_fake")} for c in cls], "logs": logs, "stats": dict(h.step_graph_stats),
                "G": h.optimizerG.flat_param, "D": h.optimizerD.flat_param, "tG": h.optimizerG.step_t, "tD": h.optimizerD.step_t}
    try:
        trees = P.three_runs(run)
    finally:
        ops.set_gemm_mode(prev)
    P.assert_same_bits(trees)
    for t in trees:
        P.assert_finite(t)
    assert trees[0]["stats"] == {"replayed": 12, "captured": 4, "eager": 4} and len(trees[0]["logs"]) == 2 * 10 * 2


@pytest.mark.parametrize("kind,disc", [("abmil", ("prj", "instance", "x")), ("patch", ("prj", "bag", "x"))])
def test_batched_evaluation_does_not_move(kind, disc):
    """MyHandler.test_model in slabs of 3 ragged bags (with a remainder), 7 head samples per bag, bf16x3."""
    from advmil_amd.model import MyHandler
    from tests.test_eval_batched_gpu import bf16x3_mode, make, nets
    lens = (256, 128, 512, 64, 192, 384, 320)
    with bf16x3_mode():
        g, d = nets(kind, disc)
        items = make(kind, lens)
        noises = [[H.noise_tensor(f"ev:{kind}:{i}", k, 192, DEV) for k in range(8)] for i in range(len(lens))]
        trees = P.three_runs(lambda: MyHandler.test_model(g, d, kind, items, times_test_sample=7, noise=noises, batch_bags=3))
    P.assert_same_bits(trees)
    for t in trees:
        P.assert_finite(t)
    assert trees[0]["dist_y_hat"].shape == (len(lens), 7, 1)


def test_two_baseline_steps_with_dropout_do_not_move():
    """BaselineHandler, abmil / surv_reg, shipped dropout, two optimizer steps over host bags (the shared ingest)."""
    from advmil_amd import ops
    from advmil_amd.model import BaselineHandler
    NB, N = 8, 512
    loader = [(torch.tensor([[i]], dtype=torch.int), [H.bag(100 + i, N), torch.zeros(1, 1)], H.label(i).clone()) for i in range(2 * NB)]
    prev = ops.get_gemm_mode()

    def run():
        h = BaselineHandler(default_baseline_cfg(bcb_mode="abmil", task="surv_reg", pdh_dims="384-1", bp_every_batch=NB, gemm_mode="bf16x3"), device=DEV)
        load_synth(h.net, "S-abmil_reg:")
        h.rng.reset(77)
        cl = h._train_each_epoch(loader, "train")
        torch.cuda.synchronize()
        return {"y_hat": cl["y_hat"], "y": cl["y"], "logs": h.pop_logs(), "P": {k: v for k, v in h.net.state_dict().items()}}
    try:
        trees = P.three_runs(run)
    finally:
        ops.set_gemm_mode(prev)
    P.assert_same_bits(trees)
    for t in trees:
        P.assert_finite(t)
    assert len(trees[0]["logs"]) == 2


def test_fill_reaches_pinned_host_memory_and_is_a_node_of_a_captured_graph():
    """The harness on the device: pinned host blocks are filled through every entry point that can ask for them (SlabStager's slabs), and
    a fill issued while a stream is being captured is an ordinary node of the graph -- every replay poisons the block again."""
    for byte in P.PATTERNS:
        with P.poisoned_allocations(byte):
            a = torch.empty(64, pin_memory=True)
            b = torch.empty_like(a, pin_memory=True)
            c = a.new_empty(8, pin_memory=True)
            d = torch.empty(16)                                   # pageable: left alone without host=True
            d.fill_(1.0)
        for t in (a, b, c):
            assert t.is_pinned() and bool((t.view(torch.uint8) == byte).all())
        assert float(d.sum()) == 16.0
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph, stream=side):
                with P.poisoned_allocations(byte):
                    t = torch.empty(1000, device=DEV)
                    h = torch.empty(8, pin_memory=True)          # (inside a capture the keyword alone decides: no driver query)
        assert bool((h.view(torch.uint8) == byte).all())
        for _ in range(2):
            graph.replay()
            torch.cuda.synchronize()
            assert bool((t.view(torch.uint8) == byte).all())
            t.zero_()
        torch.cuda.synchronize()
