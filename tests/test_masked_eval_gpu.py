"""The occlusion-robustness test out of the resident bag cache (reference model_handler.py:189-224 `exec_test` with
test_mask_ratio / baseline_handler.py:215; the reference's dataset zeroes random 4x4 square instances on the host in __getitem__:
dataset/PatchWSI.py:80-81 -> utils/func.py:14-40): `test_model(clean loader, mask_ratio=r)` masks on the device, in the launch that
stages a bag into the step slab (advmil_stage_bag_masked), and keeps the CLEAN bag in the cache.

The reference for every comparison is the only route there was before: a dataset that masks on the host (with this repo's
random_mask_square_instance, pinned to the reference's draws by tests/test_mask_cpu.py) and is therefore never cached
(`ratio_mask` set -> ingest.dataset_scope is False). Same seed, same bag order -> the same masks -> the same slab, bit for bit.
Every test runs under both allocation-poison patterns of tests/poison.py."""
import warnings

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import poison as P
from tests import test_eval_batched_gpu as EB
from tests.test_parity_gpu import DEV, load_synth

pytestmark = pytest.mark.gpu
RATIO = 0.8
DISC = {"abmil": ("prj", "instance", "x"), "patch": ("prj", "bag", "x"), "cluster": ("cat", "bag", None)}
RAGGED = (16, 48, 528, 1040)           # one slab of 4 bags, 1632 rows: below the plane threshold (a cached pass back-fills its rows)
PADDED = (2048, 2064)                  # 4112 rows: operand planes, and the 240-row slab pad sits behind masked bags


@pytest.fixture(params=P.PATTERNS, ids=["nan_ff", "big_7f"])
def byte(request):
    return request.param


class gemm_mode:
    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        from advmil_amd import ops
        self.prev = ops.get_gemm_mode()
        ops.set_gemm_mode(self.mode)

    def __exit__(self, *exc):
        from advmil_amd import ops
        ops.set_gemm_mode(self.prev)
        return False


_ITEMS = {}


def clean_items(kind, lens):
    """Host bags of a cohort, built once and never written (every loader of a test wraps the same tensors)."""
    key = (kind, tuple(lens))
    if key not in _ITEMS:
        _ITEMS[key] = EB.make(kind, lens, start=700)
    return _ITEMS[key]


def host_masked(items, seed, ratio=RATIO, rng=None):
    """The parent's route: every bag masked on the host, one draw per bag in loader order -> a dataset that is never cached."""
    from advmil_amd.utils.func import mask_square_rows, square_instance_keep
    if rng is None:
        np.random.seed(seed)
    out = []
    for idx, (x, ext), y in items:
        keep = square_instance_keep(x.shape[1], ratio, rng=rng)
        out.append((idx, [mask_square_rows(x[0], keep).unsqueeze(0), ext], y))
    return EB.Dataset(out, ratio_mask=ratio)


def noises_for(n, k=1, tag="mk"):
    return [[H.noise_tensor(f"{tag}:{i}", c, 192, DEV) for c in range(k)] for i in range(n)]


def equal(a, b):
    assert set(a) == set(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), (k, float((a[k].double() - b[k].double()).abs().max()))
        assert bool(torch.isfinite(a[k].double()).all()), k


def rng_state_equal(s0, s1):
    return s0[0] == s1[0] and np.array_equal(s0[1], s1[1]) and s0[2:] == s1[2:]


# ---- A: bit equality with the host-masking, uncached route ------------------------------------------------------------------------
@pytest.mark.parametrize("lens,bb", [(RAGGED, 4), (PADDED, 4)], ids=["ragged", "padded"])
@pytest.mark.parametrize("mode", ["exact", "bf16x3"])
@pytest.mark.parametrize("kind", ["abmil", "patch"])
def test_device_masked_eval_equals_host_masked_eval(byte, kind, mode, lens, bb):
    from advmil_amd.model import MyHandler
    g, d = EB.nets(kind, DISC[kind])
    items = clean_items(kind, lens)
    nz = noises_for(len(lens))
    with gemm_mode(mode), P.poisoned_allocations(byte):
        want = MyHandler.test_model(g, d, kind, EB.Loader(host_masked(items, 3)), noise=nz, batch_bags=bb)
        np.random.seed(3)
        got = MyHandler.test_model(g, d, kind, EB.Loader(EB.Dataset(items)), noise=nz, batch_bags=bb, mask_ratio=RATIO)
    equal(got, want)


def test_device_masked_eval_equals_host_masked_eval_bf16_storage(byte):
    from advmil_amd.model import MyHandler
    g, d = EB.nets("abmil")
    items = clean_items("abmil", RAGGED)
    nz = noises_for(len(RAGGED))
    with gemm_mode("bf16x3"), P.poisoned_allocations(byte):
        want = MyHandler.test_model(g, d, "abmil", EB.Loader(host_masked(items, 4)), noise=nz, batch_bags=4, x_storage="bf16")
        ds = EB.Dataset(items)
        for _ in range(2):                         # a first visit (masked in place behind the rounding) and a pass out of the cache
            np.random.seed(4)
            got = MyHandler.test_model(g, d, "abmil", EB.Loader(ds), noise=nz, batch_bags=4, x_storage="bf16", mask_ratio=RATIO)
            equal(got, want)


def test_device_masked_eval_equals_host_masked_eval_three_zero_noise_samples(byte):
    from advmil_amd.model import MyHandler
    g, d = EB.nets("abmil")
    items = clean_items("abmil", RAGGED)
    with P.poisoned_allocations(byte):
        want = MyHandler.test_model(g, d, "abmil", EB.Loader(host_masked(items, 5)), times_test_sample=3, test_zero_noise=True, batch_bags=4)
        np.random.seed(5)
        got = MyHandler.test_model(g, d, "abmil", EB.Loader(EB.Dataset(items)), times_test_sample=3, test_zero_noise=True, batch_bags=4,
                                   mask_ratio=RATIO)
    equal(got, want)
    assert got["dist_y_hat"].shape == (len(RAGGED), 3, 1)


# ---- B: the cache keeps the clean bag ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,lens,held", [("exact", RAGGED, False), ("bf16x3", RAGGED, False), ("bf16x3", PADDED, False),
                                            ("bf16x3", PADDED, True)], ids=["exact", "bf16x3-backfill", "bf16x3-planes-only", "bf16x3-held-planes"])
def test_the_cache_stays_clean_under_masked_passes(byte, monkeypatch, mode, lens, held):
    """After a masked first pass: the unmasked pass out of the cache == the unmasked pass with the cache off; the same seed again is
    all cache hits and the same result (also the host-masked one); another seed is another result. `held`: entries that carry their
    operand planes (ADVMIL_CACHE_PLANES=1) -- the copied-planes form of the launch."""
    from advmil_amd import ingest
    from advmil_amd.model import MyHandler
    g, d = EB.nets("abmil")
    items = clean_items("abmil", lens)
    nz = noises_for(len(lens))
    cache = ingest.device_bag_cache(DEV)
    monkeypatch.setattr(cache, "with_planes", held)
    ds = EB.Dataset(items)
    run = lambda loader, **kw: MyHandler.test_model(g, d, "abmil", loader, noise=nz, batch_bags=4, **kw)      # noqa: E731
    with gemm_mode(mode), P.poisoned_allocations(byte):
        s0 = cache.stats()
        np.random.seed(1)
        m1 = run(EB.Loader(ds), mask_ratio=RATIO)
        s1 = cache.stats()
        assert (s1["misses"] - s0["misses"], s1["hits"] - s0["hits"]) == (len(lens), 0)
        clean_cached = run(EB.Loader(ds))
        s2 = cache.stats()
        assert (s2["misses"] - s1["misses"], s2["hits"] - s1["hits"]) == (0, len(lens))
        monkeypatch.setenv("ADVMIL_BAG_CACHE_GB", "0")
        clean_uncached = run(EB.Loader(ds))
        monkeypatch.delenv("ADVMIL_BAG_CACHE_GB")
        assert cache.stats() == s2
        equal(clean_cached, clean_uncached)
        np.random.seed(1)
        m2 = run(EB.Loader(ds), mask_ratio=RATIO)
        s3 = cache.stats()
        assert (s3["misses"] - s2["misses"], s3["hits"] - s2["hits"]) == (0, len(lens))
        equal(m2, m1)
        # the cached pass took the form this case is named after: operand planes only (the slab's fp32 rows stay stale) or not
        stager = ingest.device_stager(DEV, 1024, torch.float32, torch.float32)
        assert stager.stale == (mode == "bf16x3" and lens is PADDED and not held)
        equal(m2, run(EB.Loader(host_masked(items, 1))))
        np.random.seed(2)
        m3 = run(EB.Loader(ds), mask_ratio=RATIO)
        assert not torch.equal(m3["y_hat"], m1["y_hat"]) and not torch.equal(m1["y_hat"], clean_cached["y_hat"])
        equal(m3, run(EB.Loader(host_masked(items, 2))))


# ---- C: the per-bag paths see the same masks ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["abmil", "patch"])
def test_per_bag_paths_agree_with_the_batched_result(byte, kind):
    from advmil_amd.model import MyHandler
    g, d = EB.nets(kind, DISC[kind])
    items = clean_items(kind, RAGGED)
    on_device = [(i, [x.to(DEV), ext], y) for i, (x, ext), y in items]
    nz = noises_for(len(RAGGED))
    with P.poisoned_allocations(byte):
        out = []
        for loader, bb in ((EB.Loader(EB.Dataset(items)), 4), (EB.Loader(EB.Dataset(items)), 1), (on_device, 4)):
            np.random.seed(6)
            out.append(MyHandler.test_model(g, d, kind, loader, noise=nz, batch_bags=bb, mask_ratio=RATIO))
    EB.same(out[1], out[0])
    EB.same(out[2], out[0])
    for x_dev, (_, (x, _), _) in zip((it[1][0] for it in on_device), items):
        assert torch.equal(x_dev.cpu(), x)                                     # the loader's device bags are not written


# ---- D: the float64 oracle on the masked bags ------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["exact", "bf16x3"])
def test_device_masked_eval_against_the_float64_oracle(byte, mode):
    from advmil_amd.model import MyHandler
    g, d = EB.nets("abmil")
    items = clean_items("abmil", RAGGED)
    nz = noises_for(len(RAGGED))
    with gemm_mode(mode), P.poisoned_allocations(byte):
        np.random.seed(8)
        got = MyHandler.test_model(g, d, "abmil", EB.Loader(EB.Dataset(items)), noise=nz, batch_bags=4, mask_ratio=RATIO)
    EB.vs_float64_oracle(got, "abmil", DISC["abmil"], g, d, host_masked(items, 8).items, nz)


# ---- E: the baseline handler -----------------------------------------------------------------------------------------------------
def test_baseline_handler_device_masked_eval_equals_host_masked_eval(byte):
    from advmil_amd.config import default_baseline_cfg
    from advmil_amd.model import BaselineHandler
    h = BaselineHandler(default_baseline_cfg(bcb_mode="abmil", task="surv_reg", bp_every_batch=3), device=DEV)
    load_synth(h.net, "S-abmil-ev:")
    for lens in (RAGGED, PADDED):
        items = clean_items("abmil", lens)
        with P.poisoned_allocations(byte):
            want = BaselineHandler.test_model(h.net, "abmil", EB.Loader(host_masked(items, 9)), times_test_sample=2, batch_bags=4)
            ds = EB.Dataset(items)
            for _ in range(2):                     # first visit, then out of the cache
                np.random.seed(9)
                got = BaselineHandler.test_model(h.net, "abmil", EB.Loader(ds), times_test_sample=2, batch_bags=4, mask_ratio=RATIO)
                equal(got, want)
            np.random.seed(9)
            one = BaselineHandler.test_model(h.net, "abmil", EB.Loader(ds), times_test_sample=2, batch_bags=1, mask_ratio=RATIO)
        EB.same(one, want)


# ---- F: the other cases --------------------------------------------------------------------------------------------------------------
def test_cluster_bags_are_evaluated_unmasked_with_one_warning(byte):
    from advmil_amd.model import MyHandler
    g, d = EB.nets("cluster", DISC["cluster"])
    items = clean_items("cluster", (256, 128, 512))
    nz = noises_for(3)
    with P.poisoned_allocations(byte):
        plain = MyHandler.test_model(g, d, "cluster", EB.Loader(EB.Dataset(items)), noise=nz, batch_bags=2)
        np.random.seed(10)
        s0 = np.random.get_state()
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            got = MyHandler.test_model(g, d, "cluster", EB.Loader(EB.Dataset(items)), noise=nz, batch_bags=2, mask_ratio=RATIO)
    assert len([w for w in rec if "mask_ratio" in str(w.message)]) == 1
    assert rng_state_equal(s0, np.random.get_state())
    equal(got, plain)


@pytest.mark.parametrize("ratio", [None, 0, 1.5])
def test_ratios_the_reference_ignores_are_the_unmasked_call(byte, ratio):
    from advmil_amd.model import MyHandler
    g, d = EB.nets("abmil")
    items = clean_items("abmil", RAGGED)
    nz = noises_for(len(RAGGED))
    with P.poisoned_allocations(byte):
        plain = MyHandler.test_model(g, d, "abmil", EB.Loader(EB.Dataset(items)), noise=nz, batch_bags=4)
        np.random.seed(12)
        s0 = np.random.get_state()
        got = MyHandler.test_model(g, d, "abmil", EB.Loader(EB.Dataset(items)), noise=nz, batch_bags=4, mask_ratio=ratio)
    assert rng_state_equal(s0, np.random.get_state())
    equal(got, plain)


def test_a_given_random_state_leaves_the_global_stream_alone(byte):
    from advmil_amd.model import MyHandler
    g, d = EB.nets("abmil")
    items = clean_items("abmil", RAGGED)
    nz = noises_for(len(RAGGED))
    with P.poisoned_allocations(byte):
        want = MyHandler.test_model(g, d, "abmil", EB.Loader(host_masked(items, 13)), noise=nz, batch_bags=4)
        np.random.seed(99)
        s0 = np.random.get_state()
        got = MyHandler.test_model(g, d, "abmil", EB.Loader(EB.Dataset(items)), noise=nz, batch_bags=4, mask_ratio=RATIO,
                                   mask_rng=np.random.RandomState(13))
    assert rng_state_equal(s0, np.random.get_state())
    equal(got, want)


@pytest.mark.parametrize("bb", [1, 4])
def test_a_bag_that_is_not_whole_regions_raises_before_it_is_staged(byte, bb):
    from advmil_amd import ingest
    from advmil_amd.config import default_baseline_cfg
    from advmil_amd.model import BaselineHandler, MyHandler
    g, d = EB.nets("abmil")
    items = EB.make("abmil", (32, 24), start=720)
    cache = ingest.device_bag_cache(DEV)
    with P.poisoned_allocations(byte):
        n0 = len(cache.entries)
        with pytest.raises(AssertionError, match="bag must consist of square instances."):
            MyHandler.test_model(g, d, "abmil", EB.Loader(EB.Dataset(items[1:])), batch_bags=bb, mask_ratio=RATIO)
        h = BaselineHandler(default_baseline_cfg(bcb_mode="abmil", task="surv_reg", bp_every_batch=3), device=DEV)
        with pytest.raises(AssertionError, match="bag must consist of square instances."):
            BaselineHandler.test_model(h.net, "abmil", EB.Loader(EB.Dataset(items[1:])), batch_bags=bb, mask_ratio=RATIO)
        assert len(cache.entries) == n0
        torch.cuda.synchronize()
