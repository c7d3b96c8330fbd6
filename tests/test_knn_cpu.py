"""CPU: the k-NN graph construction without a GPU -- the oracle's own definition (tests/knn_ref.py) on cases written out by hand, the
three new entry points in header / binding table / library, every validation rule of the two launching ones (argument checks run before
anything is enqueued: fake aligned addresses, as tests/test_abi_negative_cpu.py; EVERY call below is an invalid one), and the Python
layer's refusals and pure-torch helpers (advmil_amd/ops.py knn_*, advmil_amd/wsigraph.py)."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import knn_ref as R
from tests.test_abi_cpu import header_symbols

EINVAL, EWORKSPACE = -1, -2
A16 = 0x7F0000001000
NEW = ("advmil_knn_spatial", "advmil_knn_latent_workspace_bytes", "advmil_knn_latent")


def p(k, off=0):
    return ctypes.c_void_p(A16 + (k << 20) + off)


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from advmil_amd import _lib
    return _lib


# ------------------------------------------------------------------------------------------------------------------------------
# the oracle
# ------------------------------------------------------------------------------------------------------------------------------
def test_oracle_on_a_3x3_grid_by_hand():
    """Row-major 3 x 3 grid, ids 0..8. Centre (4): the four edge cells at d2 = 1 in id order, then the four corners at d2 = 2.
    Corner (0): 1 and 3 at d2 = 1, 4 at 2, 2 and 6 at 4, 5 and 7 at 5, 8 at 8."""
    xy = np.array([[c, r] for r in range(3) for c in range(3)])
    o = R.knn(xy, 8)
    assert o["nbr"][4].tolist() == [1, 3, 5, 7, 0, 2, 6, 8] and o["dist2"][4].tolist() == [1, 1, 1, 1, 2, 2, 2, 2]
    assert o["nbr"][0].tolist() == [1, 3, 4, 2, 6, 5, 7, 8] and o["dist2"][0].tolist() == [1, 1, 2, 4, 4, 5, 5, 8]
    assert o["nbr"].dtype == np.int32 and o["dist2"].dtype == np.int64
    lat = R.knn(xy.astype(np.float32), 3, latent=True)
    assert lat["nbr"][4].tolist() == [1, 3, 5] and lat["dist2"][0].tolist() == [1.0, 1.0, 2.0]


def test_oracle_duplicates_self_by_index_bags_and_short_bags():
    xy = np.array([[5, 5], [9, 9], [5, 5], [5, 5], [6, 5]])
    o = R.knn(xy, 2)
    assert o["nbr"][0].tolist() == [2, 3] and o["dist2"][0].tolist() == [0, 0]          # duplicates at distance 0 are neighbours
    assert o["nbr"][2].tolist() == [0, 3] and o["nbr"][3].tolist() == [0, 2]            # ... self leaves by index, the tie by id
    assert o["nbr"][4].tolist() == [0, 2]
    two = R.knn(np.concatenate([xy, xy + 100]), 2, lens=[5, 5])
    assert np.array_equal(two["nbr"][5:], o["nbr"]) and np.array_equal(two["nbr"][:5], o["nbr"])     # bag-local ids, no id leaves its bag
    short = R.knn(xy[:2], 3)
    assert short["nbr"].tolist() == [[1, -1, -1], [0, -1, -1]] and short["dist2"][0].tolist() == [32, np.iinfo(np.int64).max, np.iinfo(np.int64).max]


# ------------------------------------------------------------------------------------------------------------------------------
# the ABI
# ------------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_in_header_table_and_library(L):
    syms = header_symbols()
    handle = ctypes.CDLL(L.LIB_PATH)
    for name in NEW:
        assert name in syms and name in L.SIGNATURES and hasattr(handle, name), name
    lib = L.lib()
    assert lib.advmil_knn_latent_workspace_bytes(1000, 64, 8) == 4000
    assert lib.advmil_knn_latent_workspace_bytes(1001, 1024, 16) == 4016            # O(N): the rows' squared norms, rounded to 16 bytes
    assert lib.advmil_knn_latent_workspace_bytes(1000, 64, 17) == 0 and lib.advmil_knn_latent_workspace_bytes(0, 64, 8) == 0


def test_spatial_entry_validates_before_it_launches(L):
    lib = L.lib()
    f = lambda xy=p(0), N=100, k=8, nseg=1, seg=None, mlen=100, nbr=p(1), d2=p(2): lib.advmil_knn_spatial(   # noqa: E731
        xy, N, k, nseg, seg, mlen, nbr, d2, None)
    assert f(xy=None) == EINVAL and f(nbr=None) == EINVAL
    assert f(N=0, mlen=0) == EINVAL and f(N=-3) == EINVAL
    assert f(k=0) == EINVAL and f(k=17) == EINVAL
    assert f(nseg=0) == EINVAL and f(nseg=4, mlen=25) == EINVAL                      # four bags, no offsets
    assert f(mlen=0) == EINVAL and f(mlen=101) == EINVAL
    assert f(xy=p(0, 4)) == EINVAL                                                   # coordinates are read as pairs
    assert f(N=1 << 31, mlen=5) == EINVAL                                            # ids are int32


def test_latent_entry_validates_before_it_launches(L):
    lib = L.lib()
    N, C, k = 100, 64, 8
    need = lib.advmil_knn_latent_workspace_bytes(N, C, k)
    f = lambda hi=p(0), lo=p(1), ldx=C, N=N, C=C, k=k, nseg=1, seg=None, mlen=N, nbr=p(2), d2=p(3), ws=p(4), wsb=need: (   # noqa: E731
        lib.advmil_knn_latent(hi, lo, ldx, N, C, k, nseg, seg, mlen, nbr, d2, ws, wsb, None))
    assert f(hi=None) == EINVAL and f(lo=None) == EINVAL and f(nbr=None) == EINVAL and f(ws=None) == EINVAL
    assert f(N=0, mlen=0) == EINVAL
    assert f(k=0) == EINVAL and f(k=17) == EINVAL
    assert f(C=48, ldx=48) == EINVAL and f(C=0, ldx=0) == EINVAL                     # C % 32
    assert f(hi=p(0, 8)) == EINVAL and f(lo=p(1, 2)) == EINVAL                       # planes are read in 16-byte units
    assert f(ldx=60) == EINVAL and f(ldx=68) == EINVAL                               # ... every row of them: pitch >= C, pitch % 8
    assert f(nseg=3, mlen=40) == EINVAL                                              # three bags, no offsets
    assert f(mlen=0) == EINVAL and f(mlen=N + 1) == EINVAL
    assert f(wsb=need - 4) == EWORKSPACE and f(wsb=0) == EWORKSPACE


# ------------------------------------------------------------------------------------------------------------------------------
# the Python layer
# ------------------------------------------------------------------------------------------------------------------------------
def test_edges_from_neighbours_layout():
    from advmil_amd.wsigraph import edges_from_neighbours
    nbr = torch.tensor([[1, 2], [0, 2], [1, 0]], dtype=torch.int32)
    ei = edges_from_neighbours(nbr)
    assert ei.dtype == torch.int64 and ei.tolist() == [[0, 0, 1, 1, 2, 2], [1, 2, 0, 2, 1, 0]]


def test_merge_graphs_offsets_on_cpu_tensors():
    from advmil_amd.wsigraph import edges_from_neighbours, merge_graphs
    g = lambda n, c0: SimpleNamespace(x=torch.full((n, 4), float(c0)), centroid=torch.arange(2 * n).reshape(n, 2) + c0,   # noqa: E731
                                      edge_index=edges_from_neighbours(torch.arange(n).roll(1).reshape(n, 1)),
                                      edge_latent=edges_from_neighbours(torch.arange(n).roll(-1).reshape(n, 1)))
    a, b, c = g(3, 0), g(2, 10), g(4, 20)
    m = merge_graphs([a, b, c])
    assert m.x.shape == (9, 4) and m.x[:, 0].tolist() == [0.0] * 3 + [10.0] * 2 + [20.0] * 4
    assert m.centroid.shape == (9, 2) and torch.equal(m.centroid[3:5], b.centroid)
    assert m.edge_index.tolist() == [[0, 1, 2, 3, 4, 5, 6, 7, 8], [2, 0, 1, 4, 3, 8, 5, 6, 7]]
    assert m.edge_latent.tolist() == [[0, 1, 2, 3, 4, 5, 6, 7, 8], [1, 2, 0, 4, 3, 6, 7, 8, 5]]
    a.edge_latent = None
    with pytest.raises(ValueError, match="edge_latent"):
        merge_graphs([a, b])
    b.edge_latent = None
    assert merge_graphs([a, b]).edge_latent is None


def test_cpu_tensors_have_no_fallback(L):
    from advmil_amd import ops, wsigraph
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.knn_spatial(torch.zeros(20, 2, dtype=torch.int32), 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.knn_latent(torch.zeros(20, 32), 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        wsigraph.build_graph(torch.zeros(20, 32), torch.zeros(20, 2), k=8)


def test_short_bags_and_bad_k_are_refused_by_name():
    from advmil_amd import ops
    seg = ops.Segments([20, 8, 30], "cpu")
    with pytest.raises(ValueError, match="bag 1 has 8 rows"):
        ops.knn_spatial(torch.zeros(58, 2, dtype=torch.int32), 8, seg)
    with pytest.raises(ValueError, match="bag 1 has 8 rows"):
        ops.knn_latent(torch.zeros(58, 32), 8, seg)
    with pytest.raises(ValueError, match="bag 0 has 8 rows"):
        ops.knn_latent(torch.zeros(8, 32), 8)
    with pytest.raises(ValueError, match="cover 58 rows"):
        ops.knn_spatial(torch.zeros(60, 2, dtype=torch.int32), 4, seg)
    for k in (0, 17, 2.0, True):
        with pytest.raises(ValueError, match="k = "):
            ops.knn_spatial(torch.zeros(40, 2, dtype=torch.int32), k)


def test_coordinates_must_be_integers_below_2_30():
    from advmil_amd import ops
    ok = ops.knn_coords_int32(torch.tensor([[0.0, 256.0], [-512.0, 2.0 ** 29]]))
    assert ok.dtype == torch.int32 and ok.tolist() == [[0, 256], [-512, 1 << 29]]
    assert ops.knn_coords_int32(torch.tensor([[(1 << 30) - 1, -(1 << 30) + 1]], dtype=torch.int64)).tolist() == [[(1 << 30) - 1, -(1 << 30) + 1]]
    for bad in (torch.tensor([[0.5, 1.0]]), torch.tensor([[float("nan"), 1.0]]), torch.tensor([[2.0 ** 30, 0.0]]), torch.tensor([[1e30, 0.0]]),
                torch.tensor([[1 << 30, 0]], dtype=torch.int64), torch.tensor([[0, -(1 << 30)]], dtype=torch.int32),
                torch.tensor([[1 << 40, 0]], dtype=torch.int64), torch.zeros(4, 3, dtype=torch.int32), torch.zeros(4, 2, dtype=torch.uint8)):
        with pytest.raises(ValueError):
            ops.knn_coords_int32(bad)
