"""Gromov hyperbolicity on the GPU (hm_gromov.hip) against the numpy truth of tests/hyperbolicity_cases.py:
values compared by bits, witnesses by value, for both forms of the kernel, at the sizes where the tile edge (128) and the k
chunk (32) make the code take another path."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import graph_embedding_cases as GC
import hyperbolicity_cases as HC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T, K = HC.TILE, HC.KCHUNK
SIZES = [1, 2, 3, K - 1, K + 1, T - 1, T, T + 1, 2 * T + 3]


def HY():
    from hyptokenizer_amd.embedding import hyperbolicity
    return hyperbolicity


@pytest.fixture(params=[1, 2], ids=["int32_path", "packed_path"])
def form(request):
    """Both paths of int16 input (hm_debug_gromov_form); the default is restored afterwards."""
    HY().set_kernel_form(request.param)
    yield request.param
    HY().set_kernel_form(0)


_CACHE = {}


def cached(key, make):
    """References are computed once and shared (both kernel paths compare with the same truth)."""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def bases_for(n, how):
    if how == "one":
        return [n // 2]
    if how == "three":
        return [(n - 1), 0, n // 3][:min(n, 3)]
    return list(range(n))


def check(D, bases):
    """gromov_delta of D (numpy) against the truth, bit for bit."""
    D = np.asarray(D)
    is_int = D.dtype != np.float32
    want_v, want_w = (HC.truth_i16 if is_int else HC.truth_f32)(D, range(D.shape[0]) if isinstance(bases, str) else bases)
    got = HY().gromov_delta(torch.from_numpy(D).to(DEV), bases)
    raw = got.per_base.cpu().numpy()
    assert raw.dtype == want_v.dtype
    assert np.array_equal(raw.view(np.uint32), want_v.view(np.uint32)), (raw, want_v)
    # the witness gromov_delta reports is that of the first maximising base
    at = int(np.argmax(want_v))
    assert got.witness == (*want_w[at].tolist(), int(got.base_positions[at]))
    assert got.delta == (float(want_v[at]) / 2 if is_int else float(want_v[at]))
    diam = float(HC.upper(D).max())
    assert got.diameter == diam and got.n == D.shape[0]
    assert (np.isnan(got.delta_rel) if diam == 0 else got.delta_rel == 2 * got.delta / diam)
    return got


def raw_call(d, bases):
    """The C entry point itself: (values, witnesses [n_base, 3]) as numpy."""
    from hyptokenizer_amd import _lib
    L = _lib.load()
    n, ld = d.shape[0], d.stride(0)
    is_int = d.dtype == torch.int16
    b = torch.tensor(bases, dtype=torch.int32, device=DEV)
    val = torch.full((len(bases),), 12345, dtype=torch.int32 if is_int else torch.float32, device=DEV)
    wit = torch.full((len(bases), 3), 12345, dtype=torch.int32, device=DEV)
    ws = torch.empty(max(1, L.hm_gromov_workspace_bytes(n, len(bases))), dtype=torch.uint8, device=DEV)
    fn = L.hm_gromov_delta_i16 if is_int else L.hm_gromov_delta_f32
    _lib.check(fn(C.c_void_p(d.data_ptr()), n, ld, C.c_void_p(b.data_ptr()), len(bases), C.c_void_p(val.data_ptr()),
                  C.c_void_p(wit.data_ptr()), C.c_void_p(ws.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return val.cpu().numpy(), wit.cpu().numpy()


def sparse_graph_metric(n, seed):
    """int16 [n, n] of a random connected sparse graph, through GraphPaths.distance_rows; checked against the host BFS."""
    from hyptokenizer_amd.graph_paths import GraphPaths
    _, edges = HC.random_connected(n, n // 4, seed)
    nodes = np.arange(n)
    d = GraphPaths((list(range(n)), edges), device=DEV).distance_rows(nodes, nodes)
    assert np.array_equal(d.cpu().numpy(), HC.bfs_all_pairs(n, edges))
    return d


def lorentz_distances(n, scale, seed=7):
    from hyptokenizer_amd.embedding import lorentz_model
    from hyptokenizer_amd.synthetic import lorentz_table
    x = lorentz_table(n, 6, seed=seed, scale=scale).to(DEV)
    return lorentz_model.batch_distance(x, x, 1.0, sign_convention="lorentz")


# ---- 1. exact equality with the truth ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_graph_metrics_equal_the_truth_int16(form, n):
    d = sparse_graph_metric(n, seed=n)
    D = d.cpu().numpy()
    for how in ("one", "three") + (("every",) if n <= K + 1 else ()):
        wv, ww = cached(("i16", n, how), lambda: HC.truth_i16(D, bases_for(n, how)))
        gv, gw = raw_call(d, bases_for(n, how))
        assert np.array_equal(gv, wv) and np.array_equal(gw, ww), (n, how, gv, wv, gw, ww)


@pytest.mark.parametrize("scale", [1e-3, 1.0])
@pytest.mark.parametrize("n", SIZES)
def test_table_distances_equal_the_truth_fp32(n, scale):
    d = lorentz_distances(n, scale)
    D = d.cpu().numpy()
    for how in ("one", "three") + (("every",) if n <= K + 1 else ()):
        wv, ww = cached(("f32", n, scale, how), lambda: HC.truth_f32(D, bases_for(n, how)))
        gv, gw = raw_call(d, bases_for(n, how))
        assert np.array_equal(gv.view(np.uint32), wv.view(np.uint32)) and np.array_equal(gw, ww), (n, how, gv, wv, gw, ww)


@pytest.mark.parametrize("name", sorted(HC.GRAPHS))
def test_named_graphs_all_bases(form, name):
    build, want = HC.GRAPHS[name]
    n, edges = build()
    D = HC.bfs_all_pairs(n, edges)
    got = check(D, "all")
    if want is not None:
        assert got.delta == want / 2
    got_f = check(D.astype(np.float32), "all")                   # small integers are exact in float32: the same delta
    assert got_f.delta == got.delta and got_f.witness == got.witness
    assert check(D.astype(np.int64), [0, n - 1]).per_base.dtype == torch.int32       # another integer type is converted


def test_all_bases_at_64_points_fp32():
    check(lorentz_distances(64, 0.3).cpu().numpy(), "all")


def test_top_of_the_u16_range(form):
    """A cycle of circumference 65534 sampled at 300 positions: D up to 32767, B up to 65534; a line of the same span: 0."""
    Dc = HC.cycle_metric(300)
    assert Dc.max() == 32767
    got = check(Dc, [0, 150, 299])
    assert got.delta > 0
    line = check(HC.line_metric(300), [0, 17, 299])
    assert line.delta == 0.0 and line.per_base.tolist() == [0, 0, 0] and line.diameter == 32767.0


def test_repeated_rows_exercise_the_tie_rule(form):
    """Points that coincide: zero distances off the diagonal and ties everywhere; the witness is the documented first one."""
    n, edges = HC.grid(3, 4)
    pick = np.array([0, 5, 5, 11, 0, 7, 5, 11, 2, 2, 9])
    D = HC.bfs_all_pairs(n, edges)[np.ix_(pick, pick)]
    check(D, "all")
    check(D.astype(np.float32), "all")
    x = lorentz_distances(40, 1.0).cpu().numpy()
    pick = np.arange(40) // 3                                     # triples of identical rows
    check(np.ascontiguousarray(x[np.ix_(pick, pick)]), [0, 1, 20, 39])
    assert check(np.zeros((7, 7), np.int16), "all").witness == (0, 0, 0, 0)


# ---- 2. the other promises ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.int16, torch.float32])
def test_a_base_outside_the_matrix_gets_minus_one(form, dtype):
    n = T + 5
    d = sparse_graph_metric(n, seed=2).to(dtype)
    D = d.cpu().numpy()
    truth = HC.truth_i16 if dtype == torch.int16 else HC.truth_f32
    wv, ww = truth(D, [3, n - 1])
    gv, gw = raw_call(d, [3, n, -1, n - 1, 1 << 30])
    assert gv[[1, 2, 4]].tolist() == [-1, -1, -1] and (gw[[1, 2, 4]] == -1).all()
    assert np.array_equal(gv[[0, 3]], wv) and np.array_equal(gw[[0, 3]], ww)


@pytest.mark.parametrize("dtype", [torch.int16, torch.float32])
def test_padded_leading_dimension_and_lower_triangle_is_not_read(form, dtype):
    n = T + 9
    d = sparse_graph_metric(n, seed=4).to(dtype)
    wide = torch.full((n, n + 13), 99, dtype=dtype, device=DEV)
    wide[:, 3:3 + n] = torch.triu(d) + torch.tril(torch.full_like(d, 55), -1)      # junk below the diagonal and around the block
    view = wide[:, 3:3 + n]
    assert view.stride(0) == n + 13 and not view.is_contiguous()
    truth = HC.truth_i16 if dtype == torch.int16 else HC.truth_f32
    wv, ww = truth(d.cpu().numpy(), [0, n - 1])
    got = HY().gromov_delta(view, [0, n - 1])
    assert np.array_equal(got.per_base.cpu().numpy(), wv)
    gv, gw = raw_call(view, [0, n - 1])
    assert np.array_equal(gv, wv) and np.array_equal(gw, ww)


def test_two_calls_are_byte_equal(form):
    for d in (sparse_graph_metric(2 * T + 3, seed=9), lorentz_distances(2 * T + 3, 1.0)):
        a, b = raw_call(d, [0, 100, 258]), raw_call(d, [0, 100, 258])
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_trees_return_exactly_zero(form):
    for n, edges in (HC.star(T + 2), HC.tree(2 * T + 3)):
        D = HC.bfs_all_pairs(n, edges)
        got = HY().gromov_delta(torch.from_numpy(D).to(DEV), [0, 1, n - 1])
        assert got.delta == 0.0 and got.per_base.tolist() == [0, 0, 0] and got.delta_rel == 0.0
        got = HY().gromov_delta(torch.from_numpy(D.astype(np.float32)).to(DEV), [0, 1, n - 1])
        assert got.delta == 0.0 and got.per_base.tolist() == [0.0, 0.0, 0.0]


def test_graph_hyperbolicity_keeps_the_largest_sampled_component():
    from hyptokenizer_amd.graph_paths import GraphPaths
    # nodes 0..11: C12; 12..19: C8; 20..22: a path; 23: alone
    e = np.concatenate([HC.cycle(12)[1], HC.cycle(8)[1] + 12, np.array([[20, 21], [21, 22]])])
    graph = (list(range(24)), e)
    got = HY().graph_hyperbolicity(graph, base_points="all")
    assert got.n_used == 12 and got.nodes_used.tolist() == list(range(12)) and got.delta == 3.0 and got.diameter == 6.0
    assert got.delta_rel == 1.0 and HY().curvature_estimate(got.delta_rel) == 0.144 ** 2
    paths = GraphPaths(graph, device=DEV)
    got = HY().graph_hyperbolicity(paths, nodes=list(range(8, 24)), base_points="all")     # 4 of C12 against all 8 of C8
    assert got.n_used == 8 and got.nodes_used.tolist() == list(range(12, 20)) and got.delta == 2.0
    got = HY().graph_hyperbolicity(paths, nodes=[0, 1, 2, 12, 13, 14, 23], base_points="all")   # a tie: the smallest label
    assert got.n_used == 3 and got.nodes_used.tolist() == [0, 1, 2] and got.delta == 0.0
    # a sample and drawn bases: what numpy's generator gives, and the truth on exactly those
    got = HY().graph_hyperbolicity(paths, num_samples=16, base_points=3, seed=5)
    rng = np.random.default_rng(5)
    sample = np.sort(rng.choice(24, size=16, replace=False))
    labels = np.where(sample < 12, 0, np.where(sample < 20, 12, np.where(sample < 23, 20, 23)))
    names, counts = np.unique(labels, return_counts=True)
    kept = sample[labels == names[np.argmax(counts)]]
    bases = np.sort(rng.choice(kept.size, size=3, replace=False))
    assert got.n_used == kept.size and got.nodes_used.tolist() == kept.tolist() and got.base_positions.tolist() == bases.tolist()
    D = HC.bfs_all_pairs(24, e)[np.ix_(kept, kept)]
    assert np.array_equal(got.per_base.cpu().numpy(), HC.truth_i16(D, bases)[0])


def test_embedding_hyperbolicity_drops_a_nan_row():
    from hyptokenizer_amd.embedding import lorentz_model
    from hyptokenizer_amd.synthetic import lorentz_table
    x = lorentz_table(50, 5, seed=3, scale=0.7).to(DEV)
    x[17, 2] = float("nan")
    x[40, 0] = float("inf")
    got = HY().embedding_hyperbolicity(x, base_points=[0, 5, 47], c=0.5)
    keep = [k for k in range(50) if k not in (17, 40)]
    assert got.n_used == 48 and got.nodes_used.tolist() == keep and got.n == 48
    rows = x[keep].contiguous()
    D = lorentz_model.batch_distance(rows, rows, 0.5, sign_convention="lorentz").cpu().numpy()
    wv, ww = HC.truth_f32(D, [0, 5, 47])
    assert np.array_equal(got.per_base.cpu().numpy().view(np.uint32), wv.view(np.uint32))
    at = int(np.argmax(wv))
    assert got.witness == (*ww[at].tolist(), [0, 5, 47][at]) and got.delta > 0


def test_cli_flag_writes_the_statistics(tmp_path):
    from hyptokenizer_amd.scripts.train_graph_embeddings import train_graph_embeddings
    n, edges = GC.tree_graph(63)
    path = tmp_path / "tree.tsv"
    path.write_text("".join(f"n{a}\tn{b}\n" for a, b in edges.tolist()))
    common = dict(dim=4, epochs=2, batch_size=32, num_negatives=5, lr=0.1, burn_in_epochs=0, seed=1, log_every=0)
    plain, with_flag = tmp_path / "plain", tmp_path / "flag"
    train_graph_embeddings(str(path), str(plain), **common)
    res = train_graph_embeddings(str(path), str(with_flag), eval_hyperbolicity=40, **common)
    assert sorted(os.listdir(plain)) == ["embeddings.pt", "nodes.json", "train_log.json"]
    assert sorted(os.listdir(with_flag)) == ["embeddings.pt", "hyperbolicity_stats.json", "nodes.json", "train_log.json"]
    for name in ("nodes.json", "train_log.json"):                                   # the existing outputs are untouched
        assert (plain / name).read_bytes() == (with_flag / name).read_bytes()
    assert torch.equal(torch.load(plain / "embeddings.pt"), torch.load(with_flag / "embeddings.pt"))
    stats = json.loads((with_flag / "hyperbolicity_stats.json").read_text())
    assert list(stats) == ["num_samples", "seed", "graph", "embedding"]
    g, t = stats["graph"], stats["embedding"]
    assert list(g) == list(t) == ["delta", "delta_rel", "diameter", "n_used", "curvature_estimate", "witness"]
    assert g["delta"] == 0 and g["delta_rel"] == 0 and g["curvature_estimate"] == "inf"      # a tree
    assert g["n_used"] == t["n_used"] == 40                                                  # one sample
    assert t["delta"] >= 0 and t["diameter"] > 0 and t["delta_rel"] == 2 * t["delta"] / t["diameter"]
    # the embedding side is the truth on the rows of the sampled nodes, at the bases the graph side drew
    from hyptokenizer_amd.embedding import lorentz_model
    rng = np.random.default_rng(1)
    sample = np.sort(rng.choice(63, size=40, replace=False))         # a tree is connected: every sampled node is kept
    bases = np.sort(rng.choice(40, size=8, replace=False))
    rows = res.table[[res.node_mapping[res.node_names[k]] for k in sample]].contiguous()
    D = lorentz_model.batch_distance(rows, rows, 1.0, sign_convention="lorentz").cpu().numpy()
    wv, ww = HC.truth_f32(D, bases)
    at = int(np.argmax(wv))
    assert t["delta"] == float(wv[at]) and t["witness"] == [*ww[at].tolist(), int(bases[at])]
    assert t["diameter"] == float(HC.upper(D).max())
    assert g["witness"] == [0, 0, 0, int(bases[0])]                # every base of a tree gives 0: the first base, the first triple
