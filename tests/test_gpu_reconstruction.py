"""Graph reconstruction on the GPU (csrc/hm_recon.hip, hyptokenizer_amd.embedding.graph_metrics) against the truth of
tests/reconstruction_cases.py: the oracle's fp32 distance matrix and plain numpy comparisons.

The four count vectors are integers and must equal the truth exactly.  ``mean_rank`` is one float64 division of an exact
integer sum and must have the truth's bits.  ``map`` is a float64 sum of ``num_pairs`` positive terms (each a quotient of two
integers divided by a degree) divided by ``num_nodes``, against the truth's per-node means: the two differ by the order of a
float64 summation and by one more rounding per term, bounded by ``n_terms * 2^-52`` relative with
``n_terms = num_pairs + num_nodes`` -- a bound on rounding, not a measurement.
"""
import json
import os

import numpy as np
import pytest
import torch

import graph_embedding_cases as GC
import reconstruction_cases as RC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = ("anchors", "pivots", "less_all", "equal_all", "less_nb", "equal_nb")


def GM():
    from hyptokenizer_amd.embedding import graph_metrics
    return graph_metrics


@pytest.fixture(params=[1, 2], ids=["rows_in_lds", "anchor_in_registers"])
def layout(request):
    """Both tile layouts of the all-keys walk (hm_debug_recon_layout); the default is restored afterwards."""
    GM().set_walk_layout(request.param)
    yield request.param
    GM().set_walk_layout(0)


def dev_csr(row_ptr, col):
    return torch.from_numpy(row_ptr).to(DEV), torch.from_numpy(col).to(DEV)


def gpu_counts(x, row_ptr, col, nodes=None):
    """(the six slot vectors and the segments as numpy, the NeighborRankCounts) of the Python layer."""
    x = x if isinstance(x, torch.Tensor) else torch.from_numpy(x).to(DEV)
    rp, cl = dev_csr(row_ptr, col)
    c = GM().neighbor_rank_counts(x, rp, cl, None if nodes is None else torch.as_tensor(nodes, dtype=torch.int64).to(DEV))
    got = {k: getattr(c, k).cpu().numpy() for k in KEYS}
    got["segments"] = c.segments.cpu().numpy()
    return got, c


def check_counts(name, got, want):
    for k in KEYS + ("segments",):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (name, k)
        bad = np.flatnonzero(got[k] != want[k])
        assert bad.size == 0, f"{name}: {k} differs at {bad.size} slots, first {bad[:5]}: {got[k][bad[:5]]} != {want[k][bad[:5]]}"


def check_metrics(name, got, want):
    assert list(got) == ["mean_rank", "map", "num_pairs", "num_nodes"], name
    assert (got["num_pairs"], got["num_nodes"]) == (want["num_pairs"], want["num_nodes"]), name
    if want["num_pairs"] == 0:
        assert np.isnan(got["mean_rank"]) and np.isnan(got["map"]), name
        return
    assert np.float64(got["mean_rank"]).view(np.uint64) == np.float64(want["mean_rank"]).view(np.uint64), (name, got, want)
    n_terms = want["num_pairs"] + want["num_nodes"]
    assert abs(got["map"] - want["map"]) <= n_terms * 2.0 ** -52 * abs(want["map"]), (name, got, want)


# ---- 1. every size, width and graph kind against the truth ----------------------------------------------------------------------
@pytest.mark.parametrize("d1", RC.WIDTHS)
@pytest.mark.parametrize("v", RC.SIZES)
def test_counts_and_metrics_equal_the_truth(oracle, v, d1):
    """Default layout.  At V = 4097 the star is one 4096-slot segment over 64 blocks and the hub's row is read by 4096 slots;
    the sparse graph of V = 2 has no edge at all."""
    x = RC.table(v, d1)
    dist = RC.distances(oracle, x)
    xd = torch.from_numpy(x).to(DEV)
    for kind in RC.KINDS:
        row_ptr, col = RC.csr(kind, v)
        want = RC.truth_counts(dist, row_ptr, col)
        got, c = gpu_counts(xd, row_ptr, col)
        check_counts(f"{kind} V={v} d1={d1}", got, want)
        check_metrics(f"{kind} V={v} d1={d1}", GM().metrics_from_counts(c), RC.metrics(want))
        names = list(range(v))
        check_metrics(f"{kind} V={v} d1={d1} (graph)", GM().reconstruction_metrics(xd, (names, RC.graph(kind, v)[1])), RC.metrics(want))


# ---- 2. special inputs, both layouts --------------------------------------------------------------------------------------------
SPECIAL_V, SPECIAL_D1 = 130, 34


def special_table(what: str) -> np.ndarray:
    x = RC.table(SPECIAL_V, SPECIAL_D1, seed=1)
    if what == "duplicates":                                    # every row of the second half repeats one of the first 13 rows
        x[SPECIAL_V // 2:] = x[np.arange(SPECIAL_V - SPECIAL_V // 2) % 13]
    elif what == "nan":                                         # rows 0 (the star's hub, a tree root), 5 and 64 are NaN: anchors,
        x[[0, 5, 64]] = np.nan                                  # pivots of their neighbours and bystanders of everyone else
        x[7, 3] = np.nan                                        # and one row with a single NaN entry
    elif what == "off_hyperboloid":                             # -<x, y> < 1 for every pair: every u is clamped to 1, every distance 0
        x[:, 0] = 0.5
        x[:, 1:] *= 1e-2 / np.abs(x[:, 1:]).max()
    elif what == "mixed":                                       # a third of the rows off the hyperboloid, the rest as they were
        x[::3, 0] = 0.25
    else:
        raise ValueError(what)
    return x


@pytest.mark.parametrize("what", ["duplicates", "nan", "off_hyperboloid", "mixed"])
def test_ties_nan_and_clamped_rows(oracle, layout, what):
    x = special_table(what)
    dist = RC.distances(oracle, x)
    if what == "off_hyperboloid":
        assert (dist == 0).all()
    if what == "nan":
        assert np.isnan(dist[0]).all() and np.isnan(dist[:, 7]).all() and not np.isnan(dist[1, 2])
    for kind in RC.KINDS:
        row_ptr, col = RC.csr(kind, SPECIAL_V)
        want = RC.truth_counts(dist, row_ptr, col)
        got, c = gpu_counts(x, row_ptr, col)
        check_counts(f"{what} {kind}", got, want)
        check_metrics(f"{what} {kind}", GM().metrics_from_counts(c), RC.metrics(want))
    if what == "off_hyperboloid":                               # mass ties: everything equals the pivot, nothing is less
        assert (got["less_all"] == 0).all() and (got["equal_all"] == SPECIAL_V - 1).all() and (got["less_nb"] == 0).all()


@pytest.mark.parametrize("d1", [8, 34, 129])
def test_padded_leading_dimension_unaligned_base_and_node_subsets(oracle, layout, d1):
    v, pad = 130, 3
    x = RC.table(v, d1, seed=2)
    dist = RC.distances(oracle, x)
    flat = torch.full((v * (d1 + pad) + 1,), 777.0, device=DEV)
    view = flat[1:].view(v, d1 + pad)[:, :d1]                   # base 4 bytes off a 16-byte boundary, rows d1 + 3 floats apart
    view.copy_(torch.from_numpy(x))
    assert view.data_ptr() % 16 == 4 and view.stride(0) == d1 + pad
    rs = np.random.RandomState(d1)
    for kind in RC.KINDS:
        row_ptr, col = RC.csr(kind, v)
        got, _ = gpu_counts(view, row_ptr, col)
        check_counts(f"padded {kind} d1={d1}", got, RC.truth_counts(dist, row_ptr, col))
        for nodes in (rs.permutation(v)[:37], np.array([v - 1, 0]), np.array([v - 1]), rs.permutation(v)):
            got, c = gpu_counts(view, row_ptr, col, nodes)
            want = RC.truth_counts(dist, row_ptr, col, nodes)
            check_counts(f"subset {kind} d1={d1} n={nodes.size}", got, want)
            check_metrics(f"subset {kind} d1={d1} n={nodes.size}", GM().metrics_from_counts(c), RC.metrics(want))
            graph_metrics = GM().reconstruction_metrics(view, (list(range(v)), RC.graph(kind, v)[1]), nodes=nodes)
            check_metrics(f"subset (graph) {kind} d1={d1} n={nodes.size}", graph_metrics, RC.metrics(want))
    assert float(flat[0]) == 777.0 and bool((flat[1:].view(v, d1 + pad)[:, d1:] == 777.0).all())


@pytest.mark.parametrize("d1", [9, 33, 65, 66])
def test_both_layouts_in_every_column_class(oracle, layout, d1):
    """The narrowest rows of the register layout, the MAXN = 32 class at its upper end and both sides of the 64 / 128 boundary,
    every graph kind, and a node subset whose slots end inside a block."""
    v = 130
    x = RC.table(v, d1, seed=5)
    dist = RC.distances(oracle, x)
    xd = torch.from_numpy(x).to(DEV)
    nodes = np.random.RandomState(d1).permutation(v)[:37]
    for kind in RC.KINDS:
        row_ptr, col = RC.csr(kind, v)
        got, c = gpu_counts(xd, row_ptr, col)
        want = RC.truth_counts(dist, row_ptr, col)
        check_counts(f"{kind} d1={d1}", got, want)
        check_metrics(f"{kind} d1={d1}", GM().metrics_from_counts(c), RC.metrics(want))
        want = RC.truth_counts(dist, row_ptr, col, nodes)
        assert want["anchors"].size % 64 != 0
        check_counts(f"subset {kind} d1={d1}", gpu_counts(xd, row_ptr, col, nodes)[0], want)


def test_node_mapping_places_the_graph_in_a_larger_table(oracle):
    """The 63-node tree on rows 3 k + 1 of a 200-row table: the other rows are candidates in every ranking, never anchors."""
    n, edges = GC.tree_graph()
    x = RC.table(200, 9, seed=3)
    rows = 3 * np.arange(n) + 1
    names = [f"n{i}" for i in range(n)]
    row_ptr, col = RC.sorted_symmetric_csr(200, rows[edges])
    want = RC.truth_counts(RC.distances(oracle, x), row_ptr, col, rows)
    got = GM().reconstruction_metrics(torch.from_numpy(x).to(DEV), (names, edges), node_mapping={nm: int(r) for nm, r in zip(names, rows)})
    check_metrics("node_mapping", got, RC.metrics(want))
    assert got["num_pairs"] == 124 and got["num_nodes"] == 63


# ---- 3. determinism, coverage of the outputs, no edges --------------------------------------------------------------------------
def test_two_calls_are_byte_equal(layout):
    v, d1 = 1000, 33
    x = torch.from_numpy(RC.table(v, d1)).to(DEV)
    for kind in ("star", "sparse"):
        row_ptr, col = RC.csr(kind, v)
        a, ca = gpu_counts(x, row_ptr, col)
        b, cb = gpu_counts(x, row_ptr, col)
        for k in KEYS:
            assert a[k].tobytes() == b[k].tobytes(), (kind, k)
        ma, mb = GM().metrics_from_counts(ca), GM().metrics_from_counts(cb)
        assert np.array([ma["mean_rank"], ma["map"]]).tobytes() == np.array([mb["mean_rank"], mb["map"]]).tobytes()


@pytest.mark.parametrize("d1", [5, 65])
def test_every_output_element_is_written_and_nothing_else(oracle, layout, d1):
    """The C ABI on buffers filled with a pattern and 64 elements longer than the slots: every slot holds the truth afterwards
    (so it was written, and with one value: the pattern is no count and no u), the slack keeps the pattern."""
    from hyptokenizer_amd import _lib
    from hyptokenizer_amd.engine import _ptr, _stream_of
    L = _lib.load()
    v, slack, fill = 130, 64, 0x7B7B7B7B
    x = RC.table(v, d1, seed=4)
    row_ptr, col = RC.csr("sparse", v)
    want = RC.truth_counts(RC.distances(oracle, x), row_ptr, col)
    s = col.size
    xd = torch.from_numpy(x).to(DEV)
    rp, cl = dev_csr(row_ptr, col)
    ints = torch.full((7, s + slack), fill, dtype=torch.int32, device=DEV)
    u = torch.full((s + slack,), 777.0, device=DEV)
    _lib.check(L.hm_recon_slots(_ptr(rp), _ptr(cl), v, s, None, v, _ptr(rp), s, _ptr(ints[0]), _ptr(ints[1]), _ptr(ints[2]), _stream_of(xd)))
    _lib.check(L.hm_recon_counts(_ptr(xd), d1, v, d1, _ptr(ints[0]), _ptr(ints[1]), _ptr(ints[2]), _ptr(rp), s, v, _ptr(ints[3]),
                                 _ptr(ints[4]), _ptr(ints[5]), _ptr(ints[6]), _ptr(u), _stream_of(xd)))
    out = ints.cpu().numpy()
    assert (out[:, s:] == fill).all() and bool((u[s:] == 777.0).all())
    for row, k in zip((0, 1, 3, 4, 5, 6), KEYS):
        assert np.array_equal(out[row, :s], want[k]), k
    assert np.array_equal(out[2, :s], np.repeat(np.arange(v), np.diff(row_ptr)).astype(np.int32))
    uu = u[:s].cpu().numpy()
    assert (uu >= 1.0).all() and (uu != 777.0).all()
    # a slot that names a row outside the table is not dereferenced: -1 in all four vectors
    ints[0, 1] = v
    _lib.check(L.hm_recon_counts(_ptr(xd), d1, v, d1, _ptr(ints[0]), _ptr(ints[1]), _ptr(ints[2]), _ptr(rp), s, v, _ptr(ints[3]),
                                 _ptr(ints[4]), _ptr(ints[5]), _ptr(ints[6]), _ptr(u), _stream_of(xd)))
    assert ints[3:, 1].cpu().tolist() == [-1, -1, -1, -1] and ints[3:, 0].cpu().tolist()[0] == int(want["less_all"][0])


@pytest.mark.parametrize("d1", [33, 129])
def test_slots_outside_the_table_are_dead_and_their_neighbours_are_not(oracle, layout, d1):
    """The C ABI with anchors and pivots below 0 and at or past V, in the first and in the last (partial) block: those slots
    get -1, -1 and a NaN u and are never dereferenced; every other slot keeps its all-keys counts and the bits of its u."""
    from hyptokenizer_amd import _lib
    from hyptokenizer_amd.engine import _ptr, _stream_of
    L = _lib.load()
    v = 130
    x = RC.table(v, d1, seed=6)
    row_ptr, col = RC.csr("sparse", v)
    want = RC.truth_counts(RC.distances(oracle, x), row_ptr, col)
    s = col.size
    assert s > 128 and s % 64 != 0
    xd = torch.from_numpy(x).to(DEV)
    rp = torch.from_numpy(row_ptr).to(DEV)
    anchors, pivots = torch.from_numpy(want["anchors"]).to(DEV), torch.from_numpy(want["pivots"]).to(DEV)
    seg = torch.from_numpy(np.repeat(np.arange(v), np.diff(row_ptr)).astype(np.int32)).to(DEV)

    def run():
        ints = torch.full((4, s), 0x7B7B7B7B, dtype=torch.int32, device=DEV)
        u = torch.full((s,), 777.0, device=DEV)
        _lib.check(L.hm_recon_counts(_ptr(xd), d1, v, d1, _ptr(anchors), _ptr(pivots), _ptr(seg), _ptr(rp), s, v, _ptr(ints[0]),
                                     _ptr(ints[1]), _ptr(ints[2]), _ptr(ints[3]), _ptr(u), _stream_of(xd)))
        return ints.cpu().numpy(), u.cpu().numpy()

    clean, clean_u = run()
    assert np.array_equal(clean[0], want["less_all"]) and np.array_equal(clean[1], want["equal_all"])
    dead = {1: ("a", v), 5: ("p", -1), 63: ("a", -7), 64: ("p", v), 70: ("p", 2 ** 31 - 1), s - 1: ("a", v + 64)}
    for e, (which, value) in dead.items():
        (anchors if which == "a" else pivots)[e] = value
    out, u = run()
    at = np.array(sorted(dead))
    alive = np.setdiff1d(np.arange(s), at)
    assert (out[:, at] == -1).all() and np.isnan(u[at]).all()
    assert np.array_equal(out[:2, alive], clean[:2, alive]) and np.array_equal(u[alive].view(np.uint32), clean_u[alive].view(np.uint32))


def test_a_graph_without_edges_returns_nan():
    x = torch.from_numpy(RC.table(7, 5)).to(DEV)
    got = GM().reconstruction_metrics(x, (list(range(7)), np.zeros((0, 2), np.int64)))
    assert list(got) == ["mean_rank", "map", "num_pairs", "num_nodes"]
    assert np.isnan(got["mean_rank"]) and np.isnan(got["map"]) and got["num_pairs"] == 0 and got["num_nodes"] == 0
    got = GM().reconstruction_metrics(x, (list(range(7)), np.array([[3, 3]])))      # a self-loop is no edge
    assert np.isnan(got["mean_rank"]) and np.isnan(got["map"]) and got["num_pairs"] == 0
    got = GM().reconstruction_metrics(x, (list(range(7)), np.array([[0, 1]])), nodes=[2, 5])
    assert np.isnan(got["mean_rank"]) and got["num_pairs"] == 0 and got["num_nodes"] == 0


# ---- 4. memory -------------------------------------------------------------------------------------------------------------------
def test_peak_memory_is_proportional_to_the_slots():
    """V = 4097, d1 = 65, the tree (8192 slots): the peak above the inputs stays within 64 bytes per slot plus 2^20.  One V x V
    fp32 matrix would be 67 MB."""
    v, d1 = 4097, 65
    x = torch.from_numpy(RC.table(v, d1)).to(DEV)
    n, edges = RC.graph("tree", v)
    graph = (list(range(v)), edges)
    GM().reconstruction_metrics(x, graph)                      # the library and the allocator are warm
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    got = GM().reconstruction_metrics(x, graph)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    slots = got["num_pairs"]
    print(f"memory: {slots} slots, peak above the inputs {peak} bytes = {peak / slots:.1f} per slot (bound {64 * slots + 2 ** 20})")
    assert slots == 2 * (v - 1) and peak <= 64 * slots + 2 ** 20


# ---- 5. end to end -----------------------------------------------------------------------------------------------------------------
def test_fit_graph_embedding_reconstructs_the_tree(oracle):
    """The E2E recipe of graph_embedding_cases.  The GPU metrics of the initial and of the trained table equal the truth on
    those same tables; the float64 loop takes the truth from mean rank 33.44 / mAP 0.0569 (34.54 / 0.0601 under float64
    distances) to 1.048 / 0.985, and the GPU run must close at least half of that gap in both numbers (the rule
    test_fit_graph_embedding_on_a_binary_tree uses for the loss)."""
    from hyptokenizer_amd.embedding import graph_embedding as GE
    n, edges = GC.tree_graph()
    graph = ([f"n{i}" for i in range(n)], edges)
    e = GC.E2E
    res = GE.fit_graph_embedding(graph, e["dim"], epochs=e["epochs"], batch_size=e["batch_size"], num_negatives=e["num_negatives"],
                                 lr=e["lr"], seed=e["seed"], init_scale=e["init_scale"], device=DEV)
    first = GE.init_table(n, e["dim"], e["init_scale"], e["seed"], DEV)
    got = {}
    for name, t in (("initial", first), ("trained", res.table)):
        got[name] = GM().reconstruction_metrics(t, graph, node_mapping=res.node_mapping)
        want = RC.e2e_truth_metrics(oracle, t.cpu().numpy())
        print(f"e2e {name}: gpu {got[name]} truth {want}")
        check_metrics(f"e2e {name}", got[name], want)
    assert (got["initial"]["mean_rank"], got["initial"]["map"]) == pytest.approx(RC.E2E_RECON_TRUTH[0], rel=1e-9)
    for (r0, m0), (r1, m1) in ((RC.E2E_RECON_TRUTH[0], RC.E2E_RECON_TRUTH[1]), (RC.E2E_RECON_FLOAT64[0], RC.E2E_RECON_FLOAT64[1])):
        assert got["trained"]["mean_rank"] <= r0 - 0.5 * (r0 - r1)
        assert got["trained"]["map"] >= m0 + 0.5 * (m1 - m0)


def test_cli_flag_writes_the_statistics(tmp_path):
    from hyptokenizer_amd.scripts.train_graph_embeddings import train_graph_embeddings
    n, edges = GC.tree_graph(31)
    path = tmp_path / "tree.tsv"
    path.write_text("".join(f"n{a}\tn{b}\n" for a, b in edges.tolist()))
    common = dict(dim=4, epochs=3, batch_size=16, num_negatives=5, lr=0.1, burn_in_epochs=0, seed=1, log_every=0)
    plain, with_flag = tmp_path / "plain", tmp_path / "flag"
    train_graph_embeddings(str(path), str(plain), **common)
    res = train_graph_embeddings(str(path), str(with_flag), eval_reconstruction=True, **common)
    assert sorted(os.listdir(plain)) == ["embeddings.pt", "nodes.json", "train_log.json"]
    assert sorted(os.listdir(with_flag)) == ["embeddings.pt", "nodes.json", "reconstruction_stats.json", "train_log.json"]
    for name in ("embeddings.pt", "nodes.json", "train_log.json"):                  # the existing outputs are untouched
        a, b = (plain / name).read_bytes(), (with_flag / name).read_bytes()
        assert a == b or name == "embeddings.pt" and torch.equal(torch.load(plain / name), torch.load(with_flag / name))
    stats = json.loads((with_flag / "reconstruction_stats.json").read_text())
    assert list(stats) == ["mean_rank", "map", "num_pairs", "num_nodes", "initial"]
    assert list(stats["initial"]) == ["mean_rank", "map", "num_pairs", "num_nodes"]
    assert stats["num_pairs"] == stats["initial"]["num_pairs"] == 60 and stats["num_nodes"] == 31
    again = GM().reconstruction_metrics(res.table, (res.node_names, np.array([[res.node_mapping[f"n{a}"], res.node_mapping[f"n{b}"]]
                                                                             for a, b in edges.tolist()])))
    assert {k: stats[k] for k in again} == again
    assert 1.0 <= stats["mean_rank"] <= 30.0 and 0.0 < stats["map"] <= 1.0
