"""Graph embedding on the GPU (csrc/hm_edgeloss.hip, csrc/hm_negsample.hip, hyptokenizer_amd.embedding.graph_embedding)
against the float64 truth and the sampler restatement of tests/graph_embedding_cases.py.

Bound of every comparison with the truth (the rule of test_gpu_autograd.py, set by the feature's specification, not tuned):
with e_ref the error of the same expression run by torch in fp32 on the CPU against the float64 truth and e_hip ours, both the
largest absolute error of an array relative to the array's largest magnitude, ``e_hip <= 4 * e_ref + 2**-20``.  Each case
prints ``name e_ref e_hip`` before it asserts (run with -s to collect the table of DESIGN.md 5.17).  Every case has at most
257 samples.
"""
import numpy as np
import pytest
import torch

import graph_embedding_cases as GC
import riemannian_cases as RC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILL = 777.0


def GE():
    from hyptokenizer_amd.embedding import graph_embedding
    return graph_embedding


def leaf(x: torch.Tensor, pad: int = 0) -> torch.Tensor:
    """A leaf on the device holding ``x``: contiguous, or a view with leading dimension ``x.shape[1] + pad`` over FILL."""
    if pad == 0:
        return x.to(DEV).clone().requires_grad_(True)
    buf = torch.full((x.shape[0], x.shape[1] + pad), FILL, device=DEV)
    buf[:, :x.shape[1]] = x.to(DEV)
    return buf[:, :x.shape[1]].detach().requires_grad_(True)


def hip_eval(x, idx, c, g, pad=0, sparse_grad=True):
    """(loss [B], dense gradient [V, d1] of sum(g * loss)) through the Python layer, as numpy, and the raw gradient."""
    t = leaf(x, pad)
    loss = GE().edge_softmax_loss(t, idx.to(DEV), c, "none", sparse_grad=sparse_grad, validate=False)
    (loss * g.to(DEV)).sum().backward()
    assert t.grad.is_sparse == sparse_grad
    dense = t.grad.to_dense() if sparse_grad else t.grad
    return (loss.detach().cpu().numpy(), dense.cpu().numpy()), t.grad


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(params=[0, 1], ids=["group_per_sample", "wave_per_sample"])
def form(request):
    """Both work decompositions of the loss kernels (hm_debug_edge_loss_form); the default, 1, is restored afterwards."""
    from hyptokenizer_amd import _lib
    L = _lib.load()
    _lib.check(L.hm_debug_edge_loss_form(request.param))
    yield request.param
    _lib.check(L.hm_debug_edge_loss_form(1))


# ---- 1. loss and gradient against the truth -----------------------------------------------------------------------------------
@pytest.mark.parametrize("d1", GC.WIDTHS)
def test_loss_and_gradient_every_batch_and_negative_count(d1, form):
    failures = []
    for b in GC.BATCHES:
        for k in GC.NEGATIVES:
            truth, ref32 = GC.reference(d1, b, k)
            ours, _ = hip_eval(GC.table(d1), GC.index_case(b, k), 1.0, GC.upstream(b))
            GC.compare(f"f{form}_w{d1}_b{b}_k{k}", truth, ref32, ours, failures)
            if k == 0:                                          # the positive alone: d_0 - d_0, and no gradient
                assert float(np.abs(ours[0]).max()) <= 4 * 2.0 ** -21 and not ours[1].any()     # 4 ulps of a distance below 8
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("d1", GC.WIDTHS)
def test_loss_and_gradient_without_rows_near_the_origin(d1, form):
    """Rows of norm 1 and 6 only (graph_embedding_cases.table, "Conditioning"): e_ref is small and the bound tight."""
    failures = []
    for b, k, pad in ((3, 1, 0), (37, 5, 1), (37, 50, 0), (257, 50, 2)):
        truth, ref32 = GC.reference(d1, b, k, 1.0, GC.WELL)
        ours, _ = hip_eval(GC.table(d1, scales=GC.WELL), GC.index_case(b, k), 1.0, GC.upstream(b), pad=pad)
        GC.compare(f"f{form}_well_w{d1}_b{b}_k{k}", truth, ref32, ours, failures)
        assert d1 == 2 or GC.grad_error(ref32[1], ref32[1], truth[1])[0] < 1e-4      # what the cases claim (on a line, d1 = 2, 40 points do come close)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("d1", GC.WIDTHS)
def test_padded_leading_dimensions_and_curvature(d1, form):
    """Leading dimensions d1 + 1, + 2, + 3 (at least two of them no multiple of 4) and c != 1."""
    failures = []
    for pad, c in ((1, 1.0), (2, 0.5), (3, 2.0)):
        truth, ref32 = GC.reference(d1, 37, 5, c)
        ours, _ = hip_eval(GC.table(d1), GC.index_case(37, 5), c, GC.upstream(37), pad=pad)
        GC.compare(f"f{form}_w{d1}_ld{d1 + pad}_c{c}", truth, ref32, ours, failures)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("reduction", ["mean", "sum", "none"])
def test_reductions_and_dense_gradient(reduction):
    d1, b, k = 17, 37, 5
    x, idx = GC.table(d1), GC.index_case(b, k).clone()
    idx[5, 1] = -1                                              # a skipped sample: "mean" divides by the live ones
    g = torch.ones(b) if reduction != "none" else GC.upstream(b)
    t64, t32 = (GC.evaluate(x, idx, 1.0, g, dt) for dt in (torch.float64, torch.float32))
    live = int(((idx[:, :2] >= 0) & (idx[:, :2] < GC.V)).all(1).sum())
    scale = 1.0 / live if reduction == "mean" else 1.0
    assert live == b - 1
    for sparse in (True, False):
        t = leaf(x)
        out = GE().edge_softmax_loss(t, idx.to(DEV), 1.0, reduction, sparse_grad=sparse, validate=False)
        assert out.shape == ((b,) if reduction == "none" else ())
        (out * g.to(DEV)).sum().backward() if reduction == "none" else out.backward()
        dense = (t.grad.to_dense() if sparse else t.grad).cpu().numpy()
        assert t.grad.is_sparse == sparse
        failures = []
        want = [GC.reduce(a[0], idx, GC.V, reduction) for a in (t64, t32)]
        GC.compare(f"{reduction}_sparse{int(sparse)}", (want[0], t64[1] * scale), (want[1], t32[1] * scale),
                   (out.detach().cpu().numpy(), dense), failures)
        assert not failures, "\n".join(failures)
    with pytest.raises(ValueError):
        GE().edge_softmax_loss(leaf(x), idx.to(DEV))            # validate=True: the skipped sample is an error


# ---- 2. bits, masks, coincident rows ----------------------------------------------------------------------------------------
def test_d0_is_distance_bit_for_bit_at_every_width(form):
    """index (u, v, u): the anchor as its own negative is at distance exactly 0, the maximum of the shifted sum, so
    loss = d_0 + log(1 + exp(-d_0)); for d_0 > 25 log 2 the sum rounds to 1 and the loss IS d_0.  Rows of spatial norm 2e4
    are that far apart (d about 20).  The same pairs with the negative masked give a loss of exactly 0."""
    from hyptokenizer_amd.embedding import lorentz_model as lm
    compared = 0
    for d1 in range(2, 130):
        gen = torch.Generator().manual_seed(d1)
        x = RC.lift(torch.randn(16, d1 - 1, generator=gen, dtype=torch.float64) * (2e4 / np.sqrt(d1 - 1))).float().to(DEV)
        u, v = torch.arange(16, device=DEV), (torch.arange(16, device=DEV) + 1) % 16
        want = lm.distance(x[u], x[v], c=1.0, sign_convention="lorentz")
        got = GE().edge_softmax_loss(x, torch.stack([u, v, u], 1), 1.0, "none")
        far = want > 17.5
        compared += int(far.sum())
        assert torch.equal(got[far].view(torch.int32), want[far].view(torch.int32)), d1
        zero = GE().edge_softmax_loss(x, torch.stack([u, v, torch.full_like(u, -1)], 1), 1.0, "none")
        assert not zero.any(), d1
    assert compared > 128 * 8


def test_near_and_moderate_d0_follow_distance(form):
    """Where the sum does not round to 1 the loss is d_0 + log(1 + exp(-d_0)) of the SAME d_0: evaluated in float64 from the
    bits of ``distance`` it is met to 2 ulps of the loss (one rounding each of exp, the sum, log and the final sum)."""
    from hyptokenizer_amd.embedding import lorentz_model as lm
    for d1 in GC.WIDTHS:
        x = GC.table(d1).to(DEV)
        u, v = torch.arange(GC.V, device=DEV), (torch.arange(GC.V, device=DEV) + 1) % GC.V
        d0 = lm.distance(x[u], x[v], c=1.0, sign_convention="lorentz").double().cpu()
        want = (d0 + torch.log1p(torch.exp(-d0))).numpy()
        got = GE().edge_softmax_loss(x, torch.stack([u, v, u], 1), 1.0, "none").double().cpu().numpy()
        assert np.abs(got - want).max() <= 2 * 2.0 ** -23 * np.abs(want).max()


@pytest.mark.parametrize("d1", [2, 17, 66])
def test_coincident_rows_give_a_finite_loss_and_no_gradient(d1, form):
    """Rows whose u is exactly 1 in fp32: (5/4, 3/4, 0, ..) against its copy, the origin against its copy."""
    x = torch.zeros(5, d1)
    x[0, 0] = x[1, 0] = 1.25
    x[0, 1] = x[1, 1] = 0.75
    x[2, 0] = x[3, 0] = 1.0
    x[4] = RC.lift(torch.full((d1 - 1,), 0.5 / np.sqrt(d1 - 1), dtype=torch.float64)).float()
    idx = torch.tensor([[0, 1, 4], [2, 3, 3], [0, 4, 1]])
    t = leaf(x)
    loss = GE().edge_softmax_loss(t, idx.to(DEV), 1.0, "none")
    loss.sum().backward()
    val = t.grad._values().reshape(3, 3, d1).cpu().numpy()
    got = loss.detach().cpu().numpy()
    assert np.isfinite(got).all() and np.isfinite(val).all()
    assert abs(got[1] - np.log(2.0)) <= 2.0 ** -23             # two partners at distance 0
    assert not val[0, 1].any() and not val[1].any() and not val[2, 2].any()       # a_k = 0 exactly
    assert val[0, 2].any() and val[2, 1].any() and val[0, 0].any()
    truth, ref32 = (GC.evaluate(x, idx, 1.0, torch.ones(3), dt) for dt in (torch.float64, torch.float32))
    failures = []
    GC.compare(f"coincident_w{d1}", truth, ref32, (got, t.grad.to_dense().cpu().numpy()), failures)
    assert not failures, "\n".join(failures)


def test_masked_slots_and_skipped_samples(form):
    d1, b, k = 17, 37, 5
    x = GC.table(d1)
    gen = torch.Generator().manual_seed(9)
    idx = torch.randint(0, GC.V, (b, 2 + k), generator=gen)
    idx[:, 1] = (idx[:, 0] + 1) % GC.V
    short, short_grad = hip_eval(x, idx[:, :-1], 1.0, GC.upstream(b))
    masked = idx.clone()
    masked[0::2, -1] = -1
    masked[1::2, -1] = GC.V                                     # one past the end
    (loss, dense), grad = hip_eval(x, masked, 1.0, GC.upstream(b))
    # the last slot masked: the same operations in the same order as without the column -- the loss and every value row
    # bit for bit (the dense forms are sums in torch's order over different numbers of entries: equal under the measure only)
    val = grad._values().reshape(b, 2 + k, d1).cpu().numpy()
    assert np.array_equal(bits(loss), bits(short[0]))
    assert np.array_equal(bits(val[:, :-1]), bits(short_grad._values().reshape(b, 1 + k, d1).cpu().numpy()))
    assert np.abs(dense - short[1]).max() <= 2.0 ** -20 * np.abs(short[1]).max()
    coo = grad._indices().reshape(b, 2 + k).cpu().numpy()
    assert not val[:, -1].any() and np.array_equal(coo[:, -1], idx[:, 0].numpy()) and np.array_equal(coo[:, :-1], idx[:, :-1].numpy())
    # a slot masked in the middle: the sum runs over other lanes, the value is the truth's
    mid = idx.clone()
    mid[:, 3] = -1
    truth, ref32 = (GC.evaluate(x, mid, 1.0, GC.upstream(b), dt) for dt in (torch.float64, torch.float32))
    ours, _ = hip_eval(x, mid, 1.0, GC.upstream(b))
    failures = []
    GC.compare("masked_middle", truth, ref32, ours, failures)
    assert not failures, "\n".join(failures)
    # skipped samples: anchor or positive out of range
    skip = idx.clone()
    skip[3, 0] = -1
    skip[4, 1] = GC.V
    skip[5, 0] = 1 << 40
    (loss, dense), grad = hip_eval(x, skip, 1.0, GC.upstream(b))
    val = grad._values().reshape(b, 2 + k, d1).cpu().numpy()
    coo = grad._indices().reshape(b, 2 + k).cpu().numpy()
    assert not loss[3:6].any() and not val[3:6].any() and not coo[3:6].any()
    keep = np.r_[0:3, 6:b]
    t64, _ = GC.evaluate(x, skip, 1.0, GC.upstream(b), torch.float64)
    assert np.array_equal(bits(loss[keep]), bits(hip_eval(x, idx, 1.0, GC.upstream(b))[0][0][keep])) and not t64[3:6].any()


def test_two_calls_are_bit_equal(form):
    d1, b, k = 66, 257, 50
    x, idx, g = GC.table(d1), GC.index_case(b, k), GC.upstream(b)
    (l1, d1_), g1 = hip_eval(x, idx, 1.0, g)
    (l2, d2_), g2 = hip_eval(x, idx, 1.0, g)
    assert np.array_equal(bits(l1), bits(l2))
    assert torch.equal(g1._values().view(torch.int32), g2._values().view(torch.int32)) and torch.equal(g1._indices(), g2._indices())
    assert g1._values().shape == (b * (2 + k), d1) and not g1.is_coalesced()


def test_the_two_forms_share_every_u_and_differ_by_rounding_only():
    """Losses within 2 ulps of the largest (another order of the sum of exponentials), COO indices equal, zero value rows in
    the same places."""
    from hyptokenizer_amd import _lib
    L = _lib.load()
    d1, b, k = 66, 257, 50
    x, idx, g = GC.table(d1, scales=GC.WELL), GC.index_case(b, k), GC.upstream(b)
    out = []
    try:
        for f in (0, 1):
            _lib.check(L.hm_debug_edge_loss_form(f))
            (loss, dense), grad = hip_eval(x, idx, 1.0, g)
            out.append((loss, grad._values().cpu().numpy(), grad._indices().cpu().numpy()))
    finally:
        _lib.check(L.hm_debug_edge_loss_form(1))
    assert L.hm_debug_edge_loss_form(2) == _lib.HM_E_ARG
    (l0, v0, i0), (l1, v1, i1) = out
    assert np.abs(l0 - l1).max() <= 2 * 2.0 ** -23 * np.abs(l0).max() and np.array_equal(i0, i1)
    assert np.array_equal(v0.any(axis=1), v1.any(axis=1)) and np.abs(v0 - v1).max() <= 2.0 ** -20 * np.abs(v0).max()


# ---- 3. the optimisers take the sparse gradient ----------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", ["sgd", "adam"])
def test_optimiser_step_on_the_sparse_gradient(cls):
    from hyptokenizer_amd import optim
    d1, b, k, rows = 17, 37, 5, 64
    gen = torch.Generator().manual_seed(5)
    x = RC.lift(torch.randn(rows, d1 - 1, generator=gen, dtype=torch.float64) / np.sqrt(d1 - 1)).float()
    idx = torch.randint(0, 40, (b, 2 + k), generator=gen)      # rows 40.. are never named
    idx[:, 1] = (idx[:, 0] + 1) % 40
    idx[::4, 3] = -1
    p = torch.nn.Parameter(x.to(DEV))
    opt = optim.RiemannianSGD([p], lr=0.05) if cls == "sgd" else optim.RiemannianAdam([p], lr=0.05)
    GE().edge_softmax_loss(p, idx.to(DEV), 1.0, "sum").backward()
    assert p.grad.is_sparse
    opt.step()
    got = p.detach().cpu().numpy()
    named = np.unique(idx[idx >= 0].numpy())
    rest = np.setdiff1d(np.arange(rows), named)
    assert rest.size >= 24 and np.array_equal(bits(got[rest]), bits(x.numpy()[rest]))
    assert (bits(got[named]) != bits(x.numpy()[named])).any(axis=1).all()
    # the same step in fp32 on the CPU from the fp32 reference gradient: the bound of test_gpu_riemannian.py on <x, x> + 1
    _, g32 = GC.evaluate(x, idx, 1.0, torch.ones(b), torch.float32)
    g32 = torch.from_numpy(g32)
    if cls == "sgd":
        x32, _ = RC.sgd_step(x, g32, None, 0.05)
    else:
        x32, _, _ = RC.adam_step(x, g32, torch.zeros_like(x), torch.zeros(rows), 1, 0.05)
    form = lambda a: float(np.abs(-a[:, 0].astype(np.float64) ** 2 + (a[:, 1:].astype(np.float64) ** 2).sum(-1) + 1).max())  # noqa: E731
    print(f"step_{cls}: manifold e_ref={form(x32.numpy()[named]):.3e} e_hip={form(got[named]):.3e}")
    assert form(got[named]) <= RC.FACTOR * form(x32.numpy()[named]) + RC.FLOOR


# ---- 4. the sampler -------------------------------------------------------------------------------------------------------------
def sampler_pairs(n, edges, limit=70):
    """(anchor, neighbour) pairs, then every node paired with node 0 (isolated anchors included): a count that is no multiple
    of anything."""
    adj = GC.adjacency_sets(n, edges)
    pairs = [(a, b) for a in range(n) for b in sorted(adj[a])][:limit] + [(a, 0) for a in range(min(n, 7))] + [(n - 1, 0)]
    return np.array(pairs, dtype=np.int64)


@pytest.mark.parametrize("graph", ["path", "star", "complete", "random"])
@pytest.mark.parametrize("n", [1, 2, 63, 1000])
def test_sampler_equals_the_restatement(graph, n):
    if graph == "complete" and n == 1000:
        n = 200                                                 # 499 500 edges would only slow the restatement down
    n, edges = {"path": GC.path_graph, "star": GC.star_graph, "complete": GC.complete_graph, "random": GC.random_sparse_graph}[graph](n)
    pairs = sampler_pairs(n, edges)
    names = list(range(n))
    for k in (1, 50):
        s = GE().NegativeSampler((names, edges), k, seed=(0x9E3779B97F4A7C15 if k == 50 else 7), device=DEV)
        try:
            for step in (0, 7):
                got = s.sample(torch.from_numpy(pairs).to(DEV), step).cpu().numpy()
                want = GC.sample_reference(n, edges, pairs, k, s.seed, step)
                assert got.dtype == np.int64 and np.array_equal(got, want), (graph, n, k, step)
            if graph == "complete" or n == 1:
                assert (got[:, 2:] == -1).all()
        finally:
            s.close()


def test_sampler_takes_large_batches_and_bad_anchors():
    n, edges = GC.random_sparse_graph(1000, seed=1)
    rs = np.random.RandomState(2)
    pairs = rs.randint(0, n, (1031, 2)).astype(np.int64)        # several blocks, the last one partly filled
    pairs[5, 0] = -1
    pairs[6, 0] = n
    s = GE().NegativeSampler((list(range(n)), edges), 5, seed=1, device=DEV, max_tries=3)
    got = s.sample(torch.from_numpy(pairs).to(DEV), 2).cpu().numpy()
    assert np.array_equal(got, GC.sample_reference(n, edges, pairs, 5, 1, 2, max_tries=3))
    assert (got[5:7, 2:] == -1).all()
    with pytest.raises(ValueError):
        s.sample(torch.from_numpy(pairs).to(DEV).int(), 0)
    s.close()


# ---- 5. end to end ---------------------------------------------------------------------------------------------------------------
def test_fit_graph_embedding_on_a_binary_tree():
    """A balanced binary tree of 63 nodes, dim 5, 75 epochs of 4 batches (GC.E2E).  The loss is the mean over the fixed batch
    of all 124 directed edges with the negatives of step 0.  The same loop in float64 on the CPU (truth loss, sampler
    restatement, riemannian_cases.sgd_step; test_graph_embedding_host.py runs it and checks that it descends epoch by epoch)
    takes that loss from 2.397978 to 0.293686.  Trajectories diverge by rounding, so only the size of the decrease is
    comparable: the GPU run must lose at least half of 2.104292, i.e. 1.052146."""
    n, edges = GC.tree_graph()
    graph = ([f"n{i}" for i in range(n)], edges)
    e = GC.E2E
    res = GE().fit_graph_embedding(graph, e["dim"], epochs=e["epochs"], batch_size=e["batch_size"], num_negatives=e["num_negatives"],
                                   lr=e["lr"], seed=e["seed"], init_scale=e["init_scale"], device=DEV)
    assert res.table.shape == (n, e["dim"] + 1) and res.node_names == graph[0] and res.node_mapping["n5"] == 5
    assert len(res.loss_history) == e["epochs"] and res.loss_history[-1] < res.loss_history[0]
    ev = GC.e2e_eval_index()
    s = GE().NegativeSampler(graph, e["num_negatives"], seed=e["seed"], device=DEV)
    assert torch.equal(s.sample(ev[:, :2].contiguous().to(DEV), 0).cpu(), ev)
    s.close()
    before = float(GE().edge_softmax_loss(GE().init_table(n, e["dim"], e["init_scale"], e["seed"], DEV), ev.to(DEV)))
    after = float(GE().edge_softmax_loss(res.table, ev.to(DEV)))
    b64, a64 = GC.E2E_FLOAT64
    print(f"e2e: loss {before:.6f} -> {after:.6f} (float64 {b64:.6f} -> {a64:.6f})")
    assert abs(before - b64) <= 1e-4
    assert before - after >= 0.5 * (b64 - a64)
    # every row ends on the hyperboloid: the step recomputes x0 = sqrt(1 + |xs|^2) in fp32 -- the sum of 5 squares (4
    # roundings), the + 1 and the root (1 each) leave x0 with a relative error of at most 3.5 * 2^-24, x0^2 with twice that
    x = res.table.double().cpu()
    assert float(((RC.ldot(x, x) + 1).abs() / x[:, 0] ** 2).max()) <= 8 * 2.0 ** -24
