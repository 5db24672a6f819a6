"""Entailment cones on the GPU (csrc/hm_cones.hip, hyptokenizer_amd.embedding.entailment_cones) against the float64 truth of
tests/cones_cases.py.

Bound of every comparison with the truth (the rule of test_gpu_autograd.py, set by the feature's specification, not tuned):
with e_ref the error of the same expression run by torch in fp32 on the CPU against the float64 truth and e_hip ours, both the
largest absolute error of an array relative to the array's largest magnitude, ``e_hip <= 4 * e_ref + 2**-20``.  Each case
prints ``name e_ref e_hip`` before it asserts (run with -s to collect the table of DESIGN.md 5.21).  Every case has at most
257 samples; the slots that sit on a kink of a hinge are masked out of the index beforehand (cones_cases.masked_index).
"""
import json
import os

import numpy as np
import pytest
import torch

import cones_cases as CC
import riemannian_cases as RC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILL = 777.0
K_AP = CC.APERTURE_K


def EC():
    from hyptokenizer_amd.embedding import entailment_cones
    return entailment_cones


def leaf(x: torch.Tensor, pad: int = 0) -> torch.Tensor:
    """A leaf on the device holding ``x``: contiguous, or a view with leading dimension ``x.shape[1] + pad`` over FILL."""
    if pad == 0:
        return x.to(DEV).clone().requires_grad_(True)
    buf = torch.full((x.shape[0], x.shape[1] + pad), FILL, device=DEV)
    buf[:, :x.shape[1]] = x.to(DEV)
    return buf[:, :x.shape[1]].detach().requires_grad_(True)


def hip_eval(x, idx, margin, apex, g, pad=0, sparse_grad=True, aperture_k=K_AP):
    """(loss [B], dense gradient [V, d1] of sum(g * loss)) through the Python layer, as numpy, and the raw gradient."""
    t = leaf(x, pad)
    loss = EC().entailment_cone_loss(t, idx.to(DEV), margin=margin, aperture_k=aperture_k, apex=apex, reduction="none",
                                     sparse_grad=sparse_grad, validate=False)
    (loss * g.to(DEV)).sum().backward()
    assert t.grad.is_sparse == sparse_grad
    dense = t.grad.to_dense() if sparse_grad else t.grad
    return (loss.detach().cpu().numpy(), dense.cpu().numpy()), t.grad


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(params=[0, 1], ids=["group_per_sample", "wave_per_sample"])
def form(request):
    """Both work decompositions of the loss kernels (hm_debug_cone_loss_form); the default, 1, is restored afterwards."""
    from hyptokenizer_amd import _lib
    L = _lib.load()
    _lib.check(L.hm_debug_cone_loss_form(request.param))
    yield request.param
    _lib.check(L.hm_debug_cone_loss_form(1))


# ---- 1. loss and gradient against the truth -----------------------------------------------------------------------------------
@pytest.mark.parametrize("apex", CC.ROLES)
@pytest.mark.parametrize("d1", CC.WIDTHS)
def test_loss_and_gradient_every_batch_negative_count_and_margin(d1, apex, form):
    failures = []
    for margin in CC.MARGINS:
        for b in CC.BATCHES:
            for k in CC.NEGATIVES:
                x, idx, g, _, _ = CC.case(d1, b, k, apex, margin)
                truth, ref32 = CC.reference(d1, b, k, apex, margin)
                ours, _ = hip_eval(x, idx, margin, apex, g)
                CC.compare(f"f{form}_{apex}_w{d1}_m{margin}_b{b}_k{k}", truth, ref32, ours, failures)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("apex", CC.ROLES)
@pytest.mark.parametrize("d1", CC.WIDTHS)
def test_padded_leading_dimensions(d1, apex, form):
    """Leading dimensions d1 + 1, + 2, + 3 (at least two of them no multiple of 4) over a fill value."""
    failures = []
    x, idx, g, _, _ = CC.case(d1, 37, 5, apex, 0.5)
    truth, ref32 = CC.reference(d1, 37, 5, apex, 0.5)
    for pad in (1, 2, 3):
        ours, _ = hip_eval(x, idx, 0.5, apex, g, pad=pad)
        CC.compare(f"f{form}_{apex}_w{d1}_ld{d1 + pad}", truth, ref32, ours, failures)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("apex", CC.ROLES)
def test_width_two_is_a_line(apex, form):
    """On a line every A is +-1 and clamped: ext is acos(A_MAX) (the child beyond the apex, seen from the origin) or
    acos(-A_MAX).  Apexes within the radius 2 K / S_MAX have the constant aperture asin(S_MAX) as well: their losses are the two
    clamp constants max(0, acos(+-A_MAX) - asin(S_MAX)) = 0 and 1.6136, and nothing has a gradient.  Further out the aperture
    varies and is the only thing that does: the truth decides."""
    t = torch.tensor([0.05, 0.1, 0.15, -0.05, -0.12, -0.18, 1.0, 2.0, -1.5, -0.7, 0.6, 3.0], dtype=torch.float64)
    x = torch.stack([torch.cosh(t), torch.sinh(t)], 1).float()
    near, rows = 6, len(t)                                      # rows 0..5: |sinh t| < 0.2002
    assert float(x[:near, 1].abs().max()) < 2 * K_AP / CC.S_MAX < float(x[near:, 1].abs().min())
    pairs = torch.tensor([(a, b) for a in range(rows) for b in range(rows) if a != b])
    inner = (pairs[:, 0] < near) if apex == "anchor" else (pairs[:, 1] < near)
    gen = torch.Generator().manual_seed(2)
    idx = torch.cat([pairs, torch.randint(0, rows, (len(pairs), 5), generator=gen)], 1)
    const = [0.0, float(np.arccos(-CC.A_MAX) - np.arcsin(CC.S_MAX))]
    # K = 0: the energies themselves
    (loss, dense), grad = hip_eval(x, pairs, 0.5, apex, torch.ones(len(pairs)))
    val = grad._values().reshape(len(pairs), 2, 2).cpu().numpy()
    d = np.abs(loss[inner.numpy(), None] - np.array(const)[None, :]).min(1)
    # acosf within 2 ulps of pi (2^-22 each), asinf within 2 ulps of 1.53 (2^-23 each), one rounding of the difference
    assert d.max() <= 2.0 ** -20 and (loss[inner.numpy()] > 1).any() and (loss[inner.numpy()] == 0).any()
    assert not val[inner.numpy()].any()
    for k, margin in ((0, 0.5), (5, 0.5), (5, 0.01)):
        index = idx[:, :2 + k]
        g = CC.upstream(len(pairs))
        truth, ref32 = (CC.evaluate(x, index, margin, K_AP, apex, g, dt) for dt in (torch.float64, torch.float32))
        ours, _ = hip_eval(x, index, margin, apex, g)
        # the fp32 reference does not know that it is on a line: where rounding leaves its |A| below A_MAX it is off by a clamp,
        # which only widens e_ref -- so the line is held to the floor of the bound alone
        for what, tr, o in zip(("loss", "grad"), truth, ours):
            e_hip, _ = CC.grad_error(o, o, tr)
            print(f"line_{apex}_k{k}_m{margin}:{what} e_hip={e_hip:.3e}")
            assert e_hip <= 4 * 2.0 ** -23 + CC.FLOOR


@pytest.mark.parametrize("apex", CC.ROLES)
@pytest.mark.parametrize("d1", [3, 17, 66])
def test_constructed_slots(d1, apex, form):
    """A child on its parent's own ray further out lies on the cone's axis: E = 0 and zero rows.  A parent inside the radius
    2 K / S_MAX has the constant aperture asin(S_MAX): its gradient comes from the exterior angle alone.  A partner that is the
    anchor is flat."""
    d = d1 - 1
    gen = torch.Generator().manual_seed(d1)
    e = torch.randn(d, generator=gen, dtype=torch.float64)
    e = e / e.norm()
    f = torch.randn(d, generator=gen, dtype=torch.float64)
    f = f - (f * e).sum() * e
    f = f / f.norm()
    x = CC.lift(torch.stack([0.7 * e, 2.5 * e, 0.1 * e, 0.9 * f - 0.8 * e, 1.5 * f - 0.2 * e])).float()
    swap = (lambda p, c: (p, c)) if apex == "anchor" else (lambda p, c: (c, p))
    # sample 0: (parent 0, child 1) on one ray; sample 1: parent 2 inside the clamp radius, child 3 behind it (the clamped
    # aperture is 87 degrees: only an exterior angle beyond that leaves an energy); sample 2: the
    # anchor as its own negative beside a real pair
    idx = torch.tensor([[*swap(0, 1), -1], [*swap(2, 3), -1], [*swap(4, 3), swap(4, 3)[0]]])
    margin = 0.5
    (loss, dense), grad = hip_eval(x, idx, margin, apex, torch.ones(3))
    val = grad._values().reshape(3, 3, d1).cpu().numpy()
    assert loss[0] == 0.0 and not val[0].any()
    t = CC.cone_terms(x.double(), idx, margin, K_AP, apex)
    assert bool(t["clamped_s"][1, 0]) and not bool(t["clamped_a"][1, 0]) and float(t["m"][1, 0]) > 0.1
    assert val[1, 0].any() and val[1, 1].any() and not val[1, 2].any()
    apex_row, child_row = (val[1, 0], val[1, 1]) if apex == "anchor" else (val[1, 1], val[1, 0])
    # with the aperture constant nu = q (-A / n): the apex's spatial row is alpha (-b_s) + (nu / n) a_s, checked through the truth
    truth, ref32 = (CC.evaluate(x, idx, margin, K_AP, apex, torch.ones(3), dt) for dt in (torch.float64, torch.float32))
    failures = []
    CC.compare(f"f{form}_{apex}_constructed_w{d1}", truth, ref32, (loss, dense), failures)
    assert not failures, "\n".join(failures)
    assert apex_row.any() and child_row.any()
    assert not val[2, 2].any() and abs(loss[2] - (float(t["E"][2, 0]) + np.float32(margin))) <= 4 * 2.0 ** -23 * max(loss[2], 1)
    coo = grad._indices().reshape(3, 3).cpu().numpy()
    assert coo[0].tolist() == [idx[0, 0], idx[0, 1], idx[0, 0]] and coo[2].tolist() == idx[2].tolist()


@pytest.mark.parametrize("reduction", ["mean", "sum", "none"])
def test_reductions_and_dense_gradient(reduction):
    d1, b, k, apex, margin = 17, 37, 5, "anchor", 0.5
    x, idx, _, _, _ = CC.case(d1, b, k, apex, margin)
    idx = idx.clone()
    idx[5, 1] = -1                                              # a skipped sample: "mean" divides by the live ones
    g = torch.ones(b) if reduction != "none" else CC.upstream(b)
    t64, t32 = (CC.evaluate(x, idx, margin, K_AP, apex, g, dt) for dt in (torch.float64, torch.float32))
    live = int(((idx[:, :2] >= 0) & (idx[:, :2] < CC.V)).all(1).sum())
    scale = 1.0 / live if reduction == "mean" else 1.0
    for sparse in (True, False):
        t = leaf(x)
        out = EC().entailment_cone_loss(t, idx.to(DEV), margin=margin, apex=apex, reduction=reduction, sparse_grad=sparse, validate=False)
        assert out.shape == ((b,) if reduction == "none" else ())
        (out * g.to(DEV)).sum().backward() if reduction == "none" else out.backward()
        dense = (t.grad.to_dense() if sparse else t.grad).cpu().numpy()
        assert t.grad.is_sparse == sparse
        failures = []
        want = [CC.reduce(a[0], idx, CC.V, reduction) for a in (t64, t32)]
        CC.compare(f"{reduction}_sparse{int(sparse)}", (want[0], t64[1] * scale), (want[1], t32[1] * scale),
                   (out.detach().cpu().numpy(), dense), failures)
        assert not failures, "\n".join(failures)
    with pytest.raises(ValueError):
        EC().entailment_cone_loss(leaf(x), idx.to(DEV))         # validate=True: the skipped sample is an error


# ---- 2. bits, masks, indices --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("apex", CC.ROLES)
def test_two_calls_are_bit_equal_and_coo_is_the_index(apex, form):
    d1, b, k, margin = 66, 257, 50, 0.5
    x, idx, g, _, _ = CC.case(d1, b, k, apex, margin)
    idx = idx.clone()
    idx[7, 0] = -1                                              # skipped samples: anchor or positive out of range
    idx[8, 1] = CC.V
    idx[9, 0] = 1 << 40
    (l1, _), g1 = hip_eval(x, idx, margin, apex, g)
    (l2, _), g2 = hip_eval(x, idx, margin, apex, g)
    assert np.array_equal(bits(l1), bits(l2))
    assert torch.equal(g1._values().view(torch.int32), g2._values().view(torch.int32)) and torch.equal(g1._indices(), g2._indices())
    assert g1._values().shape == (b * (2 + k), d1) and not g1.is_coalesced()
    coo = g1._indices().reshape(b, 2 + k).cpu().numpy()
    val = g1._values().reshape(b, 2 + k, d1).cpu().numpy()
    want = idx.numpy().copy()
    dead = (want < 0) | (want >= CC.V)
    skipped = dead[:, 0] | dead[:, 1]                           # samples 7..9 and those whose positive sat on a kink
    want = np.where(dead, want[:, :1], want)                    # a skipped slot names its anchor ...
    want[skipped] = 0                                           # ... and a skipped sample row 0
    assert skipped[7:10].all() and np.array_equal(coo, want)
    assert not val[dead].any() and not val[skipped].any() and not l1[skipped].any()
    assert np.isfinite(val).all() and val.any()


def test_the_two_forms_share_every_slot():
    """The forms differ in the order of the sums over the partners only: partner rows and COO indices are the same bits, losses
    and anchor rows agree to rounding."""
    from hyptokenizer_amd import _lib
    L = _lib.load()
    d1, b, k, margin = 66, 257, 50, 0.5
    for apex in CC.ROLES:
        x, idx, g, _, _ = CC.case(d1, b, k, apex, margin)
        out = []
        try:
            for f in (0, 1):
                _lib.check(L.hm_debug_cone_loss_form(f))
                (loss, _), grad = hip_eval(x, idx, margin, apex, g)
                out.append((loss, grad._values().reshape(b, 2 + k, d1).cpu().numpy(), grad._indices().cpu().numpy()))
        finally:
            _lib.check(L.hm_debug_cone_loss_form(1))
        (l0, v0, i0), (l1, v1, i1) = out
        assert np.array_equal(i0, i1) and np.array_equal(bits(v0[:, 1:]), bits(v1[:, 1:]))
        assert np.abs(l0 - l1).max() <= 8 * 2.0 ** -23 * np.abs(l0).max()
        assert np.abs(v0[:, 0] - v1[:, 0]).max() <= 2.0 ** -20 * np.abs(v0[:, 0]).max()
    assert L.hm_debug_cone_loss_form(2) == _lib.HM_E_ARG


def test_cone_energy_is_the_positive_term_by_bits():
    d1 = 17
    x = CC.ray_table(d1)
    ia, ib = np.nonzero(~np.eye(CC.V, dtype=bool))
    pa, pb = torch.from_numpy(ia).to(DEV), torch.from_numpy(ib).to(DEV)
    energy = EC().cone_energy(x.to(DEV), pa, pb, aperture_k=K_AP)
    assert energy.shape == (len(ia),) and not energy.requires_grad
    masked = torch.full_like(pa, -1)
    for apex, first, second in (("anchor", pa, pb), ("partner", pb, pa)):
        idx = torch.stack([first, second, masked, masked], 1)  # every negative skipped: the loss is E_0
        loss = EC().entailment_cone_loss(x.to(DEV), idx, margin=0.5, aperture_k=K_AP, apex=apex, reduction="none")
        assert torch.equal(loss.view(torch.int32), energy.view(torch.int32)), apex
    t = CC.cone_terms(x.double(), torch.from_numpy(np.stack([ia, ib], 1)), 0.5, K_AP, "anchor")
    far = (t["m"][:, 0].abs() > 2.0 ** -10).numpy()             # away from the kink the energies are the truth's
    got = energy.cpu().numpy().astype(np.float64)
    assert np.abs(got - t["E"][:, 0].numpy())[far].max() <= 1e-4 and (got[far] == 0).any() and (got[far] > 0).any()
    stats = EC().cone_stats(x.to(DEV), np.stack([ia, ib], 1), aperture_k=K_AP)
    assert stats["num_edges"] == len(ia) and stats["mean_energy"] == pytest.approx(float(energy.double().mean()), rel=1e-12)
    assert stats["reversed_mean_energy"] == pytest.approx(stats["mean_energy"], rel=1e-6)     # all ordered pairs: their own reverse
    assert 0 < stats["share_inside"] < 1


def test_graph_capture_replays_the_same_bits():
    d1, b, k, margin = 65, 37, 50, 0.5
    x, idx, g, _, _ = CC.case(d1, b, k, "partner", margin)
    (loss, _), grad = hip_eval(x, idx, margin, "partner", g)
    t = x.to(DEV).clone().requires_grad_(True)
    di, dg = idx.to(DEV), g.to(DEV)

    def step():
        out = EC().entailment_cone_loss(t, di, margin=margin, aperture_k=K_AP, apex="partner", reduction="none", validate=False)
        gr = torch.autograd.grad((out * dg).sum(), t)[0]
        return out, gr._values(), gr._indices()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                                  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, gv, gi = step()
    for _ in range(2):
        out.zero_()
        gv.zero_()
        gi.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(bits(out.detach().cpu().numpy()), bits(loss))
        assert np.array_equal(bits(gv.cpu().numpy()), bits(grad._values().cpu().numpy())) and torch.equal(gi, grad._indices())


# ---- 3. the optimiser takes the sparse gradient ------------------------------------------------------------------------------
def test_rsgd_step_on_the_sparse_gradient_stays_on_the_hyperboloid():
    from hyptokenizer_amd import optim
    d1, b, k = 17, 37, 5
    x, idx, _, _, _ = CC.case(d1, b, k, "anchor", 0.5)
    p = torch.nn.Parameter(x.to(DEV))
    opt = optim.RiemannianSGD([p], lr=0.01)
    loss = (EC().entailment_cone_loss(p, idx.to(DEV), margin=0.5, apex="anchor", reduction="sum", validate=False) +
            EC().entailment_cone_loss(p, idx[:, [1, 0] + list(range(2, 2 + k))].to(DEV), margin=0.5, apex="partner", reduction="sum",
                                      validate=False))
    loss.backward()
    assert p.grad.is_sparse
    opt.step()
    got = p.detach().double().cpu()
    moved = (bits(got.float().numpy()) != bits(x.numpy())).any(axis=1)
    assert moved.sum() >= 10
    assert float(((RC.ldot(got, got) + 1).abs() / got[:, 0] ** 2).max()) <= 1e-5


# ---- 4. end to end ---------------------------------------------------------------------------------------------------------------
def test_fit_graph_embedding_with_cones_on_the_closure_of_a_binary_tree():
    """The 258 (ancestor, descendant) pairs of the 63-node heap tree, dim 5, 150 epochs of 9 batches (CC.E2E).  The loss is the
    mean over the fixed batches of all pairs, parent side with the negatives of step 0 plus child side with those of step 1.
    The same loop in float64 on the CPU (cones_cases.e2e_loop_float64) takes it from 4.384298 to 0.928870 (F1 of "E <= 1e-3"
    as a classifier of the closure over all ordered pairs: 0 to 0.605).  Trajectories diverge by rounding, so only the size of
    the decrease is comparable: the GPU run must lose at least half of 3.455428, i.e. 1.727714."""
    from hyptokenizer_amd.embedding import fit_graph_embedding, graph_embedding
    n, edges = CC.tree_graph()
    graph = ([f"n{i}" for i in range(n)], edges)
    e = CC.E2E
    res = fit_graph_embedding(graph, e["dim"], epochs=e["epochs"], batch_size=e["batch_size"], num_negatives=e["num_negatives"],
                              lr=e["lr"], seed=e["seed"], init_scale=e["init_scale"], objective="cones", margin=e["margin"],
                              aperture_k=e["aperture_k"], closure=True, device=DEV)
    assert res.table.shape == (n, e["dim"] + 1) and res.node_names == graph[0]
    assert len(res.loss_history) == e["epochs"] and res.loss_history[-1] < res.loss_history[0]
    ev = CC.e2e_eval_indices()
    s = graph_embedding.NegativeSampler((graph[0], CC.e2e_pairs()), e["num_negatives"], seed=e["seed"], device=DEV)
    assert torch.equal(s.sample(ev[0][:, :2].contiguous().to(DEV), 0).cpu(), ev[0])
    assert torch.equal(s.sample(ev[1][:, :2].contiguous().to(DEV), 1).cpu(), ev[1])
    s.close()

    def mean_loss(table):
        kw = dict(margin=e["margin"], aperture_k=e["aperture_k"], reduction="none")
        return float((EC().entailment_cone_loss(table, ev[0].to(DEV), apex="anchor", **kw) +
                      EC().entailment_cone_loss(table, ev[1].to(DEV), apex="partner", **kw)).mean())

    before = mean_loss(graph_embedding.init_table(n, e["dim"], e["init_scale"], e["seed"], DEV))
    after = mean_loss(res.table)
    b64, a64 = CC.E2E_FLOAT64
    f1 = CC.e2e_f1(res.table.double().cpu())
    stats = EC().cone_stats(res.table, CC.e2e_pairs(), aperture_k=e["aperture_k"])
    print(f"e2e cones: loss {before:.6f} -> {after:.6f} (float64 {b64:.6f} -> {a64:.6f}), F1 {f1:.3f} (float64 {CC.E2E_FLOAT64_F1:.3f}), {stats}")
    assert abs(before - b64) <= 1e-4
    assert before - after >= 0.5 * (b64 - a64)
    assert stats["mean_energy"] < stats["reversed_mean_energy"] and stats["share_inside"] > stats["reversed_share_inside"]
    x = res.table.double().cpu()
    assert float(((RC.ldot(x, x) + 1).abs() / x[:, 0] ** 2).max()) <= 8 * 2.0 ** -24


def test_cli_objective_cones_writes_its_files(tmp_path):
    from hyptokenizer_amd.scripts.train_graph_embeddings import train_graph_embeddings
    n, edges = CC.tree_graph(15)
    path = tmp_path / "tree.tsv"
    path.write_text("".join(f"n{a}\tn{b}\n" for a, b in edges.tolist()))
    out = tmp_path / "cones"
    res = train_graph_embeddings(str(path), str(out), dim=4, epochs=3, batch_size=16, num_negatives=5, lr=0.003, burn_in_epochs=0,
                                 seed=1, init_scale=0.5, log_every=0, objective="cones", margin=0.5, closure=True, eval_cones=True)
    assert sorted(os.listdir(out)) == ["cone_stats.json", "embeddings.pt", "nodes.json", "train_log.json"]
    log = json.loads((out / "train_log.json").read_text())
    assert log["objective"] == "cones" and log["closure"] is True and log["margin"] == 0.5 and len(log["loss_history"]) == 3
    stats = json.loads((out / "cone_stats.json").read_text())
    assert stats["num_edges"] == n - 1 and set(stats["initial"]) == set(stats) - {"initial"}
    assert res.table.shape == (n, 5) and torch.equal(torch.load(out / "embeddings.pt"), res.table.cpu())
    plain = tmp_path / "plain"                                  # the default objective: the files and the log's keys it always had
    train_graph_embeddings(str(path), str(plain), dim=4, epochs=1, batch_size=16, num_negatives=5, lr=0.1, burn_in_epochs=0, seed=1,
                           log_every=0)
    assert sorted(os.listdir(plain)) == ["embeddings.pt", "nodes.json", "train_log.json"]
    assert "objective" not in json.loads((plain / "train_log.json").read_text())
