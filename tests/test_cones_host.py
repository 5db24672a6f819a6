"""Entailment cones, the part that needs no GPU: the truth of tests/cones_cases.py agrees with Ganea's ball form and with the
closed-form gradient of DESIGN.md 5.21, the seeded cases keep what they claim, the entry points exist and refuse bad arguments
before a device is touched, and the Python layer raises what it documents."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import cones_cases as CC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("hm_cone_loss_fwd", "hm_cone_loss_bwd", "hm_debug_cone_loss_form")


# ---- 1. the truth itself ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d1", [5, 17, 66])
def test_truth_is_ganeas_ball_form(d1):
    """All ordered pairs of the ray table: the Lorentz expressions against eqs. 26 and 28 on the ball, in float64, on the slots
    where neither A nor s is clamped (the paper has no clamp).  Both sides lose digits to the same cancellations, differently:
    the issue measured 5e-6 on tables of width 5 and more."""
    x = CC.ray_table(d1).double()
    ia, ib = np.nonzero(~np.eye(CC.V, dtype=bool))
    t = CC.cone_terms(x, torch.from_numpy(np.stack([ia, ib], 1)), 0.01, CC.APERTURE_K, "anchor")
    free = ~(t["clamped_a"] | t["clamped_s"] | t["flat"])[:, 0]
    ball = CC.ball_energy(x, torch.from_numpy(ia), torch.from_numpy(ib), CC.APERTURE_K)
    assert int(free.sum()) > 1000 and float((ball - t["E"][:, 0])[free].abs().max()) < 1e-5
    # the same pairs through apex="partner" with the columns swapped are the same numbers
    p = CC.cone_terms(x, torch.from_numpy(np.stack([ib, ia], 1)), 0.01, CC.APERTURE_K, "partner")
    assert float((p["E"] - t["E"]).abs().max()) < 1e-12


@pytest.mark.parametrize("apex", CC.ROLES)
@pytest.mark.parametrize("d1,b,k,margin", [(3, 37, 5, 0.5), (5, 257, 50, 0.01), (17, 37, 50, 0.5), (66, 3, 5, 0.5), (129, 257, 5, 0.5)])
def test_autograd_gradient_of_the_truth_is_the_closed_form(d1, b, k, margin, apex):
    x, idx, g, _, _ = CC.case(d1, b, k, apex, margin)
    truth, _ = CC.reference(d1, b, k, apex, margin)
    got = CC.closed_form_grad(x.double(), idx, margin, CC.APERTURE_K, apex, g).numpy()
    assert np.abs(truth[1]).max() > 0 and np.abs(got - truth[1]).max() < 1e-12 * max(np.abs(truth[1]).max(), 1.0)


def test_loss_rules():
    """Skipped slots and samples, the flat partner, the negative inside the cone, and the clamps as constants."""
    x = CC.ray_table(5).double()
    v = CC.V
    E = lambda a, b: float(CC.cone_terms(x, torch.tensor([[a, b]]), 0.5, 0.1, "anchor")["E"][0, 0])  # noqa: E731
    idx = torch.tensor([[0, 4, 8, 12], [0, 4, -1, 12], [0, 4, v, 12], [0, -1, 8, 12], [v, 4, 8, 12], [0, 4, 0, 12]])
    t = CC.cone_terms(x, idx, 0.5, 0.1, "anchor")
    hinge = lambda e: max(0.0, 0.5 - e)  # noqa: E731
    assert abs(float(t["loss"][0]) - (E(0, 4) + hinge(E(0, 8)) + hinge(E(0, 12)))) < 1e-12
    assert abs(float(t["loss"][1]) - (E(0, 4) + hinge(E(0, 12)))) < 1e-12 and float(t["loss"][2]) == float(t["loss"][1])
    assert float(t["loss"][3]) == 0.0 and float(t["loss"][4]) == 0.0 and t["ok"].tolist() == [True, True, True, False, False, True]
    assert abs(float(t["loss"][5]) - (E(0, 4) + 0.5 + hinge(E(0, 12)))) < 1e-12            # the anchor as its own negative: flat
    p = CC.cone_terms(x, idx[:1], 0.5, 0.1, "partner")
    assert abs(float(p["loss"][0]) - (E(4, 0) + hinge(E(8, 0)) + hinge(E(12, 0)))) < 1e-12
    # a parent inside the radius 2 K / S_MAX: the aperture is the constant asin(S_MAX)
    near = CC.lift(torch.tensor([[0.05, 0.0, 0.0, 0.0], [0.3, 0.4, 0.0, 0.0]], dtype=torch.float64))
    c = CC.cone_terms(near, torch.tensor([[0, 1]]), 0.5, 0.1, "anchor")
    assert bool(c["clamped_s"][0, 0]) and abs(float(c["m"][0, 0] + np.arcsin(CC.S_MAX) - torch.acos(c["A"][0, 0]))) < 1e-12
    assert CC.reduce(t["loss"].detach().numpy(), idx, v, "mean") == t["loss"].detach().numpy().sum() / 4


def all_cases():
    return [(d1, b, k, apex, margin) for d1 in CC.WIDTHS for b in CC.BATCHES for k in CC.NEGATIVES for apex in CC.ROLES
            for margin in CC.MARGINS]


@pytest.mark.parametrize("d1", CC.WIDTHS)
def test_cases_keep_the_mask_cap_and_exercise_both_sides_of_every_hinge(d1):
    """Every case of test_gpu_cones.py loses at most MASK_CAP of its live slots to the kink mask and has an fp32 reference within
    twice E_REF_CAP of the truth.  A batch of 257 has positives inside and outside their cones and, with 5 or more negatives, an active negative hinge (a batch of 1 has one positive and
    cannot have both; with margin 0.01 the window 0 < m < margin holds about 0.2 % of the slots, so only the large batches are
    asked)."""
    for (w, b, k, apex, margin) in all_cases():
        if w != d1:
            continue
        _, idx, _, masked, live = CC.case(w, b, k, apex, margin)
        assert masked <= CC.MASK_CAP * live, (w, b, k, apex, margin, masked, live)
        truth, ref32 = CC.reference(w, b, k, apex, margin)
        assert max(CC.grad_error(r, r, t)[0] for r, t in zip(ref32, truth)) <= 2 * CC.E_REF_CAP, (w, b, k, apex, margin)
        if b == 257:
            inside, outside, active = CC.case_counts(w, b, k, apex, margin)
            assert inside >= 1 and outside >= 1, (w, b, k, apex, margin)
            assert k < 5 or active >= 1, (w, b, k, apex, margin)


def test_fast_sampler_restatement_is_the_restatement():
    n, adj, p = 63, CC.e2e_adjacency(), CC.e2e_pairs()
    assert len(p) == 258 and adj.sum() == 516
    for pairs, step in ((p[:40], 0), (p[100:140, ::-1], 7)):
        want = CC.sample_reference(n, p, pairs, 10, CC.E2E["seed"], step)
        assert np.array_equal(CC.sample_fast(n, adj, pairs, 10, CC.E2E["seed"], step), want)
    x = CC.e2e_init().double()
    assert CC.e2e_mean_loss(x, CC.e2e_eval_indices()) == pytest.approx(CC.E2E_FLOAT64[0], rel=1e-9)


# ---- 2. the C ABI ------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_listed():
    from hyptokenizer_amd import _lib
    L = _lib.load()
    with open(os.path.join(ROOT, "include", "hypmerge.h")) as f:
        header = f.read()
    for name in SYMBOLS:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(L, name)
    assert L.hm_abi_version() == 3


def test_bad_arguments_are_refused_without_a_device():
    from hyptokenizer_amd import _lib
    L = _lib.load()
    E = _lib.HM_E_ARG
    P = C.c_void_p(4096)                                        # never dereferenced: every call below fails or has n == 0
    nan, inf = float("nan"), float("inf")

    def fwd(x=P, ld=11, v=100, d1=11, index=P, n=5, k=3, ap=0.1, mg=0.01, role=0, loss=P, w=P):
        return L.hm_cone_loss_fwd(x, ld, v, d1, index, n, k, ap, mg, role, loss, w, None)

    def bwd(x=P, ld=11, v=100, d1=11, index=P, n=5, k=3, ap=0.1, mg=0.01, role=0, w=P, g=P, val=P, coo=P):
        return L.hm_cone_loss_bwd(x, ld, v, d1, index, n, k, ap, mg, role, w, g, val, coo, None)

    for fn in (fwd, bwd):
        assert fn(x=None) == E and fn(index=None) == E and fn(w=None) == E and fn(w=C.c_void_p(4100)) == E
        assert fn(d1=1) == E and fn(d1=130, ld=130) == E and fn(ld=10) == E
        assert fn(n=-1) == E and fn(k=-1) == E and fn(v=-1) == E
        assert fn(ap=0.0) == E and fn(ap=-1.0) == E and fn(ap=nan) == E and fn(ap=inf) == E
        assert fn(mg=-0.5) == E and fn(mg=nan) == E and fn(mg=inf) == E
        assert fn(role=2) == E and fn(role=-1) == E
        assert fn(n=0) == _lib.HM_OK and fn(n=0, d1=2, ld=2, role=1, mg=0.0) == _lib.HM_OK and fn(n=0, d1=129, ld=200, k=0) == _lib.HM_OK
    assert fwd(loss=None) == E and bwd(g=None) == E and bwd(val=None) == E and bwd(coo=None) == E
    assert b"hm_cone_loss_bwd" in L.hm_last_error(None)
    assert L.hm_debug_cone_loss_form(-1) == E and L.hm_debug_cone_loss_form(2) == E and L.hm_debug_cone_loss_form(1) == _lib.HM_OK


# ---- 3. the Python layer -----------------------------------------------------------------------------------------------------
def test_python_layer_raises_what_it_documents():
    from hyptokenizer_amd.embedding import cone_energy, cone_stats, entailment_cone_loss, fit_graph_embedding
    from hyptokenizer_amd.engine import HypMergeUnavailable
    x, idx = CC.ray_table(5), CC.index_case(3, 5)
    for bad in (dict(table=x.double()), dict(index=idx.int()), dict(table=torch.zeros(4, 1)), dict(table=torch.zeros(4, 130)),
                dict(sign_convention="reference"), dict(index=idx[:, :1]), dict(index=idx.reshape(-1)), dict(reduction="max"),
                dict(apex="child"), dict(margin=-1.0), dict(margin=float("nan")), dict(aperture_k=0.0), dict(aperture_k=float("inf")),
                dict(table=torch.zeros(5, 8).t())):
        kw = dict(table=x, index=idx)
        kw.update(bad)
        with pytest.raises(ValueError):
            entailment_cone_loss(kw.pop("table"), kw.pop("index"), **kw)
    with pytest.raises(HypMergeUnavailable):
        entailment_cone_loss(x, idx)                            # valid arguments on the CPU: there is no fallback
    with pytest.raises(HypMergeUnavailable):
        entailment_cone_loss(x, idx, apex="partner", margin=0.5, reduction="none")
    with pytest.raises(ValueError):
        cone_energy(x, idx[:, 0], idx[:2, 1])
    with pytest.raises(ValueError):
        cone_energy(x, idx[:, 0], idx[:, 1], aperture_k=-0.1)
    with pytest.raises(HypMergeUnavailable):
        cone_energy(x, idx[:, 0], idx[:, 1])
    with pytest.raises(HypMergeUnavailable):
        cone_stats(x, [[0, 1], [1, 2]], aperture_k=0.1)
    graph = (list("abc"), np.array([[0, 1], [1, 2]]))
    with pytest.raises(ValueError):
        fit_graph_embedding(graph, 4, epochs=1, objective="bogus", device="cpu")
    with pytest.raises(HypMergeUnavailable):
        fit_graph_embedding(graph, 4, epochs=1, objective="cones", closure=True, device="cpu")


def test_transitive_closure():
    from hyptokenizer_amd.embedding import transitive_closure
    pairs = lambda a: [tuple(int(c) for c in r) for r in a]  # noqa: E731
    path = transitive_closure(5, [[i, i + 1] for i in range(4)])
    assert path.dtype == np.int64 and pairs(path) == [(i, j) for i in range(5) for j in range(i + 1, 5)]
    n, e = CC.tree_graph()
    tree = transitive_closure(n, e)
    assert tree.shape == (258, 2) and set(pairs(tree)) == CC.closure_reference(n, e) and np.array_equal(tree, CC.e2e_pairs())
    assert pairs(transitive_closure(4, [[0, 1], [0, 2], [1, 3], [2, 3], [0, 1]])) == [(0, 1), (0, 2), (0, 3), (1, 3), (2, 3)]    # a diamond, an edge twice
    cyc = transitive_closure(5, [[0, 1], [1, 2], [2, 0], [2, 3], [3, 3]])
    assert set(pairs(cyc)) == CC.closure_reference(5, [[0, 1], [1, 2], [2, 0], [2, 3], [3, 3]]) and len(cyc) == 9   # node 4 isolated, no self-pairs
    assert transitive_closure(3, np.zeros((0, 2), np.int64)).shape == (0, 2) and transitive_closure(0, []).shape == (0, 2)
    with pytest.raises(ValueError):
        transitive_closure(3, [[0, 3]])
