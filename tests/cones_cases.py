"""Entailment cones: the truth of the cone loss, its closed-form gradient, Ganea's ball form, the ray tables
and the masked seeded cases shared by test_cones_host.py (no GPU) and test_gpu_cones.py.

The truth of a case is the loss of DESIGN.md 5.21 written out in torch and evaluated on the CPU in float64, its gradient
taken by torch autograd; the place of a reference is taken by the same expression in float32 on the CPU, whose error against
the truth is e_ref.  The measure, ``FACTOR`` and ``FLOOR`` are those of tests/autograd_cases.py:
``e_hip <= FACTOR * e_ref + FLOOR``.

For an apex row a and a child row b (``apex="anchor"``: a the anchor, b the partner; ``"partner"``: the other way round)
    u = a0 b0 - sum_s a_s b_s,  n = sqrt(sum_s a_s^2),  w = sqrt(u^2 - 1),  A = (b0 - a0 u) / (n w)
    ext = acos(clamp(A, +-A_MAX)),  s = 2 K / n,  aper = asin(min(s, S_MAX)),  m = ext - aper,  E = max(0, m)
    loss_b = E_0 + sum_{k >= 1, live} max(0, margin - E_k)
A partner with the anchor's own index, with u <= 1, or whose apex sits at the origin (n = 0: no direction to open a cone
along) is flat: E = 0 and no gradient.  A clamped factor is a constant.  At width 2 (a line) every A is +-1 by geometry and
counts as clamped with the sign it has: ext is one of two constants there.

Hinges have kinks, and a slot that sits on one is decided by rounding.  ``masked_index`` therefore takes such slots out of
the index -- before the truth, the fp32 reference or the GPU see it -- by the float64 values of the unmasked index: a
negative becomes -1, a sample whose positive is such a slot gets positive -1 (and is skipped whole).  ``MASK_CAP`` bounds the
share of live slots a case may lose that way.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

from autograd_cases import FACTOR, FLOOR, grad_error  # noqa: F401  (re-exported)
from graph_embedding_cases import index_case, sample_reference, tree_graph, upstream  # noqa: F401
from riemannian_cases import ldot, lift, sgd_step  # noqa: F401

A_MAX = 1.0 - 2.0 ** -20
S_MAX = 1.0 - 2.0 ** -10
WIDTHS = (3, 5, 17, 65, 66, 129)                               # d1: both sides of the 16 / 32-lane switch, the scalar sum (d < 8)
BATCHES = (1, 3, 37, 257)
NEGATIVES = (0, 1, 5, 50)
ROLES = ("anchor", "partner")
MARGINS = (0.01, 0.5)
APERTURE_K = 0.1
V = 40
RADII = (0.5, 1.0, 2.0, 4.0)
TILT = 0.15
MASK_CAP = 0.01
#: seed of the ray table of every width: the first one under which every case of test_gpu_cones.py keeps the cap on masked slots
#: and an e_ref of at most E_REF_CAP (loss and gradient), every batch of 257 has positives inside and outside their cones and,
#: with 5 or more negatives, an active negative hinge (test_cones_host.py asserts all of it)
TABLE_SEEDS = {3: 53, 5: 0, 17: 4, 65: 1, 66: 2, 129: 6}
#: 1 / sqrt(1 - A^2) reaches 2^9.5 at the clamp: beyond this a table tests rounding luck.  The seeds were chosen at this cap; the
#: host test allows twice as much, because e_ref moves by some tens of per cent with the CPU that computes it
E_REF_CAP = 2e-3
KINK_M, KINK_E, KINK_A, KINK_S = 2.0 ** -10, 2.0 ** -10, 2.0 ** -18, 2.0 ** -10


def f32(v: float) -> float:
    return float(np.float32(v))


# ---- the loss ---------------------------------------------------------------------------------------------------------------
def cone_terms(x: torch.Tensor, index: torch.Tensor, margin: float, aperture_k: float, apex: str):
    """dict of the per-slot quantities [B, 1 + K] (m, E, A, s, flat, live, clamped_a, clamped_s, a0, b0, u, n), ``ok`` [B]
    and ``loss`` [B] of the table ``x`` in its own dtype; ``loss`` is differentiable in ``x``."""
    assert apex in ROLES
    v, dt = x.shape[0], x.dtype
    iu, part = index[:, 0], index[:, 1:]
    live = (part >= 0) & (part < v)
    ok = live[:, 0] & (iu >= 0) & (iu < v)
    live = live & ok[:, None]
    xu = x[iu.clamp(0, v - 1)][:, None, :]
    xk = x[part.clamp(0, v - 1)]
    a, b = (xu, xk) if apex == "anchor" else (xk, xu)
    one, zero = torch.ones((), dtype=dt), torch.zeros((), dtype=dt)
    u = -ldot(xu, xk)
    nn = (a[..., 1:] * a[..., 1:]).sum(-1).expand_as(u)
    flat = (part == iu[:, None]) | ~(u > 1) | ~(nn > 0)
    us = torch.where(flat, 2 * one, u)
    n = torch.sqrt(torch.where(nn > 0, nn, one))
    w = torch.sqrt(us * us - 1)
    a0, b0 = a[..., 0].expand_as(u), b[..., 0].expand_as(u)
    A = (b0 - a0 * us) / (n * w)
    ca = ~(A.abs() <= A_MAX)
    if x.shape[1] == 2:                                         # a line: every A is +-1, whatever fp32 rows that miss the hyperboloid make of it
        ca = torch.ones_like(ca)
    edge = torch.acos(torch.tensor(A_MAX, dtype=dt))
    ext = torch.where(ca, torch.where(A.detach() > 0, edge, torch.acos(torch.tensor(-A_MAX, dtype=dt))),
                      torch.acos(torch.where(ca, zero, A)))
    s = torch.tensor(2.0 * f32(aperture_k), dtype=dt) / n
    cs = ~(s < S_MAX)
    aper = torch.where(cs, torch.asin(torch.tensor(S_MAX, dtype=dt)), torch.asin(torch.where(cs, zero, s)))
    m = ext - aper
    E = torch.where(flat | ~(m > 0), zero, m)
    mg = torch.tensor(f32(margin), dtype=dt)
    hinge = torch.where(mg - E > 0, mg - E, zero)
    neg = torch.where(live[:, 1:], hinge[:, 1:], zero).sum(1)
    loss = torch.where(ok, E[:, 0] + neg, zero)
    return dict(loss=loss, ok=ok, live=live, flat=flat, m=m, E=E, A=A, s=s, clamped_a=ca, clamped_s=cs, a0=a0, b0=b0, u=us, n=n,
                margin=mg)


def closed_form_grad(x: torch.Tensor, index: torch.Tensor, margin: float, aperture_k: float, apex: str, g: torch.Tensor):
    """Dense gradient [V, d1] of sum(g * loss) from the closed form of DESIGN.md 5.21 (no autograd)."""
    with torch.no_grad():
        t = cone_terms(x, index, margin, aperture_k, apex)
        v, d1 = x.shape
        zero = torch.zeros((), dtype=x.dtype)
        A, u, n, a0, s = t["A"], t["u"], t["n"], t["a0"], t["s"]
        w = torch.sqrt(u * u - 1)
        q = torch.where(t["clamped_a"], zero, -1 / torch.sqrt(1 - torch.where(t["clamped_a"], zero, A) ** 2))
        alpha = q * (-a0 / (n * w) - A * u / (w * w))
        beta = q * (-u / (n * w))
        delta = q / (n * w)
        nu = q * (-A / n) + torch.where(t["clamped_s"], zero, s / (n * torch.sqrt(1 - torch.where(t["clamped_s"], zero, s) ** 2)))
        sigma = torch.zeros_like(A)
        sigma[:, 0] = (t["m"][:, 0] > 0).to(x.dtype)
        sigma[:, 1:] = -((t["m"][:, 1:] > 0) & (t["m"][:, 1:] < t["margin"])).to(x.dtype)
        sigma = torch.where(t["flat"] | ~t["live"], zero, sigma) * g.to(x.dtype)[:, None]
        iu, part = index[:, 0].clamp(0, v - 1), index[:, 1:].clamp(0, v - 1)
        xu, xk = x[iu][:, None, :].expand(-1, part.shape[1], -1), x[part]
        a, b = (xu, xk) if apex == "anchor" else (xk, xu)
        flip = torch.ones(d1, dtype=x.dtype)
        flip[1:] = -1
        e0 = torch.zeros(d1, dtype=x.dtype)
        e0[0] = 1
        sp = torch.ones(d1, dtype=x.dtype)
        sp[0] = 0
        ga = sigma[..., None] * (alpha[..., None] * b * flip + beta[..., None] * e0 + (nu / n)[..., None] * a * sp)
        gb = sigma[..., None] * (alpha[..., None] * a * flip + delta[..., None] * e0)
        gu, gk = (ga, gb) if apex == "anchor" else (gb, ga)
        out = torch.zeros_like(x)
        out.index_add_(0, iu, gu.sum(1))
        out.index_add_(0, part.reshape(-1), gk.reshape(-1, d1))
        return out


def ball_energy(x: torch.Tensor, ia: torch.Tensor, ib: torch.Tensor, aperture_k: float) -> torch.Tensor:
    """Ganea, Becigneul, Hofmann (ICML 2018), eqs. 26 and 28, on the ball points p = x_s / (1 + x0): max(0, Xi(a, b) - psi(a))."""
    p = x[:, 1:] / (1 + x[:, :1])
    a, b = p[ia], p[ib]
    ab, na2, nb2 = (a * b).sum(-1), (a * a).sum(-1), (b * b).sum(-1)
    na = torch.sqrt(na2)
    xi = torch.acos((ab * (1 + na2) - na2 * (1 + nb2)) / (na * torch.sqrt(((a - b) ** 2).sum(-1)) * torch.sqrt(1 + na2 * nb2 - 2 * ab)))
    psi = torch.asin(f32(aperture_k) * (1 - na2) / na)
    return torch.clamp(xi - psi, min=0)


def evaluate(table: torch.Tensor, index: torch.Tensor, margin: float, aperture_k: float, apex: str, g: torch.Tensor, dtype):
    """(loss [B], dense gradient [V, d1] of sum(g * loss)) as numpy, evaluated in ``dtype`` on the CPU by autograd."""
    x = table.to(dtype).clone().requires_grad_(True)
    loss = cone_terms(x, index, margin, aperture_k, apex)["loss"]
    (loss * g.to(dtype)).sum().backward()
    return loss.detach().numpy(), x.grad.numpy()


def reduce(loss: np.ndarray, index: torch.Tensor, v: int, reduction: str):
    if reduction == "none":
        return loss
    live = int((((index[:, :2] >= 0) & (index[:, :2] < v)).all(1)).sum())
    return loss.sum() if reduction == "sum" else loss.sum() / max(live, 1)


# ---- seeded inputs ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ray_table(d1: int, seed: int = -1, rows: int = V) -> torch.Tensor:
    """fp32 rows on the hyperboloid: row i lies on direction i % 4 of 4 random unit directions at spatial norm
    RADII[(i // 4) % 4], tilted off its ray by an angle drawn from N(0, TILT) towards a random normal; lifted in float64.

    With the random tables of graph_embedding_cases every exterior angle is near pi / 2 and no hinge of a negative is ever
    active; rows that share a ray at several radii put children inside cones, just outside them and far away."""
    gen = torch.Generator().manual_seed(7000 * d1 + (TABLE_SEEDS.get(d1, 0) if seed < 0 else seed))
    d = d1 - 1
    dirs = torch.randn(4, d, generator=gen, dtype=torch.float64)
    dirs = dirs / dirs.norm(dim=1, keepdim=True)
    e = dirs[torch.arange(rows) % 4]
    p = torch.randn(rows, d, generator=gen, dtype=torch.float64)
    p = p - (p * e).sum(1, keepdim=True) * e
    p = p / p.norm(dim=1, keepdim=True)
    theta = torch.randn(rows, 1, generator=gen, dtype=torch.float64) * TILT
    radius = torch.tensor([RADII[(i // 4) % 4] for i in range(rows)], dtype=torch.float64)[:, None]
    return lift(radius * (e * torch.cos(theta) + p * torch.sin(theta))).float()


def kink_slots(x64: torch.Tensor, index: torch.Tensor, margin: float, aperture_k: float, apex: str) -> torch.Tensor:
    """bool [B, 1 + K]: the live slots whose float64 value lies within reach of a kink or of a clamp."""
    with torch.no_grad():
        t = cone_terms(x64, index, margin, aperture_k, apex)
    near = (t["m"].abs() < KINK_M) | ((t["margin"] - t["E"]).abs() < KINK_E)
    near = near | ((t["A"].abs() - A_MAX).abs() < KINK_A) | ((t["s"] - S_MAX).abs() < KINK_S)
    return near & t["live"] & ~t["flat"]


def masked_index(x: torch.Tensor, index: torch.Tensor, margin: float, aperture_k: float, apex: str):
    """(index with the kink slots taken out, number of slots masked, number of live slots before)."""
    x64 = x.double()
    near = kink_slots(x64, index, margin, aperture_k, apex)
    with torch.no_grad():
        live = cone_terms(x64, index, margin, aperture_k, apex)["live"]
    out = index.clone()
    out[:, 1:][near] = -1
    return out, int(near.sum()), int(live.sum())


@functools.lru_cache(maxsize=None)
def case(d1: int, b: int, k: int, apex: str, margin: float, aperture_k: float = APERTURE_K):
    """(table, masked index, upstream, masked, live) of a seeded case."""
    x = ray_table(d1)
    idx, masked, live = masked_index(x, index_case(b, k), margin, aperture_k, apex)
    return x, idx, upstream(b), masked, live


@functools.lru_cache(maxsize=None)
def reference(d1: int, b: int, k: int, apex: str, margin: float, aperture_k: float = APERTURE_K):
    """((loss, grad) float64 truth, (loss, grad) fp32 on the CPU) of the seeded case with per-sample upstream weights."""
    x, idx, g, _, _ = case(d1, b, k, apex, margin, aperture_k)
    return evaluate(x, idx, margin, aperture_k, apex, g, torch.float64), evaluate(x, idx, margin, aperture_k, apex, g, torch.float32)


def case_counts(d1: int, b: int, k: int, apex: str, margin: float, aperture_k: float = APERTURE_K):
    """(positives inside their cone, positives outside, active negative hinges) of the masked case, in float64."""
    x, idx, _, _, _ = case(d1, b, k, apex, margin, aperture_k)
    with torch.no_grad():
        t = cone_terms(x.double(), idx, margin, aperture_k, apex)
    lp, ln = t["live"][:, 0] & ~t["flat"][:, 0], t["live"][:, 1:] & ~t["flat"][:, 1:]
    mp, mn = t["m"][:, 0], t["m"][:, 1:]
    return int((lp & (mp <= 0)).sum()), int((lp & (mp > 0)).sum()), int((ln & (mn > 0) & (mn < t["margin"])).sum())


def compare(name: str, truth, ref32, ours, failures: list) -> None:
    """Prints ``name e_ref e_hip`` for the arrays of the three tuples and appends what misses the bound to ``failures``."""
    for what, t, r, o in zip(("loss", "grad"), truth, ref32, ours):
        e_ref, _ = grad_error(r, r, t)
        e_hip, pattern_ok = grad_error(np.asarray(o).reshape(np.shape(r)), r, t)
        print(f"{name}:{what} e_ref={e_ref:.3e} e_hip={e_hip:.3e}")
        if not pattern_ok:
            failures.append(f"{name}:{what}: non-finite pattern differs from the fp32 reference's")
        elif not e_hip <= FACTOR * e_ref + FLOOR:
            failures.append(f"{name}:{what}: e_ref={e_ref:.3e} e_hip={e_hip:.3e}")


# ---- graphs -------------------------------------------------------------------------------------------------------------------
def closure_reference(n: int, edges) -> set:
    """{(ancestor, descendant)} of the directed graph by repeated squaring of the boolean adjacency matrix."""
    r = np.zeros((n, n), bool)
    for a, b in np.asarray(edges, dtype=np.int64).reshape(-1, 2):
        r[a, b] = True
    while True:
        r2 = r | ((r.astype(np.int64) @ r.astype(np.int64)) > 0)
        if np.array_equal(r2, r):
            break
        r = r2
    np.fill_diagonal(r, False)
    return {(int(a), int(b)) for a, b in zip(*np.nonzero(r))}


# ---- end to end: the closure of a balanced binary tree of 63 nodes in 5 dimensions ----------------------------------------------
E2E = dict(dim=5, epochs=150, batch_size=32, num_negatives=10, lr=0.003, seed=3, init_scale=0.5, margin=0.5, aperture_k=APERTURE_K)
E2E_CLASSIFY = 1e-3                                            # "u is above v" when E(u, v) <= this


def e2e_pairs() -> np.ndarray:
    """The 258 (ancestor, descendant) pairs of the heap tree, sorted by (ancestor, descendant)."""
    n, e = tree_graph()
    return np.array(sorted(closure_reference(n, e)), dtype=np.int64)


def sample_fast(n: int, adj: np.ndarray, pairs: np.ndarray, k: int, seed: int, step: int, max_tries: int = 32) -> np.ndarray:
    """graph_embedding_cases.sample_reference with the rejection test vectorised over a boolean adjacency matrix."""
    from graph_embedding_cases import philox4x32_10
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    b = pairs.shape[0]
    out = np.full((b, 2 + k), -1, np.int64)
    out[:, :2] = pairs
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    anchor = pairs[:, :1]
    for t in range(max_tries):
        r = philox4x32_10((np.arange(b, dtype=np.uint64)[:, None], np.arange(k, dtype=np.uint64)[None, :], np.uint64(t), np.uint64(step)), key)[0]
        cand = ((r * np.uint64(n)) >> np.uint64(32)).astype(np.int64)
        take = (out[:, 2:] < 0) & (cand != anchor) & ~adj[anchor, cand]
        out[:, 2:][take] = cand[take]
    return out


def e2e_adjacency() -> np.ndarray:
    n, _ = tree_graph()
    adj = np.zeros((n, n), bool)
    p = e2e_pairs()
    adj[p[:, 0], p[:, 1]] = adj[p[:, 1], p[:, 0]] = True
    return adj


def e2e_eval_indices():
    """The fixed evaluation batches: every closure pair in natural order with the negatives of step 0 (parent side) and, the
    pairs reversed, of step 1 (child side)."""
    n, _ = tree_graph()
    p, adj = e2e_pairs(), e2e_adjacency()
    return (torch.from_numpy(sample_fast(n, adj, p, E2E["num_negatives"], E2E["seed"], 0)),
            torch.from_numpy(sample_fast(n, adj, p[:, ::-1], E2E["num_negatives"], E2E["seed"], 1)))


def e2e_init() -> torch.Tensor:
    gen = torch.Generator().manual_seed(E2E["seed"])
    s = (torch.rand((63, E2E["dim"]), generator=gen, dtype=torch.float32) * 2.0 - 1.0) * E2E["init_scale"]
    return torch.cat([torch.sqrt(1.0 + (s * s).sum(-1, keepdim=True)), s], -1)


def e2e_mean_loss(x: torch.Tensor, ev) -> float:
    """Mean over the closure pairs of the parent-side plus the child-side loss."""
    with torch.no_grad():
        return float((cone_terms(x, ev[0], E2E["margin"], E2E["aperture_k"], "anchor")["loss"] +
                      cone_terms(x, ev[1], E2E["margin"], E2E["aperture_k"], "partner")["loss"]).mean())


def e2e_f1(x: torch.Tensor) -> float:
    """F1 of "E(u, v) <= E2E_CLASSIFY" as a classifier of the closure over all ordered pairs u != v."""
    n = x.shape[0]
    uu, vv = np.nonzero(~np.eye(n, dtype=bool))
    idx = torch.from_numpy(np.stack([uu, vv], 1))
    with torch.no_grad():
        E = cone_terms(x, idx, E2E["margin"], E2E["aperture_k"], "anchor")["E"][:, 0].numpy()
    truth = np.zeros((n, n), bool)
    p = e2e_pairs()
    truth[p[:, 0], p[:, 1]] = True
    said, is_ = E <= E2E_CLASSIFY, truth[uu, vv]
    tp = float((said & is_).sum())
    return 2 * tp / max(float(said.sum() + is_.sum()), 1.0)


@functools.lru_cache(maxsize=None)
def e2e_loop_float64():
    """``fit_graph_embedding(objective="cones", closure=True)``'s loop in float64 on the CPU (truth loss, sampler restatement,
    riemannian_cases.sgd_step) -> (evaluation loss before, after, F1 after)."""
    n, _ = tree_graph()
    positives, adj = e2e_pairs(), e2e_adjacency()
    x = e2e_init().double()
    ev = e2e_eval_indices()
    before = e2e_mean_loss(x, ev)
    gen = torch.Generator().manual_seed(E2E["seed"])
    step = 0
    for _ in range(E2E["epochs"]):
        order = torch.randperm(positives.shape[0], generator=gen).numpy()
        for b0 in range(0, positives.shape[0], E2E["batch_size"]):
            batch = positives[order[b0:b0 + E2E["batch_size"]]]
            ia = torch.from_numpy(sample_fast(n, adj, batch, E2E["num_negatives"], E2E["seed"], 2 * step))
            ip = torch.from_numpy(sample_fast(n, adj, batch[:, ::-1], E2E["num_negatives"], E2E["seed"], 2 * step + 1))
            xr = x.clone().requires_grad_(True)
            (cone_terms(xr, ia, E2E["margin"], E2E["aperture_k"], "anchor")["loss"].sum() +
             cone_terms(xr, ip, E2E["margin"], E2E["aperture_k"], "partner")["loss"].sum()).backward()
            x, _ = sgd_step(x, xr.grad, None, E2E["lr"])
            step += 1
    return before, e2e_mean_loss(x, ev), e2e_f1(x)


#: what e2e_loop_float64 returns for (before, after), recorded: the GPU run must lose at least half of the difference
E2E_FLOAT64 = (4.384298225137877, 0.9288700463954449)
#: and its F1 after training (e2e_f1; 0 before: no pair of the initial table lies inside a cone)
E2E_FLOAT64_F1 = 0.6054054054054054
