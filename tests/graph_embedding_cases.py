"""Graph embedding: the truth of the edge-softmax loss, the numpy restatement of the negative sampler and
the seeded cases shared by test_graph_embedding_host.py (no GPU) and test_gpu_graph_embedding.py.

The truth of a case is the loss written out in torch and evaluated on the CPU in float64, its gradient taken by torch
autograd; the place of a reference is taken by the same expression in float32 on the CPU, whose error against the truth is
e_ref.  The measure, ``FACTOR`` and ``FLOOR`` are those of tests/autograd_cases.py: ``e_hip <= FACTOR * e_ref + FLOOR``.

The rule at u <= 1.  With u = -<x_u, x_k> the distance is acosh(max(u, 1)) / sqrt(c); where u <= 1 the slot's distance is
the constant 0 (zero gradient), and a partner that is the anchor itself (same index) has u = 1 by definition, whatever
rounding makes of -<x, x>.  ``loss_terms`` applies both before autograd sees the expression.

The sampler restatement is written from the published algorithm (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as
easy as 1, 2, 3", SC 2011; Philox4x32-10, multipliers 0xD2511F53 / 0xCD9E8D57, Weyl key increments 0x9E3779B9 /
0xBB67AE85) and checked against the known-answer vectors distributed with it.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

from autograd_cases import FACTOR, FLOOR, grad_error  # noqa: F401  (re-exported)
from riemannian_cases import ldot, lift, sgd_step  # noqa: F401

WIDTHS = (2, 5, 17, 65, 66, 129)                               # d1: both sides of the 16 / 32-lane switch
BATCHES = (1, 3, 37, 257)                                      # partly filled group, partly filled wave, several blocks
NEGATIVES = (0, 1, 5, 50)                                      # no negative, one, fewer than a group, more than a group of 16 and of 32
SCALES = (1e-3, 1.0, 6.0)                                      # spatial norm of row i is about SCALES[i % 3]
WELL = (1.0, 6.0)                                              # the well-conditioned tables: no pair of rows near the origin
V = 40                                                         # rows of the seeded tables


# ---- the loss ---------------------------------------------------------------------------------------------------------------
def loss_terms(x: torch.Tensor, index: torch.Tensor, c: float):
    """(loss [B], a [B, 1 + K], ok [B], live [B, 1 + K]) of the table ``x`` in its own dtype; differentiable in ``x``.
    ``a`` is the closed-form coefficient of the gradient (detached)."""
    v = x.shape[0]
    iu, part = index[:, 0], index[:, 1:]
    live = (part >= 0) & (part < v)
    ok = live[:, 0] & (iu >= 0) & (iu < v)
    live = live & ok[:, None]
    xu = x[iu.clamp(0, v - 1)]
    xk = x[part.clamp(0, v - 1)]
    one, zero = torch.ones((), dtype=x.dtype), torch.zeros((), dtype=x.dtype)
    sqrt_c = torch.sqrt(torch.tensor(float(np.float32(c)), dtype=x.dtype))
    u = -ldot(xu[:, None, :], xk)
    u = torch.where(part == iu[:, None], one, u)
    flat = ~(u > 1)
    d = torch.where(flat, zero, torch.acosh(torch.where(flat, 2 * one, u))) / sqrt_c
    neg = torch.where(live, -d, torch.full((), -float("inf"), dtype=x.dtype))
    neg = torch.where(ok[:, None], neg, zero)                   # a skipped sample: any finite row, its loss is replaced below
    loss = torch.where(ok, d[:, 0] + torch.logsumexp(neg, dim=1), zero)
    with torch.no_grad():
        p = torch.softmax(neg, dim=1)
        first = torch.zeros_like(p)
        first[:, 0] = 1
        den = sqrt_c * torch.sqrt(torch.where(flat, 2 * one, u) ** 2 - 1)
        a = torch.where(flat | ~live, zero, (first - p) / den)
    return loss, a, ok, live


def closed_form_grad(x: torch.Tensor, index: torch.Tensor, a: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    """Dense gradient [V, d1] from the coefficients: anchor += g a_k (-J x_k), partner k += g a_k (-J x_u), J = diag(-1, 1, ..)."""
    v = x.shape[0]
    iu, part = index[:, 0].clamp(0, v - 1), index[:, 1:].clamp(0, v - 1)
    flip = torch.ones(x.shape[1], dtype=x.dtype)
    flip[1:] = -1                                               # -J x = (x0, -xs)
    w = (a * g[:, None]).unsqueeze(-1)
    out = torch.zeros_like(x)
    out.index_add_(0, iu, (w * (x[part] * flip)).sum(1))
    out.index_add_(0, part.reshape(-1), (w * (x[iu] * flip)[:, None, :]).reshape(-1, x.shape[1]))
    return out


def evaluate(table: torch.Tensor, index: torch.Tensor, c: float, g: torch.Tensor, dtype):
    """(loss [B], dense gradient [V, d1] of sum(g * loss)) as numpy, evaluated in ``dtype`` on the CPU by autograd."""
    x = table.to(dtype).clone().requires_grad_(True)
    loss, _, _, _ = loss_terms(x, index, c)
    (loss * g.to(dtype)).sum().backward()
    return loss.detach().numpy(), x.grad.numpy()


def reduce(loss: np.ndarray, index: torch.Tensor, v: int, reduction: str):
    if reduction == "none":
        return loss
    live = int((((index[:, :2] >= 0) & (index[:, :2] < v)).all(1)).sum())
    return loss.sum() if reduction == "sum" else loss.sum() / max(live, 1)


# ---- seeded inputs ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def table(d1: int, seed: int = 0, rows: int = V, scales=SCALES) -> torch.Tensor:
    """fp32 rows on the hyperboloid; row i has spatial norm about scales[i % len(scales)].

    Conditioning.  Two rows of norm 1e-3 have u - 1 of about 1e-6, eight ulps of u: d_k and 1 / sqrt(u^2 - 1) of such a pair
    carry a relative error of several per cent in ANY fp32 evaluation, and since a_k is about 700 there, that one slot sets
    the largest gradient entry and e_ref of the whole array (up to 1 at d1 = 2).  The bound is then wide, and meaningful
    only because the kernel's u has the bits of the reference's.  ``WELL = (1, 6)`` leaves those rows out: e_ref is then of
    the order of 1e-6 and the bound tests the arithmetic of every slot."""
    gen = torch.Generator().manual_seed(1000 * d1 + seed)
    d = d1 - 1
    scale = torch.tensor([scales[i % len(scales)] for i in range(rows)], dtype=torch.float64)[:, None]
    return lift(torch.randn(rows, d, generator=gen, dtype=torch.float64) * (scale / np.sqrt(d))).float()


@functools.lru_cache(maxsize=None)
def index_case(b: int, k: int, seed: int = 0, rows: int = V) -> torch.Tensor:
    """int64 [b, 2 + k] with, where the shape has room for them: repeated negatives within a sample, a negative equal to the
    positive, a negative equal to the anchor, -1 slots, a fully masked negative set, and a row that is the anchor of one sample
    and a partner in another.  Anchors and positives are in range and differ."""
    gen = torch.Generator().manual_seed(77 * b + 13 * k + seed)
    idx = torch.randint(0, rows, (b, 2 + k), generator=gen, dtype=torch.int64)
    idx[:, 1] = (idx[:, 0] + 1 + torch.randint(0, rows - 1, (b,), generator=gen)) % rows
    if k >= 1:
        idx[0, 2] = idx[0, 1]                                   # negative == positive
        if b >= 2:
            idx[1, 2] = idx[1, 0]                               # negative == anchor: u <= 1
            idx[1, 1] = idx[0, 0]                               # the anchor of sample 0 is the positive of sample 1
        if b >= 3:
            idx[2, 2:] = -1                                     # every negative masked
        if b >= 4:
            idx[3::5, 2] = -1
    if k >= 2:
        idx[0, 3] = idx[0, 2]                                   # repeated negatives
        if b >= 5:
            idx[4, 3] = idx[4, 2] = idx[4, 1 + k]
    if k >= 5:
        idx[::3, 4] = -1
    return idx


@functools.lru_cache(maxsize=None)
def upstream(b: int, seed: int = 0) -> torch.Tensor:
    gen = torch.Generator().manual_seed(5 * b + seed)
    return (0.5 + torch.rand(b, generator=gen, dtype=torch.float64)).float()


@functools.lru_cache(maxsize=None)
def reference(d1: int, b: int, k: int, c: float = 1.0, scales=SCALES):
    """((loss, grad) float64 truth, (loss, grad) fp32 on the CPU) of the seeded case with per-sample upstream weights."""
    x, idx, g = table(d1, scales=scales), index_case(b, k), upstream(b)
    return evaluate(x, idx, c, g, torch.float64), evaluate(x, idx, c, g, torch.float32)


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


# ---- the sampler ------------------------------------------------------------------------------------------------------------
M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """Philox4x32-10: ``ctr`` four and ``key`` two arrays (or scalars) of 32-bit words -> the four output words (uint64 arrays
    holding 32-bit values)."""
    c = [np.asarray(w, dtype=np.uint64) & M32 for w in ctr]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = (np.asarray(w, dtype=np.uint64) & M32 for w in key)
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    for _ in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]                           # 32 x 32 -> 64 bits, exact in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & M32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return c


def adjacency_sets(n: int, edges) -> list:
    adj = [set() for _ in range(n)]
    for a, b in np.asarray(edges, dtype=np.int64).reshape(-1, 2):
        adj[int(a)].add(int(b))
        adj[int(b)].add(int(a))
    return adj


def sample_reference(n: int, edges, pairs, k: int, seed: int, step: int, max_tries: int = 32, rows=None) -> np.ndarray:
    """int64 [B, 2 + k]: what ``NegativeSampler(graph, k, seed, max_tries=max_tries).sample(pairs, step)`` must return.
    ``rows`` (optional): the sample numbers b of the pairs, when they are not 0 .. B - 1 (batch-order invariance)."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    b = pairs.shape[0]
    rows = np.arange(b, dtype=np.uint64) if rows is None else np.asarray(rows, dtype=np.uint64)
    adj = adjacency_sets(n, edges)
    out = np.full((b, 2 + k), -1, np.int64)
    out[:, :2] = pairs
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    slots = np.arange(k, dtype=np.uint64)
    for t in range(max_tries):
        if k == 0 or b == 0:
            break
        r = philox4x32_10((rows[:, None], slots[None, :], np.uint64(t), np.uint64(step)), key)[0]
        cand = ((r * np.uint64(n)) >> np.uint64(32)).astype(np.int64)
        for i in range(b):
            a = int(pairs[i, 0])
            if not 0 <= a < n:
                continue
            for j in range(k):
                if out[i, 2 + j] < 0:
                    cj = int(cand[i, j])
                    if cj != a and cj not in adj[a]:
                        out[i, 2 + j] = cj
    return out


def path_graph(n):
    return n, np.array([(i, i + 1) for i in range(n - 1)], dtype=np.int64).reshape(-1, 2)


def star_graph(n):
    return n, np.array([(0, i) for i in range(1, n)], dtype=np.int64).reshape(-1, 2)


def complete_graph(n):
    return n, np.array([(i, j) for i in range(n) for j in range(i + 1, n)], dtype=np.int64).reshape(-1, 2)


def random_sparse_graph(n, seed=0):
    """About 2 n random edges with repeats and self-loops left in; node n - 1 has no edge."""
    rs = np.random.RandomState(seed)
    e = rs.randint(0, max(n - 1, 1), (2 * n, 2)).astype(np.int64)
    return n, e


def tree_graph(n=63):
    """Balanced binary tree in heap order: node i has children 2 i + 1 and 2 i + 2."""
    return n, np.array([((i - 1) // 2, i) for i in range(1, n)], dtype=np.int64)


# ---- end to end: a balanced binary tree of 63 nodes in 5 dimensions ------------------------------------------------------------
E2E = dict(dim=5, epochs=75, batch_size=32, num_negatives=10, lr=0.1, seed=3, init_scale=1e-3)      # 4 batches an epoch: 300 batches


def e2e_eval_index():
    """The fixed evaluation batch: every edge in both directions, natural order, negatives of step 0."""
    n, e = tree_graph()
    pairs = np.concatenate([e, e[:, ::-1]], 0)
    return torch.from_numpy(sample_reference(n, e, pairs, E2E["num_negatives"], E2E["seed"], 0))


def e2e_init():
    gen = torch.Generator().manual_seed(E2E["seed"])
    s = (torch.rand((63, E2E["dim"]), generator=gen, dtype=torch.float32) * 2.0 - 1.0) * E2E["init_scale"]
    return torch.cat([torch.sqrt(1.0 + (s * s).sum(-1, keepdim=True)), s], -1)


def e2e_mean_loss(x: torch.Tensor, index: torch.Tensor) -> float:
    return float(loss_terms(x, index, 1.0)[0].mean())


@functools.lru_cache(maxsize=None)
def e2e_loop_float64():
    """``fit_graph_embedding``'s loop in float64 on the CPU (truth loss, sampler restatement, riemannian_cases.sgd_step) ->
    (evaluation loss before, after, evaluation loss after every epoch)."""
    n, e = tree_graph()
    positives = np.concatenate([e, e[:, ::-1]], 0)
    x = e2e_init().double()
    ev = e2e_eval_index()
    before = e2e_mean_loss(x, ev)
    gen = torch.Generator().manual_seed(E2E["seed"])
    history, step = [], 0
    for _ in range(E2E["epochs"]):
        order = torch.randperm(positives.shape[0], generator=gen).numpy()
        for b0 in range(0, positives.shape[0], E2E["batch_size"]):
            idx = torch.from_numpy(sample_reference(n, e, positives[order[b0:b0 + E2E["batch_size"]]], E2E["num_negatives"],
                                                    E2E["seed"], step))
            xr = x.clone().requires_grad_(True)
            loss_terms(xr, idx, 1.0)[0].sum().backward()
            x, _ = sgd_step(x, xr.grad, None, E2E["lr"])
            step += 1
        history.append(e2e_mean_loss(x, ev))
    return before, history[-1], history


#: what e2e_loop_float64 returns for (before, after), recorded: the GPU run must lose at least half of the difference
E2E_FLOAT64 = (2.397978104011292, 0.2936862070842693)
