"""Lorentz-centroid pooling: the truth, the closed-form backward and the seeded cases shared by
test_pooling_host.py (no GPU) and test_gpu_pooling.py.

The truth of a case is the definition written out in torch and evaluated on the CPU in float64, both gradients taken by
torch autograd; the place of a reference is taken by the same expression in float32 on the CPU, whose error against the
truth is e_ref.  The measure, ``FACTOR`` and ``FLOOR`` are those of tests/autograd_cases.py: ``e_hip <= FACTOR * e_ref + FLOOR``.

The definition.  Segment i is ids[offsets[i] : offsets[i] + len_i] (len_i = lengths[i], or the whole span); a token is live
when it lies inside that length and its id lies in [0, V).  s_i = sum_t w_t x_{ids[t]} over the live tokens,
q_i = s_i0^2 - |s_is|^2, mu_i = s_i / sqrt(q_i).  Where a segment has no live token or q_i is not positive and finite the
result is the origin and every gradient of the segment is exactly zero: ``centroid`` finds those segments first and keeps
their tokens out of the differentiated expression.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

from autograd_cases import FACTOR, FLOOR, grad_error, infonce  # noqa: F401  (re-exported)
from graph_embedding_cases import SCALES, V, WELL, WIDTHS, table  # noqa: F401
from riemannian_cases import ldot, lift, sgd_step  # noqa: F401

BATCHES = (1, 3, 37, 257)                                      # partly filled group, partly filled wave, several blocks
LENGTHS = (0, 1, 2, 3, 7, 16, 33, 70, 1, 5)                    # empty, below the rows in flight, below / above the groups of a wave, several rounds
SLACK = (0, 0, 1, 0, 2, 0, 0, 3, 0, 0)                         # positions behind the tokens of a span


# ---- the definition ---------------------------------------------------------------------------------------------------------
def segment_of(t: int, offsets: torch.Tensor, lengths) -> torch.Tensor:
    """int64 [T]: the segment a position belongs to, -1 for slack and for positions outside every span."""
    seg = np.full(t, -1, np.int64)
    off = offsets.tolist()
    for i in range(len(off) - 1):
        n = off[i + 1] - off[i] if lengths is None else int(lengths[i])
        seg[off[i]:off[i] + n] = i
    return torch.from_numpy(seg)


def _sums(x, ids, seg, w, n):
    s = torch.zeros((n, x.shape[1]), dtype=x.dtype)
    return s.index_add(0, seg, w[:, None] * x[ids])


def centroid(x: torch.Tensor, ids: torch.Tensor, offsets: torch.Tensor, lengths=None, weights=None):
    """(mu [n, d1], ok [n]) in the dtype of ``x``; differentiable in ``x`` and ``weights``."""
    n, v = offsets.numel() - 1, x.shape[0]
    seg = segment_of(ids.numel(), offsets, lengths)
    live = (seg >= 0) & (ids >= 0) & (ids < v)
    w = torch.ones(ids.numel(), dtype=x.dtype) if weights is None else weights.to(x.dtype)
    with torch.no_grad():
        s = _sums(x, ids[live], seg[live], w[live], n)
        q = s[:, 0] ** 2 - (s[:, 1:] ** 2).sum(-1)
        ok = (q > 0) & torch.isfinite(q)
    live = live & ok[seg.clamp(min=0)]
    s = _sums(x, ids[live], seg[live], w[live], n)
    q = s[:, 0] ** 2 - (s[:, 1:] ** 2).sum(-1)
    origin = torch.zeros_like(s)
    origin[:, 0] = 1
    one = torch.ones((), dtype=x.dtype)
    return torch.where(ok[:, None], s / torch.sqrt(torch.where(ok, q, one))[:, None], origin), ok


def closed_form(x, ids, offsets, lengths, weights, g):
    """(dense table gradient [V, d1], weight gradient [T]) from DESIGN.md 5.18: h = (g + (g . mu) J mu) / nu, position t of
    segment i adds w_t h_i to row ids[t] and has dL/dw_t = h_i . x_{ids[t]}."""
    n, v = offsets.numel() - 1, x.shape[0]
    seg = segment_of(ids.numel(), offsets, lengths)
    w = torch.ones(ids.numel(), dtype=x.dtype) if weights is None else weights.to(x.dtype)
    mu, ok = centroid(x, ids, offsets, lengths, weights)
    live = (seg >= 0) & (ids >= 0) & (ids < v)
    live = live & ok[seg.clamp(min=0)]
    s = _sums(x, ids[live], seg[live], w[live], n)
    nu = torch.sqrt(torch.where(ok, s[:, 0] ** 2 - (s[:, 1:] ** 2).sum(-1), torch.ones((), dtype=x.dtype)))
    jmu = torch.cat([-mu[:, :1], mu[:, 1:]], -1)
    h = (g + (g * mu).sum(-1, keepdim=True) * jmu) / nu[:, None]
    h = torch.where(ok[:, None], h, torch.zeros_like(h))
    gx = torch.zeros_like(x).index_add(0, ids[live], w[live, None] * h[seg[live]])
    gw = torch.zeros(ids.numel(), dtype=x.dtype)
    gw[live] = (h[seg[live]] * x[ids[live]]).sum(-1)
    return gx, gw


def evaluate(x, ids, offsets, lengths, weights, g, dtype):
    """(mu, dense table gradient, weight gradient [T] or None) of sum(g * mu) as numpy, by autograd in ``dtype`` on the CPU."""
    xr = x.to(dtype).clone().requires_grad_(True)
    wr = None if weights is None else weights.to(dtype).clone().requires_grad_(True)
    mu, _ = centroid(xr, ids, offsets, lengths, wr)
    (mu * g.to(dtype)).sum().backward()
    gx = xr.grad if xr.grad is not None else torch.zeros_like(xr)
    gw = None if wr is None else (wr.grad if wr.grad is not None else torch.zeros_like(wr)).numpy()
    return mu.detach().numpy(), gx.numpy(), gw


def defect(mu) -> np.ndarray:
    """|mu0^2 - |mu_s|^2 - 1| per row, evaluated in float64."""
    mu = np.asarray(mu, np.float64)
    return np.abs(mu[:, 0] ** 2 - (mu[:, 1:] ** 2).sum(-1) - 1)


# ---- seeded inputs ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def bags(n: int, seed: int = 0, rows: int = V):
    """(ids int64 [T], offsets int64 [n + 1], lengths int32 [n], weights fp32 [T]) of ``n`` bags whose lengths and slack cycle
    through LENGTHS and SLACK.  The slack holds valid ids (they must be skipped because of ``lengths``, not of their value);
    every bag of 3 has a -1 in the middle and every bag of 16 starts with one, every bag of 7 repeats its first id twice."""
    gen = torch.Generator().manual_seed(31 * n + seed)
    lens = [LENGTHS[i % len(LENGTHS)] for i in range(n)]
    span = [lens[i] + SLACK[i % len(SLACK)] for i in range(n)]
    offsets = torch.zeros(n + 1, dtype=torch.int64)
    offsets[1:] = torch.cumsum(torch.tensor(span, dtype=torch.int64), 0)
    t = int(offsets[-1])
    ids = torch.randint(0, rows, (t,), generator=gen, dtype=torch.int64)
    for i in range(n):
        b = int(offsets[i])
        if lens[i] == 3:
            ids[b + 1] = -1
        if lens[i] == 16:
            ids[b] = -1
        if lens[i] == 7:
            ids[b + 1] = ids[b + 3] = ids[b]
    weights = (0.25 + torch.rand(t, generator=gen, dtype=torch.float64)).float()
    return ids, offsets, torch.tensor(lens, dtype=torch.int32), weights


def compact(ids, offsets, lengths, weights):
    """The slab without its slack: (ids, offsets, weights) whose whole spans are the bags."""
    keep = segment_of(ids.numel(), offsets, lengths) >= 0
    off = torch.zeros_like(offsets)
    off[1:] = torch.cumsum(lengths.to(torch.int64), 0)
    return ids[keep], off, weights[keep]


@functools.lru_cache(maxsize=None)
def upstream(n: int, d1: int, seed: int = 0) -> torch.Tensor:
    gen = torch.Generator().manual_seed(7 * n + 1000 * d1 + seed)
    return torch.randn(n, d1, generator=gen, dtype=torch.float64).float()


def variant(n: int, use_lengths: bool, use_weights: bool):
    """(ids, offsets, lengths | None, weights | None) of the seeded bags."""
    ids, offsets, lengths, weights = bags(n)
    return ids, offsets, (lengths if use_lengths else None), (weights if use_weights else None)


@functools.lru_cache(maxsize=None)
def reference(d1: int, n: int, use_lengths: bool, use_weights: bool, scales=SCALES):
    """((mu, table gradient, weight gradient) float64 truth, the same in fp32 on the CPU) of a seeded case, computed once."""
    x, g = table(d1, scales=scales), upstream(n, d1)
    ids, offsets, lengths, weights = variant(n, use_lengths, use_weights)
    return tuple(evaluate(x, ids, offsets, lengths, weights, g, dt) for dt in (torch.float64, torch.float32))


def compare(name: str, truth, ref32, ours, failures: list) -> None:
    """Prints ``name e_ref e_hip`` for mu, the table gradient and the weight gradient and appends what misses the bound."""
    for what, t, r, o in zip(("mu", "grad", "wgrad"), truth, ref32, ours):
        if t is None:
            continue
        e_ref, _ = grad_error(r, r, t)
        e_hip, pattern_ok = grad_error(np.asarray(o).reshape(np.shape(r)), r, t)
        print(f"{name}:{what} e_ref={e_ref:.3e} e_hip={e_hip:.3e}")
        if not pattern_ok:
            failures.append(f"{name}:{what}: non-finite pattern differs from the fp32 reference's")
        elif not e_hip <= FACTOR * e_ref + FLOOR:
            failures.append(f"{name}:{what}: e_ref={e_ref:.3e} e_hip={e_hip:.3e}")


# ---- composition: two sets of 32 bags over a 60-row table of width 6, InfoNCE between their centroids ---------------------------
E2E = dict(rows=60, d1=6, bags=32, steps=30, lr=1.0, temp=0.2, seed=11, scale=0.3)


@functools.lru_cache(maxsize=None)
def e2e_inputs():
    """(table fp32 [60, 6], bags a, bags b): bag k of both sets shares three "topic" rows (k, k + 1, k + 2 mod 60) and adds
    random ones, so pulling mu_a[k] towards mu_b[k] and away from the other bags is learnable."""
    e = E2E
    gen = torch.Generator().manual_seed(e["seed"])
    x = lift(torch.randn(e["rows"], e["d1"] - 1, generator=gen, dtype=torch.float64) * e["scale"]).float()
    sets = []
    for _ in range(2):
        ids, offsets = [], [0]
        for k in range(e["bags"]):
            extra = torch.randint(0, e["rows"], (int(torch.randint(1, 6, (1,), generator=gen)),), generator=gen).tolist()
            ids += [(2 * k) % e["rows"], (2 * k + 1) % e["rows"], (2 * k + 2) % e["rows"]] + extra
            offsets.append(len(ids))
        sets.append((torch.tensor(ids, dtype=torch.int64), torch.tensor(offsets, dtype=torch.int64)))
    return x, sets[0], sets[1]


def e2e_loss(x, a, b):
    mu_a, _ = centroid(x, a[0], a[1])
    mu_b, _ = centroid(x, b[0], b[1])
    return infonce(mu_a, mu_b, E2E["temp"], "mean", -1.0)


@functools.lru_cache(maxsize=None)
def e2e_loop_float64():
    """The training loop in float64 on the CPU (truth pooling, autograd_cases.infonce, riemannian_cases.sgd_step) ->
    (loss before, loss after, loss after every step)."""
    x, a, b = e2e_inputs()
    x = x.double()
    before = float(e2e_loss(x, a, b))
    history = []
    for _ in range(E2E["steps"]):
        xr = x.clone().requires_grad_(True)
        e2e_loss(xr, a, b).backward()
        x, _ = sgd_step(x, xr.grad, None, E2E["lr"])
        history.append(float(e2e_loss(x, a, b)))
    return before, history[-1], history


#: what e2e_loop_float64 returns for (before, after), recorded: the GPU run must lose at least half of the difference
E2E_FLOAT64 = (3.1620301400508053, 1.1270567256601214)
