#!/usr/bin/env python
"""A/B of the fused Riemannian optimiser steps (hyptokenizer_amd.optim) against the same step composed from torch ops, on
one GPU in one process.  There is no fallback: without a GPU the probe fails.

Per shape (50 000 x 101 and 2^20 x 65, dense) and optimiser (RSGD without and with momentum, RAdam), and for one indexed
run (8 192 distinct rows of the 50 000-row table, through a coalesced sparse gradient): one sample is a batch of
``--calls`` back-to-back steps between two device events (a single step is tens of microseconds: too short a window),
divided by the number of calls; fused, composed and copy are interleaved sample by sample and the median, minimum and
maximum over ``--reps`` samples are reported.  ``copy`` is a ``copy_`` of as many bytes as the fused step has to move
(x, g and m read once, x and m written once, v read and written) -- the machine's own bandwidth yardstick.  Also: peak
memory of one step above parameters, gradient and state.  The learning rate is tiny so that hundreds of steps along one
fixed gradient leave the points where they started.  Writes profiles/riemannian_probe.json.

Usage:  python tools/riemannian_probe.py [--reps 15] [--calls 20] [--out profiles/riemannian_probe.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from hyptokenizer_amd.optim import RiemannianAdam, RiemannianSGD  # noqa: E402

DEV = "cuda:0"
SHAPES = ((50000, 101), (1 << 20, 65))
INDEXED = (50000, 101, 8192)
LR = 1e-4
OPTIMISERS = {"rsgd": dict(momentum=0.0), "rsgd_momentum": dict(momentum=0.9), "radam": dict(betas=(0.9, 0.999), eps=1e-8)}


# ---- the same step composed from torch ops -------------------------------------------------------------
def ldot(a, b):
    return -a[..., 0] * b[..., 0] + (a[..., 1:] * b[..., 1:]).sum(-1)


def rgrad(x, g):
    h = torch.cat([-g[..., :1], g[..., 1:]], -1)
    return h + ldot(x, h).unsqueeze(-1) * x


def retract(x, s):
    n = torch.sqrt(torch.clamp(ldot(s, s), min=0)).unsqueeze(-1)
    one = torch.ones_like(n)
    ys = (torch.cosh(n) * x + torch.where(n > 0, torch.sinh(n) / torch.where(n > 0, n, one), one) * s)[..., 1:]
    return torch.cat([torch.sqrt(1 + (ys * ys).sum(-1, keepdim=True)), ys], -1)


def transport(x, y, w):
    w = w + (ldot(y, w) / (1 - ldot(x, y))).unsqueeze(-1) * (x + y)
    return w + ldot(y, w).unsqueeze(-1) * y


def composed_values(name, x, g, m, v, t):
    """(x', m', v') of one step as new tensors; m, v None where the optimiser has none."""
    u = rgrad(x, g)
    if name == "rsgd":
        return retract(x, -LR * u), None, None
    if name == "rsgd_momentum":
        m2 = 0.9 * m + u
        y = retract(x, -LR * m2)
        return y, transport(x, y, m2), None
    m2 = 0.9 * m + 0.1 * u
    v2 = 0.999 * v + 0.001 * ldot(u, u)
    y = retract(x, -LR * (m2 / (1 - 0.9 ** t)) / (torch.sqrt(v2 / (1 - 0.999 ** t)) + 1e-8).unsqueeze(-1))
    return y, transport(x, y, m2), v2


class Composed:
    """In-place step from torch ops on its own copies of the parameter and state; ``idx``: only those rows."""

    def __init__(self, name, x, g, idx=None):
        self.name, self.x, self.g, self.idx, self.t = name, x.clone(), g, idx, 0
        self.m = torch.zeros_like(x) if name != "rsgd" else None
        self.v = torch.zeros(x.shape[0], device=DEV) if name == "radam" else None

    @torch.no_grad()
    def step(self):
        self.t += 1
        if self.idx is None:
            y, m2, v2 = composed_values(self.name, self.x, self.g, self.m, self.v, self.t)
            self.x.copy_(y)
            if m2 is not None:
                self.m.copy_(m2)
            if v2 is not None:
                self.v.copy_(v2)
            return
        i = self.idx
        y, m2, v2 = composed_values(self.name, self.x[i], self.g, None if self.m is None else self.m[i],
                                    None if self.v is None else self.v[i], self.t)
        self.x.index_copy_(0, i, y)
        if m2 is not None:
            self.m.index_copy_(0, i, m2)
        if v2 is not None:
            self.v.index_copy_(0, i, v2)


class Fused:
    def __init__(self, name, x, grad):
        self.p = torch.nn.Parameter(x.clone())
        kw = OPTIMISERS[name]
        self.opt = (RiemannianAdam if name == "radam" else RiemannianSGD)([self.p], lr=LR, **kw)
        self.p.grad = grad

    def step(self):
        self.opt.step()


def table(rows, d1, gen):
    s = torch.randn(rows, d1 - 1, device=DEV, generator=gen) / (d1 - 1) ** 0.5
    return torch.cat([torch.sqrt(1 + (s * s).sum(-1, keepdim=True)), s], -1)


def timed(fn, calls):
    """ms per call of a batch of ``calls`` back-to-back calls."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - base)


def moved_bytes(name, n, d1, indexed):
    per_row = {"rsgd": 3, "rsgd_momentum": 5, "radam": 5}[name] * d1 * 4 + (8 if name == "radam" else 0) + (8 if indexed else 0)
    return n * per_row


def measure(name, rows, d1, n_idx, gen, reps, calls):
    x = table(rows, d1, gen)
    if n_idx:
        idx = torch.randperm(rows, device=DEV, generator=gen)[:n_idx].sort().values
        g = torch.randn(n_idx, d1, device=DEV, generator=gen) / d1 ** 0.5
        grad = torch.sparse_coo_tensor(idx.unsqueeze(0), g, (rows, d1)).coalesce()
        composed = Composed(name, x, g, idx)
    else:
        g = torch.randn(rows, d1, device=DEV, generator=gen) / d1 ** 0.5
        grad, composed = g, Composed(name, x, g)
    fused = Fused(name, x, grad)
    moved = moved_bytes(name, n_idx or rows, d1, bool(n_idx))
    src, dst = torch.empty(moved // 8, device=DEV), torch.empty(moved // 8, device=DEV)
    variants = {"fused": fused.step, "composed": composed.step, "copy": lambda: dst.copy_(src)}
    for fn in variants.values():                                          # warm-up of every shape that is timed (and of the state)
        for _ in range(3):
            fn()
    peaks = {k: peak(variants[k]) for k in ("fused", "composed")}
    times = {k: [] for k in variants}
    for _ in range(reps):                                                 # interleaved: one sample of each per round
        for k, fn in variants.items():
            times[k].append(timed(fn, calls))
    ms = {k: statistics.median(v) for k, v in times.items()}
    finite = bool(torch.isfinite(fused.p).all()) and bool(torch.isfinite(composed.x).all())
    drift = float((fused.p.detach() - composed.x).abs().max())
    return {"optimiser": name, "rows": rows, "d1": d1, "indexed_rows": n_idx, "lr": LR, "reps": reps, "calls_per_sample": calls,
            "median_ms": ms, "min_ms": {k: min(v) for k, v in times.items()}, "max_ms": {k: max(v) for k, v in times.items()},
            "bytes_moved_fused": moved, "fused_GBps": moved / ms["fused"] / 1e6, "copy_GBps": moved / ms["copy"] / 1e6,
            "fused_fraction_of_copy": ms["copy"] / ms["fused"], "speedup_over_composed": ms["composed"] / ms["fused"],
            "peak_bytes_above_parameters_gradient_and_state": peaks,
            "all_finite_after_the_run": finite, "max_abs_difference_fused_vs_composed_after_the_run": drift}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "riemannian_probe.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "riemannian_probe.py measures on a GPU; there is nothing to report without one"
    gen = torch.Generator(device=DEV).manual_seed(7)
    results = []
    for rows, d1, n_idx in [s + (0,) for s in SHAPES] + [INDEXED]:
        for name in OPTIMISERS:
            row = measure(name, rows, d1, n_idx, gen, args.reps, args.calls)
            results.append(row)
            print(json.dumps(row), flush=True)
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "results": results}, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
