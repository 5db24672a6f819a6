#!/usr/bin/env python
"""A/B of the fused Poincare-ball kernels against the same expressions composed from torch ops, on one GPU in one process.

Per op and shape (50 000 x 100 and 2^20 x 64): forward, and forward plus backward.  One sample is a batch of ``--calls``
back-to-back calls between two device events (a single call is 50-250 us: too short a window), divided by the number of
calls; the variants are interleaved sample by sample and the median, minimum and maximum over ``--reps`` samples are
reported.  Also: peak memory above the inputs; a ``copy_`` of as many bytes as the fused forward has to move (operands
read once, result written once) as the machine's own bandwidth yardstick, and the achieved GB/s of the fused forward as
a fraction of that copy.  The composed form is the reference's expression written with torch ops (below).  Writes
profiles/poincare_probe.json.

Usage:  python tools/poincare_probe.py [--reps 15] [--calls 20] [--out profiles/poincare_probe.json]
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

from hyptokenizer_amd.embedding import poincare_ball as pb  # noqa: E402

DEV = "cuda:0"
SHAPES = ((50000, 100), (1 << 20, 64))
C = 1.0


# ---- the same expressions composed from torch ops (embedding/poincare_ball.py of the reference, c a float) ----------------
def _norm(x):
    return torch.norm(x, dim=-1, keepdim=True)


def _mobius_addition(x, y, c):
    x2, y2, xy = (x * x).sum(-1, keepdim=True), (y * y).sum(-1, keepdim=True), (x * y).sum(-1, keepdim=True)
    return ((1 + 2 * c * xy + c * y2) * x + (1 - c * x2) * y) / (1 + 2 * c * xy + c * c * x2 * y2)


def _mobius_scalar_mul(r, x, c):
    a = c ** 0.5 * torch.clamp(_norm(x), min=1e-8)
    return torch.tanh(r * torch.atanh(a)) / a * x


def _zero_map(f, v, c):
    n = _norm(v)
    mask = (n == 0).to(v.dtype)
    a = c ** 0.5 * torch.clamp(n, min=1e-8)
    return f(a) / a * v * (1 - mask) + mask * v


def _distance(x, y, c):
    return 2 / c ** 0.5 * torch.atanh(c ** 0.5 * _norm(_mobius_addition(-x, y, c)))


def _poincare_to_lorentz(x, c):
    x2 = (x * x).sum(-1, keepdim=True)
    f = 1.0 / (1 - c * x2)
    return torch.cat([f * (1 + c * x2) / (2 * c ** 0.5), f * x], dim=-1)


COMPOSED = {
    "mobius_addition": _mobius_addition,
    "mobius_scalar_mul": _mobius_scalar_mul,
    "exp_map_zero": lambda v, c: _zero_map(torch.tanh, v, c),
    "log_map_zero": lambda x, c: _zero_map(torch.atanh, x, c),
    "distance": _distance,
    "lorentz_to_poincare": lambda x, c: x[..., 1:] / (x[..., 0:1] + 1 / c ** 0.5),
    "poincare_to_lorentz": _poincare_to_lorentz,
}


def inputs(op, rows, d, gen):
    v = torch.randn(rows, d, device=DEV, generator=gen)
    x = v / v.norm(dim=-1, keepdim=True) * (0.05 + 0.85 * torch.rand(rows, 1, device=DEV, generator=gen))
    if op in ("mobius_addition", "distance"):
        w = torch.randn(rows, d, device=DEV, generator=gen)
        return [x, w / w.norm(dim=-1, keepdim=True) * (0.05 + 0.85 * torch.rand(rows, 1, device=DEV, generator=gen))]
    if op == "mobius_scalar_mul":
        return [torch.rand(rows, 1, device=DEV, generator=gen) * 2, x]
    if op == "lorentz_to_poincare":
        z = torch.randn(rows, d + 1, device=DEV, generator=gen) / d ** 0.5
        z[:, 0] = torch.sqrt(1 + (z[:, 1:] ** 2).sum(-1))
        return [z]
    return [x]


def timed(fn, calls):
    """ms per call of a batch of ``calls`` back-to-back calls."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def peak(fn, live):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    keep = fn()
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base
    del keep
    return int(extra)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "poincare_probe.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "poincare_probe.py measures on a GPU; there is nothing to report without one"
    gen = torch.Generator(device=DEV).manual_seed(5)
    results = []
    for rows, d in SHAPES:
        for op in COMPOSED:
            ins = inputs(op, rows, d, gen)
            fused, composed = getattr(pb, op), COMPOSED[op]
            out = fused(*ins, C)
            g = torch.randn_like(out)
            moved = sum(t.numel() for t in ins) * 4 + out.numel() * 4
            src, dst = torch.empty(moved // 8, device=DEV), torch.empty(moved // 8, device=DEV)

            def fwd(f):
                return lambda: f(*ins, C)

            def fwd_bwd(f):
                def run():
                    leaves = [t.detach().requires_grad_() for t in ins]
                    f(*leaves, C).backward(g)
                    return [t.grad for t in leaves]
                return run

            variants = {"fused_fwd": fwd(fused), "composed_fwd": fwd(composed), "fused_fwd_bwd": fwd_bwd(fused),
                        "composed_fwd_bwd": fwd_bwd(composed), "copy": lambda: dst.copy_(src)}
            for fn in variants.values():                                  # warm-up of every shape that is timed
                for _ in range(3):
                    fn()
            times = {k: [] for k in variants}
            for _ in range(args.reps):                                    # interleaved: one run of each per round
                for k, fn in variants.items():
                    times[k].append(timed(fn, args.calls))
            ms = {k: statistics.median(v) for k, v in times.items()}
            row = {"op": op, "rows": rows, "d": d, "c": C, "reps": args.reps, "calls_per_sample": args.calls, "median_ms": ms,
                   "min_ms": {k: min(v) for k, v in times.items()}, "max_ms": {k: max(v) for k, v in times.items()},
                   "bytes_moved_fused_fwd": moved,
                   "fused_fwd_GBps": moved / ms["fused_fwd"] / 1e6, "copy_GBps": moved / ms["copy"] / 1e6,
                   "fused_fwd_fraction_of_copy": ms["copy"] / ms["fused_fwd"],
                   "speedup_fwd": ms["composed_fwd"] / ms["fused_fwd"], "speedup_fwd_bwd": ms["composed_fwd_bwd"] / ms["fused_fwd_bwd"],
                   "peak_bytes_above_inputs": {k: peak(fn, ins) for k, fn in variants.items() if k != "copy"}}
            results.append(row)
            print(json.dumps(row), flush=True)
            del src, dst, out, g, ins
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "results": results}, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
