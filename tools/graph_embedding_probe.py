#!/usr/bin/env python
"""A/B of the fused graph-embedding step (hyptokenizer_amd.embedding.graph_embedding) against the same step composed from
torch ops, on one GPU in one process.  There is no fallback: without a GPU the probe fails.

Graph: the synthetic WordNet-shaped graph of tools/hierarchy_distortion_probe.py (82 115 nodes).  Per shape (d1 in {11, 101},
B in {1 024, 16 384}, K = 50) four things are timed, each as fused / composed / copy:
  sampler   NegativeSampler.sample                    | torch.randint + cat -- NO neighbour rejection, so it does less work
  forward   edge_softmax_loss, no gradient            | gather table[index] + lorentz_model.distance + logsumexp
  fwd_bwd   loss + backward (sparse COO gradient)     | the same under autograd: a dense [V, d1] gradient by index_put
  step      sampler + fwd_bwd + RiemannianSGD.step    | randint + fwd_bwd + RiemannianSGD.step on the dense gradient
``copy`` is a ``copy_`` of as many bytes as the fused kernels of that row have to move (index read, partner rows gathered,
weights, values and COO indices written; for ``step`` also the optimiser's rows) -- the machine's own bandwidth yardstick.
One sample is a batch of ``--calls`` back-to-back calls between two device events divided by the number of calls; the three
variants are interleaved sample by sample and the median, minimum and maximum over ``--reps`` samples are reported, with the
peak memory of one call above the table.  The learning rate is tiny so that the table stays where it started (the composed
table does not stay finite: ``randint`` draws the anchor as its own negative now and then, and the derivative of ``distance``
at u = 1 is NaN -- the fused loss has a zero gradient there).  Rows ``kernel_*``: the two loss kernels alone through the C
ABI on preallocated buffers, 50 launches per sample, in both work decompositions (``hm_debug_edge_loss_form``); everything
else runs the default form.  Writes profiles/graph_embedding_probe.json.

Usage:  python tools/graph_embedding_probe.py [--reps 11] [--calls 10] [--out profiles/graph_embedding_probe.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from hierarchy_distortion_probe import wordnet_shaped_graph  # noqa: E402
from hyptokenizer_amd.embedding import lorentz_model as lm  # noqa: E402
from hyptokenizer_amd.embedding.graph_embedding import NegativeSampler, edge_softmax_loss  # noqa: E402
from hyptokenizer_amd.optim import RiemannianSGD  # noqa: E402

DEV = "cuda:0"
WIDTHS, BATCHES, K, LR = (11, 101), (1024, 16384), 50, 1e-6


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def peak(fn, params=()):
    for p in params:                                          # a gradient left by an earlier call would hide the new one
        p.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - base)


def composed_loss(table, index):
    x = table[index]
    d = lm.distance(x[:, :1], x[:, 1:], sign_convention="lorentz")
    return (d[:, 0] + torch.logsumexp(-d, dim=1)).sum()


def moved_bytes(b, d1):
    slots, row = b * (2 + K), d1 * 4
    fwd = slots * (8 + row) + b * (1 + K) * 4 * 3 + b * 4
    bwd = slots * (8 + row) + b * (1 + K) * 4 + b * 4 + slots * (row + 8)
    sampler = b * 16 + slots * 8
    return {"sampler": sampler, "forward": fwd, "fwd_bwd": fwd + bwd, "step": sampler + fwd + bwd + slots * (8 + 3 * row)}


def measure(graph, sampler, pairs_all, d1, b, reps, calls, gen):
    v = sampler.n
    s = (torch.rand(v, d1 - 1, device=DEV, generator=gen) * 2 - 1) * 0.5 / (d1 - 1) ** 0.5
    x0 = torch.cat([torch.sqrt(1 + (s * s).sum(-1, keepdim=True)), s], -1)
    pairs = pairs_all[torch.randperm(pairs_all.shape[0], device=DEV, generator=gen)[:b]].contiguous()
    index = sampler.sample(pairs, 0)
    pf, pc = torch.nn.Parameter(x0.clone()), torch.nn.Parameter(x0.clone())
    of, oc = RiemannianSGD([pf], lr=LR), RiemannianSGD([pc], lr=LR)
    state = {"step": 0}

    def composed_index():
        return torch.cat([pairs, torch.randint(0, v, (b, K), device=DEV)], 1)

    def fused_fb(idx=index):
        pf.grad = None
        edge_softmax_loss(pf, idx, 1.0, "sum", validate=False).backward()

    def composed_fb(idx=index):
        pc.grad = None
        composed_loss(pc, idx).backward()

    def fused_step():
        state["step"] += 1
        fused_fb(sampler.sample(pairs, state["step"]))
        of.step()

    def composed_step():
        composed_fb(composed_index())
        oc.step()

    def fused_fwd():
        with torch.no_grad():
            return edge_softmax_loss(pf, index, 1.0, "sum", validate=False)

    def composed_fwd():
        with torch.no_grad():
            return composed_loss(pc, index)

    with torch.no_grad():                                     # before any step: the two forms of the loss agree
        agree = float((fused_fwd() - composed_fwd()).abs() / composed_fwd().abs())

    pairs_of = {"sampler": (lambda: sampler.sample(pairs, 1), composed_index), "forward": (fused_fwd, composed_fwd),
                "fwd_bwd": (fused_fb, composed_fb), "step": (fused_step, composed_step)}
    moved = moved_bytes(b, d1)
    rows = []
    for what, (fused, composed) in pairs_of.items():
        n8 = max(moved[what] // 8, 1)
        src, dst = torch.empty(n8, device=DEV), torch.empty(n8, device=DEV)
        variants = {"fused": fused, "composed": composed, "copy": lambda: dst.copy_(src)}
        for fn in variants.values():
            for _ in range(3):
                fn()
        peaks = {k: peak(variants[k], (pf, pc)) for k in ("fused", "composed")}
        times = {k: [] for k in variants}
        for _ in range(reps):
            for k, fn in variants.items():
                times[k].append(timed(fn, calls))
        ms = {k: statistics.median(t) for k, t in times.items()}
        rows.append({"what": what, "nodes": v, "d1": d1, "batch": b, "negatives": K, "reps": reps, "calls_per_sample": calls,
                     "median_ms": ms, "min_ms": {k: min(t) for k, t in times.items()}, "max_ms": {k: max(t) for k, t in times.items()},
                     "bytes_moved_fused": moved[what], "fused_GBps": moved[what] / ms["fused"] / 1e6,
                     "copy_GBps": moved[what] / ms["copy"] / 1e6, "fused_fraction_of_copy": ms["copy"] / ms["fused"],
                     "speedup_over_composed": ms["composed"] / ms["fused"], "peak_bytes_above_the_table": peaks})
        print(json.dumps(rows[-1]), flush=True)
    rows += kernel_rows(x0, index, b, d1, v, moved, reps)
    finite = {"fused": bool(torch.isfinite(pf).all()), "composed": bool(torch.isfinite(pc).all())}
    for r in rows:
        r["relative_difference_of_the_two_losses_before_the_run"] = agree
        r["table_finite_after_the_run"] = finite
    return rows


def kernel_rows(x, index, b, d1, v, moved, reps, calls=50):
    """The two loss kernels alone, through the C ABI on preallocated buffers: ``calls`` back-to-back launches between two
    events, so that what is timed is the device (or, below a few microseconds per kernel, the launch rate)."""
    from hyptokenizer_amd import _lib
    from hyptokenizer_amd.engine import _ptr, _stream_of
    L = _lib.load()
    loss, w, gl = torch.empty(b, device=DEV), torch.empty((b, 1 + K), device=DEV), torch.ones(b, device=DEV)
    val = torch.empty((b * (2 + K), d1), device=DEV)
    coo = torch.empty(b * (2 + K), dtype=torch.int64, device=DEV)
    st = _stream_of(x)

    def fwd():
        _lib.check(L.hm_edge_loss_fwd(_ptr(x), d1, v, d1, _ptr(index), b, K, 1.0, _ptr(loss), _ptr(w), st))

    def bwd():
        _lib.check(L.hm_edge_loss_bwd(_ptr(x), d1, v, d1, _ptr(index), b, K, 1.0, _ptr(w), _ptr(gl), _ptr(val), _ptr(coo), st))

    rows = []
    cases = [(f"kernel_{what}_{name}", form, fn, nbytes) for form, name in ((0, "group_per_sample"), (1, "wave_per_sample"))
             for what, fn, nbytes in (("forward", fwd, moved["forward"]), ("backward", bwd, moved["fwd_bwd"] - moved["forward"]))]
    for what, form, fn, nbytes in cases:
        _lib.check(L.hm_debug_edge_loss_form(form))
        src, dst = torch.empty(max(nbytes // 8, 1), device=DEV), torch.empty(max(nbytes // 8, 1), device=DEV)
        variants = {"fused": fn, "copy": lambda: dst.copy_(src)}
        for f in variants.values():
            for _ in range(3):
                f()
        times = {k: [] for k in variants}
        for _ in range(reps):
            for k, f in variants.items():
                times[k].append(timed(f, calls))
        ms = {k: statistics.median(t) for k, t in times.items()}
        rows.append({"what": what, "nodes": v, "d1": d1, "batch": b, "negatives": K, "reps": reps, "calls_per_sample": calls,
                     "median_ms": ms, "min_ms": {k: min(t) for k, t in times.items()}, "max_ms": {k: max(t) for k, t in times.items()},
                     "bytes_moved_fused": nbytes, "fused_GBps": nbytes / ms["fused"] / 1e6, "copy_GBps": nbytes / ms["copy"] / 1e6,
                     "fused_fraction_of_copy": ms["copy"] / ms["fused"]})
        print(json.dumps(rows[-1]), flush=True)
    _lib.check(L.hm_debug_edge_loss_form(1))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "graph_embedding_probe.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "graph_embedding_probe.py measures on a GPU; there is nothing to report without one"
    graph, _ = wordnet_shaped_graph(0)
    edges = np.asarray(graph.edge_index, dtype=np.int64)
    sampler = NegativeSampler((graph.names, edges), K, seed=0, device=DEV)
    pairs_all = torch.from_numpy(np.concatenate([edges, edges[:, ::-1]], 0).copy()).to(DEV)
    gen = torch.Generator(device=DEV).manual_seed(7)
    results = []
    for d1 in WIDTHS:
        for b in BATCHES:
            results += measure(graph, sampler, pairs_all, d1, b, args.reps, args.calls, gen)
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "torch": torch.__version__,
                   "graph": {"nodes": sampler.n, "csr_entries": sampler.nnz, "note": "synthetic, WordNet noun-hypernym shape"},
                   "kernel_form": "default: one wave per sample (form 1), 4 partner rows in flight per lane group",
                   "note": "the composed sampler is torch.randint: it rejects neither the anchor nor its neighbours",
                   "results": results}, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
