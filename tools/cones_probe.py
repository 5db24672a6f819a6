#!/usr/bin/env python
"""A/B of the fused entailment-cone step (hyptokenizer_amd.embedding.entailment_cones) against the same loss composed from
torch ops, on one GPU in one process.  There is no fallback: without a GPU the probe fails.

Graph: the synthetic WordNet-shaped graph of tools/hierarchy_distortion_probe.py (82 115 nodes), its edges as (parent, child)
pairs.  Per shape (d1 in {11, 101}, B in {1 024, 16 384}, K = 50) and per apex role three things are timed, each as
fused / composed / copy:
  forward   entailment_cone_loss, no gradient         | gather table[index] + the expressions of DESIGN.md 5.21 in fp32
  fwd_bwd   loss + backward (sparse COO gradient)     | the same under autograd: a dense [V, d1] gradient by index_put
  step      sampler + fwd_bwd + RiemannianSGD.step    | randint + fwd_bwd + RiemannianSGD.step on the dense gradient
``composed`` is the fp32 truth expression of tests/cones_cases.py written for the device (gather, a dozen elementwise launches,
``acos`` / ``asin`` and autograd's saved copies), not this code.  ``copy`` is a ``copy_`` of as many bytes as the fused kernels
of that row have to move (index read, partner rows gathered, weights, values and COO indices written; for ``step`` also the
sampler's and the optimiser's rows) -- the machine's own bandwidth yardstick.  One sample is a batch of ``--calls`` back-to-back
calls between two device events divided by the number of calls; the three variants are interleaved sample by sample and the
median, minimum and maximum over ``--reps`` samples are reported, with the peak memory of one call above the table.  The
learning rate is tiny so that the table stays where it started.  ``apex="partner"`` is given the pairs reversed, as the training
loop does.  Rows ``kernel_*``: the two kernels alone through the C ABI on preallocated buffers, 50 launches per sample, in both
work decompositions (``hm_debug_cone_loss_form``); everything else runs the default form.  Writes profiles/cones_probe.json.

Usage:  python tools/cones_probe.py [--reps 11] [--calls 10] [--out profiles/cones_probe.json]
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

from graph_embedding_probe import peak, timed  # noqa: E402
from hierarchy_distortion_probe import wordnet_shaped_graph  # noqa: E402
from hyptokenizer_amd.embedding.entailment_cones import ROLES, entailment_cone_loss  # noqa: E402
from hyptokenizer_amd.embedding.graph_embedding import NegativeSampler  # noqa: E402
from hyptokenizer_amd.optim import RiemannianSGD  # noqa: E402

DEV = "cuda:0"
WIDTHS, BATCHES, K, LR = (11, 101), (1024, 16384), 50, 1e-6
MARGIN, APERTURE_K = 0.01, 0.1
A_MAX, S_MAX = 1.0 - 2.0 ** -20, 1.0 - 2.0 ** -10


def composed_loss(table, index, apex):
    """tests/cones_cases.cone_terms in fp32 on the device, summed: every index of the probe is in range."""
    x = table[index]
    xu, xk = x[:, :1], x[:, 1:]
    a, b = (xu, xk) if apex == "anchor" else (xk, xu)
    u = xu[..., 0] * xk[..., 0] - (xu[..., 1:] * xk[..., 1:]).sum(-1)
    nn = (a[..., 1:] * a[..., 1:]).sum(-1).expand_as(u)
    flat = (index[:, 1:] == index[:, :1]) | ~(u > 1) | ~(nn > 0)
    us = torch.where(flat, 2.0, u)
    n = torch.sqrt(torch.where(nn > 0, nn, 1.0))
    A = (b[..., 0] - a[..., 0] * us) / (n * torch.sqrt(us * us - 1))
    ca = ~(A.abs() <= A_MAX)
    ext = torch.where(ca, torch.where(A.detach() > 0, float(np.arccos(A_MAX)), float(np.arccos(-A_MAX))), torch.acos(torch.where(ca, 0.0, A)))
    s = (2.0 * APERTURE_K) / n
    cs = ~(s < S_MAX)
    m = ext - torch.where(cs, float(np.arcsin(S_MAX)), torch.asin(torch.where(cs, 0.0, s)))
    E = torch.where(flat | ~(m > 0), 0.0, m)
    hinge = torch.where(MARGIN - E > 0, MARGIN - E, 0.0)
    return (E[:, 0] + hinge[:, 1:].sum(1)).sum()


def moved_bytes(b, d1):
    slots, row = b * (2 + K), d1 * 4
    fwd = slots * (8 + row) + b * (1 + K) * 16 + b * 4
    bwd = slots * (8 + row) + b * (1 + K) * 16 + b * 4 + slots * (row + 8)
    sampler = b * 16 + slots * 8
    return {"forward": fwd, "fwd_bwd": fwd + bwd, "step": sampler + fwd + bwd + slots * (8 + 3 * row)}


def measure(sampler, pairs_all, d1, b, apex, reps, calls, gen):
    v = sampler.n
    s = (torch.rand(v, d1 - 1, device=DEV, generator=gen) * 2 - 1) / (d1 - 1) ** 0.5
    x0 = torch.cat([torch.sqrt(1 + (s * s).sum(-1, keepdim=True)), s], -1)
    pairs = pairs_all[torch.randperm(pairs_all.shape[0], device=DEV, generator=gen)[:b]]
    pairs = (pairs if apex == "anchor" else pairs[:, [1, 0]]).contiguous()
    index = sampler.sample(pairs, 0)
    pf, pc = torch.nn.Parameter(x0.clone()), torch.nn.Parameter(x0.clone())
    of, oc = RiemannianSGD([pf], lr=LR), RiemannianSGD([pc], lr=LR)
    state = {"step": 0}
    kw = dict(margin=MARGIN, aperture_k=APERTURE_K, apex=apex, reduction="sum", validate=False)

    def composed_index():
        return torch.cat([pairs, torch.randint(0, v, (b, K), device=DEV)], 1)

    def fused_fb(idx=index):
        pf.grad = None
        entailment_cone_loss(pf, idx, **kw).backward()

    def composed_fb(idx=index):
        pc.grad = None
        composed_loss(pc, idx, apex).backward()

    def fused_step():
        state["step"] += 1
        fused_fb(sampler.sample(pairs, state["step"]))
        of.step()

    def composed_step():
        composed_fb(composed_index())
        oc.step()

    def fused_fwd():
        with torch.no_grad():
            return entailment_cone_loss(pf, index, **kw)

    def composed_fwd():
        with torch.no_grad():
            return composed_loss(pc, index, apex)

    with torch.no_grad():                                     # before any step: the two forms of the loss agree
        agree = float((fused_fwd() - composed_fwd()).abs() / composed_fwd().abs().clamp(min=1e-30))

    pairs_of = {"forward": (fused_fwd, composed_fwd), "fwd_bwd": (fused_fb, composed_fb), "step": (fused_step, composed_step)}
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
        rows.append({"what": what, "apex": apex, "nodes": v, "d1": d1, "batch": b, "negatives": K, "reps": reps, "calls_per_sample": calls,
                     "median_ms": ms, "min_ms": {k: min(t) for k, t in times.items()}, "max_ms": {k: max(t) for k, t in times.items()},
                     "bytes_moved_fused": moved[what], "fused_GBps": moved[what] / ms["fused"] / 1e6,
                     "copy_GBps": moved[what] / ms["copy"] / 1e6, "fused_fraction_of_copy": ms["copy"] / ms["fused"],
                     "speedup_over_composed": ms["composed"] / ms["fused"], "peak_bytes_above_the_table": peaks})
        print(json.dumps(rows[-1]), flush=True)
    rows += kernel_rows(x0, index, b, d1, v, apex, moved, reps)
    for r in rows:
        r["relative_difference_of_the_two_losses_before_the_run"] = agree
    return rows


def kernel_rows(x, index, b, d1, v, apex, moved, reps, calls=50):
    """The two kernels alone, through the C ABI on preallocated buffers: ``calls`` back-to-back launches between two events,
    so that what is timed is the device (or, below a few microseconds per kernel, the launch rate)."""
    from hyptokenizer_amd import _lib
    from hyptokenizer_amd.engine import _ptr, _stream_of
    L = _lib.load()
    loss, w, gl = torch.empty(b, device=DEV), torch.empty((b, 1 + K, 4), device=DEV), torch.ones(b, device=DEV)
    val = torch.empty((b * (2 + K), d1), device=DEV)
    coo = torch.empty(b * (2 + K), dtype=torch.int64, device=DEV)
    st, role = _stream_of(x), ROLES[apex]

    def fwd():
        _lib.check(L.hm_cone_loss_fwd(_ptr(x), d1, v, d1, _ptr(index), b, K, APERTURE_K, MARGIN, role, _ptr(loss), _ptr(w), st))

    def bwd():
        _lib.check(L.hm_cone_loss_bwd(_ptr(x), d1, v, d1, _ptr(index), b, K, APERTURE_K, MARGIN, role, _ptr(w), _ptr(gl), _ptr(val),
                                      _ptr(coo), st))

    rows = []
    cases = [(f"kernel_{what}_{name}", form, fn, nbytes) for form, name in ((0, "group_per_sample"), (1, "wave_per_sample"))
             for what, fn, nbytes in (("forward", fwd, moved["forward"]), ("backward", bwd, moved["fwd_bwd"] - moved["forward"]))]
    for what, form, fn, nbytes in cases:
        _lib.check(L.hm_debug_cone_loss_form(form))
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
        rows.append({"what": what, "apex": apex, "nodes": v, "d1": d1, "batch": b, "negatives": K, "reps": reps, "calls_per_sample": calls,
                     "median_ms": ms, "min_ms": {k: min(t) for k, t in times.items()}, "max_ms": {k: max(t) for k, t in times.items()},
                     "bytes_moved_fused": nbytes, "fused_GBps": nbytes / ms["fused"] / 1e6, "copy_GBps": nbytes / ms["copy"] / 1e6,
                     "fused_fraction_of_copy": ms["copy"] / ms["fused"]})
        print(json.dumps(rows[-1]), flush=True)
    _lib.check(L.hm_debug_cone_loss_form(1))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cones_probe.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "cones_probe.py measures on a GPU; there is nothing to report without one"
    graph, _ = wordnet_shaped_graph(0)
    edges = np.asarray(graph.edge_index, dtype=np.int64)
    sampler = NegativeSampler((graph.names, edges), K, seed=0, device=DEV)
    pairs_all = torch.from_numpy(edges.copy()).to(DEV)
    gen = torch.Generator(device=DEV).manual_seed(7)
    results = []
    for d1 in WIDTHS:
        for b in BATCHES:
            for apex in ROLES:
                results += measure(sampler, pairs_all, d1, b, apex, args.reps, args.calls, gen)
                torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "torch": torch.__version__,
                   "graph": {"nodes": sampler.n, "csr_entries": sampler.nnz, "note": "synthetic, WordNet noun-hypernym shape"},
                   "kernel_form": "default: one wave per sample (form 1), 4 partner rows in flight per lane group",
                   "loss": {"margin": MARGIN, "aperture_k": APERTURE_K},
                   "note": "the composed sampler is torch.randint: it rejects neither the anchor nor its neighbours",
                   "results": results}, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
