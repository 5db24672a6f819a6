#!/usr/bin/env python
"""A/B of the fused Lorentz-centroid pooling (hyptokenizer_amd.embedding.pooling) against the same thing composed from torch
ops, on one GPU in one process.  There is no fallback: without a GPU the probe fails.

Input of every shape: the slab ``BatchEncoder.encode_device`` produces -- ids int64 [T], offsets, lengths, 0..3 positions of
slack behind the tokens of every line -- with per-token weights.  Per shape two things are timed, each as
fused / composed / composed_compact / copy:
  forward   lorentz_centroid, no gradient
  fwd_bwd   lorentz_centroid + backward of a fixed upstream gradient (sparse COO gradient on the table)
``composed`` compacts the slab (boolean mask from the lengths, which costs a read-back), runs
``F.embedding_bag(mode="sum", per_sample_weights=..., sparse=True)`` and normalises with torch ops under autograd;
``composed_compact`` is the same without the compaction, on a slab compacted beforehand.  ``copy`` is a ``copy_`` of as many
bytes as the fused kernels of that row have to move (ids, weights and gathered rows read, centroids written; for the backward
ids, weights, centroids and upstream rows read, value rows and COO indices written) -- the machine's own bandwidth yardstick.
One sample is a batch of ``--calls`` back-to-back calls between two device events divided by the number of calls; the
variants are interleaved sample by sample and the median, minimum and maximum over ``--reps`` samples are reported, with the
peak memory of one call above the inputs.  The fused backward must allocate nothing of the size of the table: its peak, less
the value rows, indices and centroids it returns, has to stay below ``V * d1 * 4`` bytes (asserted).
Rows ``kernel_*``: the two kernels alone through the C ABI on preallocated buffers, 50 launches per sample, in both work
decompositions (``hm_debug_centroid_form``); everything else runs the default choice.  Writes profiles/pooling_probe.json.

Usage:  python tools/pooling_probe.py [--reps 11] [--calls 10] [--out profiles/pooling_probe.json]
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
import torch.nn.functional as F  # noqa: E402

from hyptokenizer_amd.embedding.pooling import lorentz_centroid  # noqa: E402

DEV = "cuda:0"
#: name -> (table rows, d1, lines, length distribution)
SHAPES = {
    "v50000_w101_n1024": (50000, 101, 1024, "uniform"),
    "v50000_w101_n16384": (50000, 101, 16384, "uniform"),
    "v50000_w101_n16384_skewed": (50000, 101, 16384, "skewed"),
    "v1048576_w65_n16384": (1 << 20, 65, 16384, "uniform"),
}


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


def line_lengths(n, kind, gen):
    """About 32 tokens a line.  uniform: 24..40.  skewed: three quarters of the lines have 4..11 tokens, the rest 8..200, one
    line in 64 has 512 -- the mean stays near 32 while a wave's segments differ by two orders of magnitude."""
    if kind == "uniform":
        return torch.randint(24, 41, (n,), generator=gen)
    lens = torch.randint(4, 12, (n,), generator=gen)
    long = torch.rand(n, generator=gen) < 0.25
    lens = torch.where(long, torch.randint(8, 201, (n,), generator=gen), lens)
    lens[::64] = 512
    return lens


def make_case(v, d1, n, kind, gen):
    lens = line_lengths(n, kind, gen)
    span = lens + torch.randint(0, 4, (n,), generator=gen)
    offsets = torch.zeros(n + 1, dtype=torch.int64)
    offsets[1:] = torch.cumsum(span, 0)
    t = int(offsets[-1])
    ids = torch.randint(0, v, (t,), generator=gen)
    w = torch.rand(t, generator=gen) + 0.5
    s = (torch.rand(v, d1 - 1, generator=gen) * 2 - 1) * 0.5 / (d1 - 1) ** 0.5
    x = torch.cat([torch.sqrt(1 + (s * s).sum(-1, keepdim=True)), s], -1)
    g = torch.randn(n, d1, generator=gen)
    return tuple(a.to(DEV) for a in (x, ids, offsets, lens.to(torch.int32), w, g)), t, int(lens.sum())


def compacted(ids, offsets, lengths, w):
    t = ids.numel()
    span = offsets[1:] - offsets[:-1]
    pos = torch.arange(t, device=ids.device) - torch.repeat_interleave(offsets[:-1], span, output_size=t)
    keep = pos < torch.repeat_interleave(lengths.to(torch.int64), span, output_size=t)
    off = torch.zeros_like(offsets)
    off[1:] = torch.cumsum(lengths.to(torch.int64), 0)
    return ids[keep], off, w[keep]


def composed_centroid(table, ids, off, w):
    s = F.embedding_bag(ids, table, off[:-1], mode="sum", per_sample_weights=w, sparse=True)
    q = s[:, 0] * s[:, 0] - (s[:, 1:] * s[:, 1:]).sum(-1)
    return s / torch.sqrt(q).unsqueeze(-1)


def moved_bytes(t, live, n, d1):
    row = d1 * 4
    fwd = t * 12 + n * 20 + live * row + n * (row + 4)
    bwd = t * 12 + n * 20 + n * (2 * row + 4) + t * (row + 8)
    return {"forward": fwd, "fwd_bwd": fwd + bwd, "backward": bwd}


def measure(name, reps, calls, gen):
    v, d1, n, kind = SHAPES[name]
    (x, ids, offsets, lengths, w, g), t, live = make_case(v, d1, n, kind, gen)
    pf, pc = torch.nn.Parameter(x.clone()), torch.nn.Parameter(x.clone())
    del x
    cids, coff, cw = compacted(ids, offsets, lengths, w)

    def fused_fwd():
        with torch.no_grad():
            return lorentz_centroid(pf, ids, offsets, lengths, w, validate=False)

    def composed_fwd():
        with torch.no_grad():
            return composed_centroid(pc, *compacted(ids, offsets, lengths, w))

    def compact_fwd():
        with torch.no_grad():
            return composed_centroid(pc, cids, coff, cw)

    def fused_fb():
        pf.grad = None
        lorentz_centroid(pf, ids, offsets, lengths, w, validate=False).backward(g)

    def composed_fb():
        pc.grad = None
        composed_centroid(pc, *compacted(ids, offsets, lengths, w)).backward(g)

    def compact_fb():
        pc.grad = None
        composed_centroid(pc, cids, coff, cw).backward(g)

    agree = float((fused_fwd() - compact_fwd()).abs().max())
    fused_fb()
    compact_fb()
    gf, gc = pf.grad.coalesce(), pc.grad.coalesce()
    grad_agree = float((gf.to_dense() - gc.to_dense()).abs().max() / gc._values().abs().max())
    del gf, gc
    moved = moved_bytes(t, live, n, d1)
    rows = []
    for what, fns in (("forward", (fused_fwd, composed_fwd, compact_fwd)), ("fwd_bwd", (fused_fb, composed_fb, compact_fb))):
        n8 = max(moved[what] // 8, 1)
        src, dst = torch.empty(n8, device=DEV), torch.empty(n8, device=DEV)
        variants = {"fused": fns[0], "composed": fns[1], "composed_compact": fns[2], "copy": lambda: dst.copy_(src)}
        for fn in variants.values():
            for _ in range(3):
                fn()
        peaks = {k: peak(variants[k], (pf, pc)) for k in ("fused", "composed", "composed_compact")}
        times = {k: [] for k in variants}
        for _ in range(reps):
            for k, fn in variants.items():
                times[k].append(timed(fn, calls))
        ms = {k: statistics.median(tt) for k, tt in times.items()}
        returned = n * (d1 + 1) * 4 + (t * (d1 * 4 + 8) + n * d1 * 4 if what == "fwd_bwd" else 0)
        rows.append({"what": what, "shape": name, "table_rows": v, "d1": d1, "lines": n, "lengths": kind, "positions": t, "tokens": live,
                     "reps": reps, "calls_per_sample": calls, "median_ms": ms, "min_ms": {k: min(tt) for k, tt in times.items()},
                     "max_ms": {k: max(tt) for k, tt in times.items()}, "bytes_moved_fused": moved[what],
                     "fused_GBps": moved[what] / ms["fused"] / 1e6, "copy_GBps": moved[what] / ms["copy"] / 1e6,
                     "fused_fraction_of_copy": ms["copy"] / ms["fused"], "speedup_over_composed": ms["composed"] / ms["fused"],
                     "speedup_over_composed_compact": ms["composed_compact"] / ms["fused"], "peak_bytes_above_the_inputs": peaks,
                     "fused_peak_less_what_it_returns": peaks["fused"] - returned, "table_bytes": v * d1 * 4,
                     "max_abs_difference_of_the_centroids": agree, "relative_difference_of_the_table_gradients": grad_agree})
        assert rows[-1]["fused_peak_less_what_it_returns"] < v * d1 * 4, "the fused call allocated something of the table's size"
        print(json.dumps(rows[-1]), flush=True)
        del src, dst
    rows += kernel_rows(name, pf.detach(), ids, offsets, lengths, w, g, t, moved, reps)
    return rows


def kernel_rows(name, x, ids, offsets, lengths, w, g, t, moved, reps, calls=50):
    """The kernels alone, through the C ABI on preallocated buffers: ``calls`` back-to-back launches between two events."""
    from hyptokenizer_amd import _lib
    from hyptokenizer_amd.engine import _ptr, _stream_of
    L = _lib.load()
    v, d1 = x.shape
    n = offsets.numel() - 1
    mu, inv = torch.empty((n, d1), device=DEV), torch.empty(n, device=DEV)
    val, coo, gw = torch.empty((t, d1), device=DEV), torch.empty(t, dtype=torch.int64, device=DEV), torch.empty(t, device=DEV)
    st = _stream_of(x)

    def fwd():
        _lib.check(L.hm_centroid_fwd(_ptr(x), d1, v, d1, _ptr(ids), t, _ptr(offsets), _ptr(lengths), _ptr(w), n, _ptr(mu), _ptr(inv), st))

    def bwd(wgrad=None):
        _lib.check(L.hm_centroid_bwd(_ptr(x), d1, v, d1, _ptr(ids), t, _ptr(offsets), _ptr(lengths), _ptr(w), n, _ptr(mu), _ptr(inv),
                                     _ptr(g), _ptr(val), _ptr(coo), _ptr(wgrad), st))

    rows = []
    cases = [(f"kernel_{what}_{fname}", form, fn, nbytes) for form, fname in ((0, "group_per_segment"), (1, "wave_per_segment"))
             for what, fn, nbytes in (("forward", fwd, moved["forward"]), ("backward", bwd, moved["backward"]),
                                      ("backward_with_weight_gradient", lambda: bwd(gw), moved["backward"] + moved["forward"]))]
    for what, form, fn, nbytes in cases:
        _lib.check(L.hm_debug_centroid_form(form))
        fwd()
        src, dst = torch.empty(max(nbytes // 8, 1), device=DEV), torch.empty(max(nbytes // 8, 1), device=DEV)
        variants = {"fused": fn, "copy": lambda: dst.copy_(src)}
        for f in variants.values():
            for _ in range(3):
                f()
        times = {k: [] for k in variants}
        for _ in range(reps):
            for k, f in variants.items():
                times[k].append(timed(f, calls))
        ms = {k: statistics.median(tt) for k, tt in times.items()}
        rows.append({"what": what, "shape": name, "reps": reps, "calls_per_sample": calls, "median_ms": ms,
                     "min_ms": {k: min(tt) for k, tt in times.items()}, "max_ms": {k: max(tt) for k, tt in times.items()},
                     "bytes_moved_fused": nbytes, "fused_GBps": nbytes / ms["fused"] / 1e6, "copy_GBps": nbytes / ms["copy"] / 1e6,
                     "fused_fraction_of_copy": ms["copy"] / ms["fused"]})
        print(json.dumps(rows[-1]), flush=True)
        del src, dst
    _lib.check(L.hm_debug_centroid_form(-1))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pooling_probe.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "pooling_probe.py measures on a GPU; there is nothing to report without one"
    gen = torch.Generator().manual_seed(7)
    results = []
    for name in SHAPES:
        results += measure(name, args.reps, args.calls, gen)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "torch": torch.__version__,
                   "kernel_form": "default: chosen per call from n and the mean segment length (hm_pool.hip, pl_auto_form)",
                   "note": "composed = slab compaction + F.embedding_bag(sum, per_sample_weights, sparse) + normalisation in torch ops",
                   "results": results}, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
