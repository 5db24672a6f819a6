#!/usr/bin/env python
"""A/B of the fused graph-reconstruction counts (hyptokenizer_amd.embedding.graph_metrics) against the same
counts composed from what the library had before, on one GPU in one process.  There is no fallback: without a GPU the probe
fails.

Composed form: the evaluated nodes in slabs of ``--slab`` anchors; per slab ``batch_distance(table[slab], table)`` (the fused
HIP distance kernel, so both forms see the same fp32 distances), a boolean neighbour mask ``[slab, V]`` scattered from the
CSR, and per chunk of ``--chunk`` slots the row of the slot's anchor gathered from the slab, compared with the slot's pivot
(``<`` and ``==``), with and without the mask, and summed.  The anchor's own column is set to ``inf`` first.  The tables have no
NaN, so plain comparisons are the definitions.

Cases: the synthetic WordNet-shaped graph of tools/hierarchy_distortion_probe.py (82 115 nodes) at d + 1 in {11, 101}, every
node and a ``nodes=`` sample of 1 024 nodes; a star of the same size (the hub's segment has V - 1 slots) at d + 1 = 11; the
whole graph again at ``--sweep-widths`` (between the two, where the faster walk layout changes).  The
fused call is timed in both tile layouts where both exist (``hm_debug_recon_layout``).  The variants alternate in one process:
one warm-up each, then ``--reps`` interleaved rounds, one call between two device events per sample; median [min, max] are
reported.  The counts of the forms are compared in the same run (``equal``), and the peak memory of one call above the inputs
(table and CSR) is recorded for each.  Writes profiles/reconstruction_probe.json.

Usage:  python tools/reconstruction_probe.py [--reps 3] [--sweep-widths 17 25 33 34 65] [--out profiles/reconstruction_probe.json]
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
from hyptokenizer_amd.embedding import graph_metrics as gm  # noqa: E402
from hyptokenizer_amd.embedding import lorentz_model as lm  # noqa: E402
from hyptokenizer_amd.embedding.graph_embedding import sorted_symmetric_csr  # noqa: E402

DEV = "cuda:0"
WIDTHS, SAMPLE = (11, 101), 1024
KEYS = ("less_all", "equal_all", "less_nb", "equal_nb")


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    got = int(torch.cuda.max_memory_allocated() - base)
    del out
    return got


def composed_counts(table, row_ptr, col, nodes, slab, chunk):
    """The four count vectors [slots] of the module docstring's composed form, in the slot order of the fused call."""
    v = table.shape[0]
    nodes = torch.arange(v, device=DEV) if nodes is None else nodes
    out = [[] for _ in KEYS]
    for s0 in range(0, nodes.shape[0], slab):
        anchors = nodes[s0:s0 + slab]
        lo, hi = row_ptr[anchors], row_ptr[anchors + 1]
        deg = hi - lo
        n_slots = int(deg.sum())
        if n_slots == 0:
            continue
        local = torch.repeat_interleave(torch.arange(anchors.shape[0], device=DEV), deg)      # slab row of every slot
        first = torch.cumsum(deg, 0) - deg
        entry = lo[local] + (torch.arange(n_slots, device=DEV) - first[local])
        pivots = col[entry].long()
        dist = lm.batch_distance(table[anchors], table, 1.0, sign_convention="lorentz")
        dist[torch.arange(anchors.shape[0], device=DEV), anchors] = float("inf")
        mask = torch.zeros((anchors.shape[0], v), dtype=torch.bool, device=DEV)
        mask[local, pivots] = True
        for c0 in range(0, n_slots, chunk):
            loc = local[c0:c0 + chunk]
            rows = dist[loc]
            piv = rows.gather(1, pivots[c0:c0 + chunk, None])
            less, equal, nb = rows < piv, rows == piv, mask[loc]
            for k, t in enumerate((less, equal, less & nb, equal & nb)):
                out[k].append(t.sum(1, dtype=torch.int32))
    return [torch.cat(o) if o else torch.zeros(0, dtype=torch.int32, device=DEV) for o in out]


def measure(name, table, row_ptr, col, nodes, reps, slab, chunk):
    d1 = table.shape[1]

    def fused(layout=0):
        gm.set_walk_layout(layout)
        try:
            return gm.neighbor_rank_counts(table, row_ptr, col, nodes, validate=False)
        finally:
            gm.set_walk_layout(0)

    variants = {"fused": fused, "composed": lambda: composed_counts(table, row_ptr, col, nodes, slab, chunk)}
    if d1 >= 9:
        variants["fused_rows_in_lds"] = lambda: fused(1)
        variants["fused_anchor_in_registers"] = lambda: fused(2)
    results = {k: fn() for k, fn in variants.items()}          # the warm-up, kept for the comparison
    want = results["composed"]
    equal = {k: all(bool(torch.equal(getattr(r, key), w)) for key, w in zip(KEYS, want)) for k, r in results.items() if k != "composed"}
    slots = int(want[0].shape[0])
    stats = gm.metrics_from_counts(results["fused"])
    del results, want
    peaks = {k: peak(variants[k]) for k in ("fused", "composed")}
    times = {k: [] for k in variants}
    for _ in range(reps):
        for k, fn in variants.items():
            times[k].append(timed(fn))
    ms = {k: statistics.median(t) for k, t in times.items()}
    row = {"case": name, "nodes": table.shape[0], "d1": d1, "evaluated_nodes": table.shape[0] if nodes is None else int(nodes.shape[0]),
           "slots": slots, "walk_blocks": (slots + 63) // 64, "reps": reps, "median_ms": ms, "min_ms": {k: min(t) for k, t in times.items()},
           "max_ms": {k: max(t) for k, t in times.items()}, "speedup_over_composed": ms["composed"] / ms["fused"],
           "counts_equal_to_composed": equal, "peak_bytes_above_the_inputs": peaks,
           "fused_peak_bytes_per_slot": peaks["fused"] / max(slots, 1), "metrics": stats}
    print(json.dumps(row), flush=True)
    return row


def lorentz_rows(v, d1, gen):
    s = (torch.rand(v, d1 - 1, device=DEV, generator=gen) * 2 - 1) * 0.5 / (d1 - 1) ** 0.5
    return torch.cat([torch.sqrt(1 + (s * s).sum(-1, keepdim=True)), s], -1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--slab", type=int, default=2048)
    ap.add_argument("--chunk", type=int, default=4096)
    ap.add_argument("--sweep-widths", type=int, nargs="*", default=[17, 25, 33, 34, 65])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reconstruction_probe.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "reconstruction_probe.py measures on a GPU; there is nothing to report without one"
    graph, _ = wordnet_shaped_graph(0)
    v = len(graph.names)
    csrs = {"wordnet": sorted_symmetric_csr(v, np.asarray(graph.edge_index, dtype=np.int64)),
            "star": sorted_symmetric_csr(v, np.stack([np.zeros(v - 1, np.int64), np.arange(1, v, dtype=np.int64)], 1))}
    csrs = {k: (torch.from_numpy(r).to(DEV), torch.from_numpy(c).to(DEV)) for k, (r, c) in csrs.items()}
    gen = torch.Generator(device=DEV).manual_seed(7)
    sample = torch.randperm(v, device=DEV, generator=gen)[:SAMPLE].contiguous()
    results = []
    for d1 in WIDTHS:
        table = lorentz_rows(v, d1, gen)
        results.append(measure("wordnet", table, *csrs["wordnet"], None, args.reps, args.slab, args.chunk))
        results.append(measure(f"wordnet, nodes= sample of {SAMPLE}", table, *csrs["wordnet"], sample, args.reps, args.slab, args.chunk))
        if d1 == WIDTHS[0]:
            results.append(measure("star", table, *csrs["star"], None, args.reps, args.slab, args.chunk))
        del table
        torch.cuda.empty_cache()
    for d1 in args.sweep_widths:                              # where the default layout changes: the whole graph only
        results.append(measure("wordnet (layout sweep)", lorentz_rows(v, d1, gen), *csrs["wordnet"], None, args.reps, args.slab, args.chunk))
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "torch": torch.__version__,
                   "graph": {"nodes": v, "wordnet_csr_entries": int(csrs["wordnet"][1].shape[0]), "star_csr_entries": int(csrs["star"][1].shape[0]),
                             "note": "synthetic, WordNet noun-hypernym shape; star: node 0 joined to every other node"},
                   "composed": {"slab_anchors": args.slab, "chunk_slots": args.chunk},
                   "results": results}, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
