#!/usr/bin/env python
"""A/B of the fused Gromov-delta walk (hyptokenizer_amd.embedding.hyperbolicity) against the same quantity
composed from torch ops, and of its packed 16-bit path against its 32-bit path, on one GPU in one process.  There is no
fallback: without a GPU the probe fails.

Composed form, per base point: the product matrix ``B = D[:, w, None] + D[None, :, w] - D`` (int32, or the float32 ``A`` of the
kernel's definition), then slabs of ``torch.minimum(B[i0:i1, :, None], B[None]).amax(1)`` with the ``[slab, n, n]`` temporary
sized to ``--budget-mib``, minus ``B[i0:i1]``, and the maximum over the upper triangle.  It is timed for ONE base point at every
size (its cost is linear in the bases) and for 8 only where ``--composed-max-n`` allows.

Inputs: the int16 metric of a random connected sparse graph through ``GraphPaths.distance_rows``; the float32 distances of
``synthetic.lorentz_table`` rows through ``batch_distance``.  Sizes n in {512, 2048, 4096, 8192}, 1 and 8 base points.  The
variants alternate in one process: one warm-up each (kept: the values of all forms are compared, ``equal``), then ``--reps``
interleaved rounds, one call between two device events per sample; median [min, max] are reported, the peak memory of one
call above the input matrix for each, and the fraction of the arithmetic bound the fused call reaches: 2 VALU lane-operations
per (i <= j, k) of the tiles walked, halved on the packed path, against 256 CUs x 64 lanes x 2.4 GHz = 39.3 T lane-ops/s (an
estimate, not a measured peak).  Writes profiles/hyperbolicity_probe.json.

Usage:  python tools/hyperbolicity_probe.py [--reps 5] [--sizes 512 2048 4096 8192] [--out profiles/hyperbolicity_probe.json]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from hyptokenizer_amd import _lib  # noqa: E402
from hyptokenizer_amd.embedding import hyperbolicity as hy  # noqa: E402
from hyptokenizer_amd.embedding import lorentz_model as lm  # noqa: E402
from hyptokenizer_amd.graph_paths import GraphPaths  # noqa: E402
from hyptokenizer_amd.synthetic import lorentz_table  # noqa: E402

DEV = "cuda:0"
TILE = 128
LANE_OPS_PER_S = 256 * 64 * 2.4e9


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


def fused(d, bases, form=0):
    """The C entry point alone (no host read): the values on the device."""
    L = _lib.load()
    n = d.shape[0]
    is_int = d.dtype == torch.int16
    val = torch.empty(bases.shape[0], dtype=torch.int32 if is_int else torch.float32, device=DEV)
    wit = torch.empty((bases.shape[0], 3), dtype=torch.int32, device=DEV)
    ws = torch.empty(L.hm_gromov_workspace_bytes(n, bases.shape[0]), dtype=torch.uint8, device=DEV)
    hy.set_kernel_form(form)
    try:
        fn = L.hm_gromov_delta_i16 if is_int else L.hm_gromov_delta_f32
        _lib.check(fn(C.c_void_p(d.data_ptr()), n, d.stride(0), C.c_void_p(bases.data_ptr()), bases.shape[0], C.c_void_p(val.data_ptr()),
                      C.c_void_p(wit.data_ptr()), C.c_void_p(ws.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    finally:
        hy.set_kernel_form(0)
    return val


def composed(d, bases, budget):
    n = d.shape[0]
    is_int = d.dtype == torch.int16
    D = torch.triu(d) + torch.triu(d, 1).t()
    D = D.int() if is_int else D
    slab = max(1, budget // (n * n * 4))
    out = []
    for w in bases.tolist():
        col = D[:, w]
        if is_int:
            B = col[:, None] + col[None, :] - D
        else:
            B = 0.5 * ((col[:, None] + col[None, :]) - D) + 0.0
        best = None
        for i0 in range(0, n, slab):
            i1 = min(i0 + slab, n)
            v = torch.minimum(B[i0:i1, :, None], B[None]).amax(1) - B[i0:i1]
            v = torch.where(torch.arange(n, device=DEV)[None, :] >= torch.arange(i0, i1, device=DEV)[:, None], v, torch.full_like(v, -1))
            m = v.max()
            best = m if best is None else torch.maximum(best, m)
        out.append(best)
    return torch.stack(out)


def measure(kind, d, n_base, reps, budget, with_composed):
    n = d.shape[0]
    bases = torch.from_numpy(np.random.default_rng(n).choice(n, size=n_base, replace=False).astype(np.int32)).to(DEV)
    variants = {"fused": lambda: fused(d, bases)}
    if kind == "int16":
        variants["fused_int32_path"] = lambda: fused(d, bases, 1)
        variants["fused_packed_path"] = lambda: fused(d, bases, 2)
    if with_composed:
        variants["composed"] = lambda: composed(d, bases, budget)
    results = {k: fn() for k, fn in variants.items()}           # the warm-up, kept for the comparison
    equal = {k: bool(torch.equal(r, results["fused"])) for k, r in results.items() if k != "fused"}
    values = results["fused"].tolist()
    del results
    peaks = {k: peak(variants[k]) for k in variants if k in ("fused", "composed")}
    times = {k: [] for k in variants}
    for _ in range(reps):
        for k, fn in variants.items():
            times[k].append(timed(fn))
    ms = {k: statistics.median(t) for k, t in times.items()}
    nt = -(-n // TILE)
    pair_k = n_base * (nt * (nt + 1) // 2) * TILE * TILE * n     # (i, j, k) triples the tile kernel evaluates
    bound_ms = {"fused_int32_path" if kind == "int16" else "fused": 2 * pair_k / LANE_OPS_PER_S * 1e3}
    if kind == "int16":
        bound_ms["fused_packed_path"] = pair_k / LANE_OPS_PER_S * 1e3
    row = {"kind": kind, "n": n, "bases": n_base, "reps": reps, "median_ms": ms, "min_ms": {k: min(t) for k, t in times.items()},
           "max_ms": {k: max(t) for k, t in times.items()},
           "speedup_over_composed": ms["composed"] / ms["fused"] if with_composed else None,
           "packed_over_int32_path": ms["fused_int32_path"] / ms["fused_packed_path"] if kind == "int16" else None,
           "values_equal_to_fused": equal, "peak_bytes_above_the_matrix": peaks,
           "arithmetic_bound_ms_unmeasured_peak": bound_ms, "fraction_of_arithmetic_bound": {k: b / ms[k] for k, b in bound_ms.items()},
           "values": values}
    print(json.dumps(row), flush=True)
    return row


def graph_metric(n):
    rs = np.random.RandomState(n)
    edges = [(int(rs.randint(0, k)), k) for k in range(1, n)] + [tuple(int(v) for v in rs.randint(0, n, 2)) for _ in range(n)]
    nodes = np.arange(n)
    return GraphPaths((list(range(n)), np.array(edges, dtype=np.int64)), device=DEV).distance_rows(nodes, nodes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="*", default=[512, 2048, 4096, 8192])
    ap.add_argument("--budget-mib", type=int, default=1024)
    ap.add_argument("--composed-max-n", type=int, default=2048, help="largest n at which the composed form is also timed for 8 bases")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hyperbolicity_probe.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "hyperbolicity_probe.py measures on a GPU; there is nothing to report without one"
    results = []
    for n in args.sizes:
        x = lorentz_table(n, 10, seed=n, scale=0.5).to(DEV)
        inputs = {"int16": graph_metric(n), "fp32": lm.batch_distance(x, x, 1.0, sign_convention="lorentz")}
        for kind, d in inputs.items():
            for n_base in (1, 8):
                with_composed = n_base == 1 or n <= args.composed_max_n
                results.append(measure(kind, d, n_base, args.reps, args.budget_mib << 20, with_composed))
        del inputs, x
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "torch": torch.__version__,
                   "composed": {"budget_mib": args.budget_mib, "note": "timed for 8 bases only up to n = %d: its cost is linear in the bases" % args.composed_max_n},
                   "arithmetic_bound": "2 lane-ops per (i, j, k) of the tiles walked (1 on the packed path) over 256 CUs x 64 lanes x 2.4 GHz; an estimate, not a measured peak",
                   "results": results}, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
