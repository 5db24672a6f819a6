#!/usr/bin/env python
"""Time and measure the memory of the fused retrieval calls against the same results composed from what the library had
before them, on the same GPU in the same process.

  ranks : ``retrieval_ranks`` (the default layout, and each of the rank kernel's two tile layouts forced through
          ``set_rank_layout``: A and B rows in LDS / A rows in registers with B read as 16-byte LDS broadcasts) against
          ``batch_distance`` (the whole matrix where it has at most --slab-elems entries, row slabs otherwise) followed by the torch comparisons that count, per row and per column, the entries before the
          diagonal one.  The composed form is checked to give the same ranks.
  knn   : ``hyperbolic_knn`` against ``batch_distance`` in row slabs + ``torch.topk(largest=False, sorted=True)``.
          torch.topk does not promise the index order of equal distances, so only the distance bits are compared.
          One shape is repeated under the "reference" convention, where every distance is 0 and every pair passes the k-NN's
          admission bound (the all-ties worst case of its serial list update).

Per shape: --warmup untimed rounds, then --repeats rounds in which the two forms alternate; every timing is a host clock
around work that ends in a device synchronise; peak memory is ``torch.cuda.max_memory_allocated`` above the inputs.  Each
step runs once; the first failure ends the probe, and so does the first shape that takes longer than --step-seconds (checked
when the shape returns: a call that never returns is ended by the caller, so run the probe under ``timeout -k 10 <seconds>``).  One JSON document goes to --out (median, min,
max per form and the ratio of the medians, composed / fused).

Usage:  timeout -k 10 900 python tools/retrieval_probe.py --out profiles/retrieval_probe.json
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from hyptokenizer_amd.embedding.lorentz_model import batch_distance  # noqa: E402
from hyptokenizer_amd.multimodal.retrieval import hyperbolic_knn, retrieval_ranks, set_rank_layout  # noqa: E402

SIGN = "lorentz"
#: what hipcc -Rpass-analysis=kernel-resource-usage reports for gfx950 (recorded next to the timings; not measured here).
#: blocks_per_cu: by LDS (160 KiB per CU) and registers (256 threads = one wave per SIMD and block), at the d1 / k named
KERNEL_RESOURCES = {
    "hm_retrieval_rank_kernel<0> (layout 1)": {"vgprs": 68, "scratch_bytes": 0, "waves_per_simd_by_registers": 7, "static_lds_bytes": 2048,
                                               "dynamic_lds_bytes": "4 * (2 * 64 * (d1 | 1) + 136)", "blocks_per_cu": {"d1=65": 4, "d1=129": 2}},
    "hm_retrieval_rank_kernel<32> (layout 2, d1 <= 33)": {"vgprs": 104, "scratch_bytes": 0, "waves_per_simd_by_registers": 4,
                                                          "static_lds_bytes": 2048, "dynamic_lds_bytes": 4 * 64 * 36, "blocks_per_cu": 4},
    "hm_retrieval_rank_kernel<64> (layout 2, d1 <= 65)": {"vgprs": 145, "scratch_bytes": 0, "waves_per_simd_by_registers": 3,
                                                          "static_lds_bytes": 2048, "dynamic_lds_bytes": 4 * 64 * 68, "blocks_per_cu": 3},
    "hm_retrieval_rank_kernel<128> (layout 2, d1 <= 129)": {"vgprs": 213, "scratch_bytes": 0, "waves_per_simd_by_registers": 2,
                                                            "static_lds_bytes": 2048, "dynamic_lds_bytes": 4 * 64 * 132, "blocks_per_cu": 2},
    "hm_knn_kernel": {"vgprs": 79, "scratch_bytes": 0, "waves_per_simd_by_registers": 6, "static_lds_bytes": 1536,
                      "dynamic_lds_bytes": "4 * (2 * 64 * (d1 | 1) + 64 * 65 + 2 * 64 * (k | 1))",
                      "blocks_per_cu": {"d1=65,k=10": 2, "d1=129,k=128": 1}},
}


def with_layout(layout, fn):
    def run():
        set_rank_layout(layout)
        try:
            return fn()
        finally:
            set_rank_layout(0)
    return run


def make_pairs(n, d, seed, dev):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(n, d + 1, generator=g) * 0.3
    b = a + torch.randn(n, d + 1, generator=g) * 0.7
    for t in (a, b):
        t[:, 0] = torch.sqrt(1.0 + (t[:, 1:] ** 2).sum(-1))
    return a.to(dev), b.to(dev)


def composed_ranks(zt, zi, slab_elems):
    n = zt.shape[0]
    idx = torch.arange(n, device=zt.device)
    rows = max(1, min(n, slab_elems // n))
    rank_r = torch.empty(n, dtype=torch.int64, device=zt.device)
    rank_c = torch.empty(n, dtype=torch.int64, device=zt.device)
    if rows == n:
        D = batch_distance(zt, zi, 1.0, sign_convention=SIGN)
        diag = D.diagonal()
        rank_r = (D < diag[:, None]).sum(1) + ((D == diag[:, None]) & (idx[None, :] < idx[:, None])).sum(1)
        rank_c = (D < diag[None, :]).sum(0) + ((D == diag[None, :]) & (idx[:, None] < idx[None, :])).sum(0)
        return rank_r, rank_c
    for s in range(0, n, rows):
        own = idx[s:s + rows]
        loc = torch.arange(own.numel(), device=zt.device)
        D = batch_distance(zt[s:s + rows], zi, 1.0, sign_convention=SIGN)
        diag = D[loc, own]
        rank_r[s:s + rows] = (D < diag[:, None]).sum(1) + ((D == diag[:, None]) & (idx[None, :] < own[:, None])).sum(1)
        D = batch_distance(zt, zi[s:s + rows], 1.0, sign_convention=SIGN)
        diag = D[own, loc]
        rank_c[s:s + rows] = (D < diag[None, :]).sum(0) + ((D == diag[None, :]) & (idx[:, None] < own[None, :])).sum(0)
    return rank_r, rank_c


def composed_knn(q, keys, k, exclude_self, slab_elems, sign=SIGN):
    nq, nk = q.shape[0], keys.shape[0]
    rows = max(1, min(nq, slab_elems // nk))
    out_d = torch.empty((nq, k), dtype=torch.float32, device=q.device)
    out_i = torch.empty((nq, k), dtype=torch.int64, device=q.device)
    for s in range(0, nq, rows):
        D = batch_distance(q[s:s + rows], keys, 1.0, sign_convention=sign)
        if exclude_self:
            own = torch.arange(s, min(s + rows, nq), device=q.device)
            own = own[own < nk]
            D[own - s, own] = float("inf")
        out_d[s:s + rows], out_i[s:s + rows] = torch.topk(D, k, dim=1, largest=False, sorted=True)
    return out_d, out_i


def timed(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    return ms, torch.cuda.max_memory_allocated() - base, out


def measure(forms, warmup, repeats):
    for _ in range(warmup):
        for fn in forms.values():
            timed(fn)
    runs = {k: [] for k in forms}
    last = {}
    for _ in range(repeats):
        for name, fn in forms.items():                   # interleaved
            ms, peak, out = timed(fn)
            runs[name].append((ms, peak))
            last[name] = out
    stats = {}
    for name, rr in runs.items():
        ms = [r[0] for r in rr]
        stats[name] = {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms),
                       "peak_extra_bytes": max(r[1] for r in rr), "runs": len(rr)}
    return stats, last


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rank-sizes", type=int, nargs="*", default=[1024, 5000, 8192, 16384, 65536])
    ap.add_argument("--knn-shapes", type=str, nargs="*", default=["16384,16384,10,0", "1000,50000,100,0", "50000,50000,50,1"],
                    help="Q,N,k,exclude_self")
    ap.add_argument("--dims", type=int, nargs="+", default=[64, 100], help="d of the k-NN shapes (ranks use the first)")
    ap.add_argument("--slab-elems", type=int, default=1 << 28, help="largest distance matrix (entries) the composed form builds at once")
    ap.add_argument("--item-loop-rows", type=int, default=32, help="rows of the B = 1024 per-pair .item() loop to time (0: skip)")
    ap.add_argument("--step-seconds", type=float, default=240.0, help="a shape that takes longer than this ends the probe")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "retrieval_probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("retrieval_probe.py needs a HIP device; nothing is measured without one")
    dev = torch.device("cuda:0")
    doc = {"tool": "tools/retrieval_probe.py", "device": torch.cuda.get_device_name(0), "warmup": args.warmup, "repeats": args.repeats,
           "sign_convention": SIGN, "slab_elems": args.slab_elems, "kernel_resources": KERNEL_RESOURCES, "ranks": [], "knn": []}
    clock = {"t": time.perf_counter()}

    def step_done(what):
        now = time.perf_counter()
        took, clock["t"] = now - clock["t"], now
        if took > args.step_seconds:
            sys.exit(f"{what} took {took:.0f} s, more than --step-seconds = {args.step_seconds:.0f}")


    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)

    for B in args.rank_sizes:
        zt, zi = make_pairs(B, args.dims[0], B, dev)
        fused = lambda: retrieval_ranks(zt, zi, sign_convention=SIGN)  # noqa: E731
        stats, last = measure({"fused_hip": fused, "fused_lds_layout": with_layout(1, fused), "fused_reg_layout": with_layout(2, fused),
                               "composed": lambda: composed_ranks(zt, zi, args.slab_elems)}, args.warmup, args.repeats)
        same = all(torch.equal(f.long(), c) for name in ("fused_hip", "fused_lds_layout", "fused_reg_layout")
                   for f, c in zip(last[name], last["composed"]))
        entry = {"B": B, "d": args.dims[0], "same_ranks": bool(same), "r@1_text2image": float((last["fused_hip"][0] < 1).sum()) / B,
                 "ratio_composed_over_fused": stats["composed"]["ms_median"] / stats["fused_hip"]["ms_median"],
                 "ratio_lds_layout_over_reg_layout": stats["fused_lds_layout"]["ms_median"] / stats["fused_reg_layout"]["ms_median"], **stats}
        print(json.dumps(entry), flush=True)
        doc["ranks"].append(entry)
        save()
        if not same:
            sys.exit(f"ranks differ at B = {B}")
        step_done(f"ranks at B = {B}")
    if args.item_loop_rows > 0:
        # context only: the shape of the reference's loop (one distance call and one .item() per pair), on this library's
        # own row-wise distance; timed over the first --item-loop-rows rows of a B = 1024 table and scaled to B^2 calls
        from hyptokenizer_amd.embedding.lorentz_model import distance
        B, rows = 1024, min(args.item_loop_rows, 1024)
        zt, zi = make_pairs(B, args.dims[0], B, dev)
        ms, _, _ = timed(lambda: [distance(zt[i].unsqueeze(0), zi[j].unsqueeze(0), sign_convention=SIGN).item()
                                  for i in range(rows) for j in range(B)])
        doc["item_loop"] = {"B": B, "d": args.dims[0], "rows_timed": rows, "calls_timed": rows * B, "ms_timed": ms,
                            "us_per_call": ms * 1e3 / (rows * B), "ms_scaled_to_B_squared_calls": ms * B / rows}
        print(json.dumps(doc["item_loop"]), flush=True)
        save()
        step_done("the per-pair loop")
    for shape in args.knn_shapes:
        nq, nk, k, ex = (int(v) for v in shape.split(","))
        for d in args.dims:
            q, keys = make_pairs(max(nq, nk), d, nq + nk + d, dev)
            q, keys = q[:nq], keys[:nk]
            stats, last = measure({"fused_hip": lambda: hyperbolic_knn(q, keys, k, sign_convention=SIGN, exclude_self=bool(ex)),
                                   "composed": lambda: composed_knn(q, keys, k, bool(ex), args.slab_elems)}, args.warmup, args.repeats)
            same = torch.equal(last["fused_hip"][0].view(torch.int32), last["composed"][0].view(torch.int32))
            entry = {"Q": nq, "N": nk, "k": k, "exclude_self": bool(ex), "d": d, "same_distance_bits": bool(same),
                     "ratio_composed_over_fused": stats["composed"]["ms_median"] / stats["fused_hip"]["ms_median"], **stats}
            print(json.dumps(entry), flush=True)
            doc["knn"].append(entry)
            save()
            if not same:
                sys.exit(f"k-NN distances differ at {shape}, d = {d}")
            step_done(f"k-NN at {shape}, d = {d}")
    if args.knn_shapes:
        # the all-ties worst case: under "reference" every distance is 0, every pair passes the admission bound
        nq, nk, k, ex = (int(v) for v in args.knn_shapes[0].split(","))
        d = args.dims[0]
        q, keys = make_pairs(max(nq, nk), d, 7, dev)
        q, keys = q[:nq], keys[:nk]
        stats, last = measure({"fused_hip": lambda: hyperbolic_knn(q, keys, k, sign_convention="reference", exclude_self=bool(ex)),
                               "composed": lambda: composed_knn(q, keys, k, bool(ex), args.slab_elems, "reference")}, args.warmup, args.repeats)
        same = torch.equal(last["fused_hip"][0].view(torch.int32), last["composed"][0].view(torch.int32))
        doc["knn_all_ties"] = {"Q": nq, "N": nk, "k": k, "exclude_self": bool(ex), "d": d, "sign_convention": "reference",
                               "same_distance_bits": bool(same),
                               "ratio_composed_over_fused": stats["composed"]["ms_median"] / stats["fused_hip"]["ms_median"], **stats}
        print(json.dumps(doc["knn_all_ties"]), flush=True)
        save()
        if not same:
            sys.exit("k-NN distances differ in the all-ties case")


if __name__ == "__main__":
    main()
