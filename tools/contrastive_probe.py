#!/usr/bin/env python
"""Time and measure the memory of forward + backward of the fused hyperbolic InfoNCE loss against the reference's
expression written in torch on the same GPU.

The torch form is the reference's algorithm as it stands (multimodal/contrastive_loss.py:36-58): a B x B matrix filled
by a Python loop of B row-wise ``distance`` expressions, then cross-entropy in both directions; "lorentz" sign.  Per
batch size B in --sizes (d = --dim): --warmup untimed rounds, then --repeats rounds in which the two forms alternate;
every timing is a host clock around work that ends in a device synchronise; peak memory is
``torch.cuda.max_memory_allocated`` above the inputs.  One JSON document goes to --out (median, min, max per form).

Usage:  python tools/contrastive_probe.py --out profiles/contrastive_probe.json
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

from hyptokenizer_amd.multimodal.contrastive_loss import hyperbolic_contrastive_loss  # noqa: E402


def torch_loop_loss(zt, zi, temp):
    B = zt.size(0)
    dist = torch.zeros((B, B), device=zt.device)
    for i in range(B):
        x = zt[i].unsqueeze(0).expand(B, -1)
        u = x[..., 0] * zi[..., 0] - torch.sum(x[..., 1:] * zi[..., 1:], dim=-1)
        dist[i] = torch.acosh(torch.clamp(u, min=1.0 + 1e-8))
    s = -dist / temp
    labels = torch.arange(B, device=zt.device)
    ce = torch.nn.functional.cross_entropy
    return (ce(s, labels) + ce(s.t(), labels)) / 2.0


def one_round(fn, zt, zi, temp):
    zt.grad = zi.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    t0 = time.perf_counter()
    loss = fn(zt, zi, temp)
    loss.backward()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    return ms, torch.cuda.max_memory_allocated() - base, float(loss.detach()), zt.grad.clone()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 4096, 16384])
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--temp", type=float, default=0.5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "contrastive_probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("contrastive_probe.py needs a HIP device; nothing is measured without one")
    dev = torch.device("cuda:0")
    forms = {"fused_hip": lambda a, b, t: hyperbolic_contrastive_loss(a, b, temp=t, sign_convention="lorentz"),
             "torch_loop": torch_loop_loss}
    results = []
    for B in args.sizes:
        g = torch.Generator().manual_seed(B)
        scale = 1.0 / args.dim ** 0.5
        a = torch.randn(B, args.dim + 1, generator=g) * scale
        b = a + torch.randn(B, args.dim + 1, generator=g) * 0.5 * scale
        for t in (a, b):
            t[:, 0] = torch.sqrt(1.0 + (t[:, 1:] ** 2).sum(-1))
        zt, zi = a.to(dev).requires_grad_(), b.to(dev).requires_grad_()
        for _ in range(args.warmup):
            for fn in forms.values():
                one_round(fn, zt, zi, args.temp)
        runs = {k: [] for k in forms}
        last = {}
        for _ in range(args.repeats):
            for name, fn in forms.items():               # interleaved
                ms, peak, loss, grad = one_round(fn, zt, zi, args.temp)
                runs[name].append({"ms": ms, "peak_extra_bytes": peak})
                last[name] = (loss, grad)
        gdiff = float((last["fused_hip"][1] - last["torch_loop"][1]).abs().max() / last["torch_loop"][1].abs().max())
        entry = {"B": B, "d": args.dim, "temp": args.temp, "loss_fused": last["fused_hip"][0], "loss_torch": last["torch_loop"][0],
                 "grad_max_rel_diff": gdiff}
        for name, rr in runs.items():
            ms = [r["ms"] for r in rr]
            entry[name] = {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms),
                           "peak_extra_bytes": max(r["peak_extra_bytes"] for r in rr), "runs": len(rr)}
        print(json.dumps(entry), flush=True)
        results.append(entry)
    doc = {"tool": "tools/contrastive_probe.py", "device": torch.cuda.get_device_name(0), "warmup": args.warmup,
           "repeats": args.repeats, "results": results}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
