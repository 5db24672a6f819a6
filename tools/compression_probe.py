#!/usr/bin/env python
"""Where a CompressionAwareTokenizer.optimize_merges step goes at V = 50 000, d = 100, lorentz.

Seeded synthetic corpus: 1 000 lines of 256 code points, each built from concatenations of near pairs (the first
candidates of the table, so that the scored merges occur in the text) and random vocabulary characters.  The
threshold is the 3 000th smallest pair distance.  Per step: candidate selection (row-range counts + listing +
argmin), the matcher call (hm_greedy_count, device time from events and the host-side call), and the rest (host
scoring, merge, cache upkeep).  Prints one JSON line (and writes it to --out).

    python tools/compression_probe.py --steps 30 --warmup 3 --out profiles/compression_probe.json
Kernel times: run the same command under ``rocprofv3 --kernel-trace --stats -d DIR -o probe -- python ...``.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("TQDM_DISABLE", "1")

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--vocab", type=int, default=50_000)
    ap.add_argument("--dim", type=int, default=100)
    ap.add_argument("--lines", type=int, default=1000)
    ap.add_argument("--line-len", type=int, default=256)
    ap.add_argument("--candidates", type=int, default=3000)
    ap.add_argument("--sample-size", type=int, default=100)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    from hyptokenizer_amd.synthetic import cjk_vocab, lorentz_table
    from hyptokenizer_amd.tokenizer.compression_aware_tokenizer import CompressionAwareTokenizer, select_row_major

    dev = torch.device("cuda")
    V = a.vocab
    vocab = cjk_vocab(V)
    X = lorentz_table(V, a.dim, seed=42, scale=0.05)
    tok = CompressionAwareTokenizer(vocab, torch.nn.Parameter(X), max_vocab_size=V + a.warmup + a.steps + 8, device=dev,
                                    sign_convention="lorentz", sample_size=a.sample_size)
    eng = tok._get_engine()
    dd = eng.topk(1.0, 10.0, a.candidates)[0]
    tok.merge_threshold = float(dd[-1])
    first, _ = select_row_major(eng, 1.0, tok._search_threshold(), 400)
    near = [vocab[i] + vocab[j] for i, j, _ in first]
    rng = np.random.default_rng(1234)
    lines = []
    for _ in range(a.lines):
        parts, size = [], 0
        while size < a.line_len:
            piece = near[int(rng.integers(len(near)))] if rng.random() < 0.5 else vocab[int(rng.integers(V))]
            parts.append(piece)
            size += len(piece)
        lines.append("".join(parts)[:a.line_len])
    tok.corpus_sample = lines

    t0 = time.perf_counter()
    tok.optimize_merges(steps=a.warmup, log_every=10 ** 9)      # first scoring: "original", matcher build
    torch.cuda.synchronize()
    warm_ms = (time.perf_counter() - t0) * 1e3

    sel, dev_ms, call_ms, step_ms = [], [], [], []
    orig = tok._best_scored

    def timed():
        hit = orig()
        t = tok.last_timing
        sel.append(t.get("select_ms", 0.0))
        dev_ms.append(t.get("matcher_device_ms", 0.0))
        call_ms.append(t.get("matcher_call_ms", 0.0))
        return hit

    tok._best_scored = timed
    for _ in range(a.steps):
        t1 = time.perf_counter()
        tok.optimize_merges(steps=1, log_every=10 ** 9)
        torch.cuda.synchronize()
        step_ms.append((time.perf_counter() - t1) * 1e3)
    del tok._best_scored

    # one scan of the table for comparison (the pair scan this step also runs, through the count / argmin calls)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    reps = 10
    for _ in range(reps):
        eng.argmin(1.0, tok._search_threshold())
    torch.cuda.synchronize()
    argmin_ms = (time.perf_counter() - t2) * 1e3 / reps

    med = lambda v: float(np.median(v)) if v else 0.0  # noqa: E731
    res = {
        "vocab": V, "dim": a.dim, "sign": "lorentz", "lines": a.lines, "line_len": a.line_len,
        "threshold": tok.merge_threshold, "sample_size": a.sample_size, "steps": a.steps, "warmup": a.warmup,
        "merges": len(tok.merge_history), "warmup_ms_total": round(warm_ms, 3),
        "ms_per_step_median": round(med(step_ms), 3), "ms_per_step_mean": round(float(np.mean(step_ms)), 3),
        "select_ms_median": round(med(sel), 3),
        "matcher_device_ms_median": round(med(dev_ms), 4),
        "matcher_call_ms_median": round(med(call_ms), 3),
        "rest_ms_median": round(med(step_ms) - med(sel) - med(call_ms), 3),
        "argmin_call_ms": round(argmin_ms, 3),
        "device": torch.cuda.get_device_name(0),
    }
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
