#!/usr/bin/env python
"""Where FrequencyAwareHyperbolicTokenizer's time goes on the MI355X: one JSON line.

(a) corpus leg -- a seeded corpus of --lines lines, --cps code points in all (Zipf-like over the vocabulary's
    characters), written to a temporary file and counted under --rules merge rules by the device pass
    (pair_counter.count_lines_device): host reading, host encoding (symbols), upload, tokenizer kernel, counter
    (hm_pairfreq_add, device + host waits), dict build.  The host loop (the reference's) is timed on a --host-cps slice
    and scaled.
(b) step leg -- V = --vocab, d = --dim, lorentz, threshold at the --candidates-th smallest distance, --steps timed
    optimize_merges steps after --warmup; the median step split into listing, RNG, coherence kernel (coherence minus
    RNG), host scoring and sort, merge.

    python tools/frequency_probe.py --out profiles/frequency_probe.json
Kernel times: run the same command under ``rocprofv3 --kernel-trace --stats -d DIR -o probe -- python ...``.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("TQDM_DISABLE", "1")

import numpy as np  # noqa: E402
import torch  # noqa: E402


def note(msg: str) -> None:
    print(f"[frequency_probe {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


def corpus_leg(a, dev):
    from hyptokenizer_amd.synthetic import cjk_vocab, lorentz_table
    from hyptokenizer_amd.tokenizer.hyperbolic_merge import HyperbolicTokenizer
    from hyptokenizer_amd.tokenizer.pair_counter import count_lines_device, count_pair_frequencies_host, read_corpus_lines
    V = a.corpus_vocab
    vocab = cjk_vocab(V)
    tok = HyperbolicTokenizer(vocab, torch.nn.Parameter(lorentz_table(V, 4)), device=dev, max_vocab_size=V + 8,
                              sign_convention="lorentz")
    note("corpus leg: generating the corpus")
    rng = np.random.default_rng(99)
    p = 1.0 / np.arange(1, V + 1) ** 1.1
    p /= p.sum()
    per_line = a.cps // a.lines
    chars = rng.choice(V, size=a.lines * per_line, p=p).astype(np.int64) + 0x4E00
    body = chars.astype(np.uint32).tobytes()
    flat = body.decode("utf-32-le")
    lines = [flat[k * per_line:(k + 1) * per_line] for k in range(a.lines)]
    # merge rules: the most frequent adjacent character pairs of a sample
    rules, seen = [], set()
    sample = flat[:2_000_000]
    pairs = {}
    for x, y in zip(sample, sample[1:]):
        pairs[(x, y)] = pairs.get((x, y), 0) + 1
    for (x, y), _c in sorted(pairs.items(), key=lambda kv: -kv[1]):
        if len(rules) >= a.rules:
            break
        if (x, y) not in seen:
            seen.add((x, y))
            rules.append((x, y, x + y))
    tok.merge_history = rules
    note(f"{len(rules)} rules; writing and reading the file")
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "corpus.txt")
        with open(path, "w", encoding="utf-8") as f:
            f.write("\n".join(lines) + "\n")
        size = os.path.getsize(path)
        t0 = time.perf_counter()
        got_lines = read_corpus_lines(path)
        read_ms = (time.perf_counter() - t0) * 1e3
    note("device pass")
    timing, into = {}, {}
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    total = count_lines_device(tok, got_lines, into, timing=timing)
    torch.cuda.synchronize()
    device_pass_ms = (time.perf_counter() - t1) * 1e3
    note("host loop on a slice")
    # host loop on a slice, scaled
    cut, cps = [], 0
    for line in got_lines:
        if cps >= a.host_cps:
            break
        cut.append(line)
        cps += len(line)
    t2 = time.perf_counter()
    count_pair_frequencies_host(tok, cut, {})
    host_ms = (time.perf_counter() - t2) * 1e3
    host_rate = cps / (host_ms / 1e3)
    total_cps = sum(len(x) for x in got_lines)
    end_to_end = read_ms + device_pass_ms
    return {"code_points": total_cps, "lines": len(got_lines), "file_bytes": size, "rules": len(rules),
            "distinct_pairs": len(into), "total_pairs": total, "read_ms": round(read_ms, 2),
            **{k: (round(v, 3) if isinstance(v, float) else v) for k, v in timing.items()},
            "device_pass_ms": round(device_pass_ms, 2), "end_to_end_ms": round(end_to_end, 2),
            "host_loop_cps_per_s": round(host_rate), "host_loop_est_ms": round(total_cps / host_rate * 1e3, 1),
            "speedup_vs_host_loop": round(total_cps / host_rate * 1e3 / end_to_end, 1)}


def step_leg(a, dev):
    from hyptokenizer_amd.synthetic import cjk_vocab, lorentz_table
    from hyptokenizer_amd.tokenizer.frequency_aware_hyperbolic_merge import FrequencyAwareHyperbolicTokenizer
    note("step leg")
    V = a.vocab
    vocab = cjk_vocab(V)
    X = lorentz_table(V, a.dim, seed=42, scale=0.05)
    tok = FrequencyAwareHyperbolicTokenizer(vocab, torch.nn.Parameter(X), device=dev, sign_convention="lorentz",
                                            max_vocab_size=V + a.warmup + a.steps + 8)
    eng = tok._get_engine()
    dd, ii, jj, _ = eng.topk(1.0, 10.0, a.candidates)
    tok.merge_threshold = float(dd[-1])
    rng = np.random.default_rng(5)
    tok.pair_frequencies = {(vocab[i], vocab[j]): int(rng.integers(1, 1000)) for i, j in zip(ii.tolist(), jj.tolist())}
    torch.manual_seed(0)
    rows = []
    for s in range(a.warmup + a.steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tok.optimize_merges(steps=1, log_every=10 ** 9)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        if s >= a.warmup:
            t = dict(tok.last_timing)
            t["step_ms"] = ms
            t["candidates"] = len(tok._distance_candidates()[0])
            rows.append(t)
    med = sorted(rows, key=lambda r: r["step_ms"])[len(rows) // 2]
    coh_kernel = med.get("coherence_ms", 0.0) - med.get("rng_ms", 0.0)
    return {"vocab": V, "dim": a.dim, "steps": a.steps, "candidates": med["candidates"],
            "median_step_ms": round(med["step_ms"], 3), "list_ms": round(med.get("list_ms", 0.0), 3),
            "rng_ms": round(med.get("rng_ms", 0.0), 3), "coherence_kernel_ms": round(coh_kernel, 3),
            "score_sort_ms": round(med.get("score_sort_ms", 0.0), 3), "merge_ms": round(med.get("merge_ms", 0.0), 3),
            "rng_us_per_candidate": round(1e3 * med.get("rng_ms", 0.0) / max(med["candidates"], 1), 2),
            "all_steps_ms": [round(r["step_ms"], 3) for r in rows]}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--cps", type=int, default=100_000_000)
    ap.add_argument("--lines", type=int, default=1_000_000)
    ap.add_argument("--corpus-vocab", type=int, default=3000)
    ap.add_argument("--rules", type=int, default=5000)
    ap.add_argument("--host-cps", type=int, default=1_000_000)
    ap.add_argument("--vocab", type=int, default=50_000)
    ap.add_argument("--dim", type=int, default=100)
    ap.add_argument("--candidates", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--legs", default="ab")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda")
    res = {"probe": "frequency"}
    if "a" in a.legs:
        res["corpus"] = corpus_leg(a, dev)
    if "b" in a.legs:
        res["step"] = step_leg(a, dev)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
