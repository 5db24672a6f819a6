#!/usr/bin/env python
"""What the corpus metrics of a tokenizer cost on the MI355X, new path against the ways the code allowed before: one JSON line.

Workload: a seeded corpus of --lines lines of --cps / --lines code points (Zipf-like over a CJK vocabulary, as
tools/frequency_probe.py builds it) under --rules merge rules.

* ``kernel``: ``hm_tokstats`` alone on the token stream of the first slab, event-timed, interleaved with a ``copy_`` of a
  tensor of the same number of bytes (--repeats rounds after --warmup; median / min / max).  The kernel reads its bytes
  once; the copy reads and writes them, so its traffic is twice the size.  The per-line output and a one-block-per-CU
  grid are timed beside it.
* ``encoder``: ``hm_tokenize_batch`` on the same slab (with its length sort), event-timed.
* ``corpus_statistics``: wall time of the whole call on all lines (host symbols, upload, encoder, statistics), and its
  event-timed kernel shares.
* ``tokenize_batch_then_host_loop``: the same integers the way the previous code allowed -- ``tokenize_batch`` (tokens to
  the host as Python strings), then the counting loop -- on the first --parent-lines lines, scaled to all lines.
* ``per_line_tokenize``: ``tok.tokenize`` line by line plus the counting loop on --host-lines lines, scaled.
* ``small_corpora``: wall time of the device path against the per-line host loop on 1 ... 10 000 lines (where the fixed
  cost of the device path shows).

    python tools/corpus_stats_probe.py --out profiles/corpus_stats_probe.json
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
os.environ.setdefault("TQDM_DISABLE", "1")

import numpy as np  # noqa: E402
import torch  # noqa: E402


def note(msg: str) -> None:
    print(f"[corpus_stats_probe {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4), "n": len(xs)}


def build(a, dev):
    from hyptokenizer_amd.synthetic import cjk_vocab, lorentz_table
    from hyptokenizer_amd.tokenizer.hyperbolic_merge import HyperbolicTokenizer
    V = a.corpus_vocab
    vocab = cjk_vocab(V)
    tok = HyperbolicTokenizer(vocab, torch.nn.Parameter(lorentz_table(V, 4)), device=dev, max_vocab_size=V + 8,
                              sign_convention="lorentz")
    rng = np.random.default_rng(99)
    p = 1.0 / np.arange(1, V + 1) ** 1.1
    p /= p.sum()
    per_line = a.cps // a.lines
    chars = rng.choice(V, size=a.lines * per_line, p=p).astype(np.int64) + 0x4E00
    flat = chars.astype(np.uint32).tobytes().decode("utf-32-le")
    lines = [flat[k * per_line:(k + 1) * per_line] for k in range(a.lines)]
    rules, pairs = [], {}
    sample = flat[:2_000_000]
    for x, y in zip(sample, sample[1:]):
        pairs[(x, y)] = pairs.get((x, y), 0) + 1
    for (x, y), _c in sorted(pairs.items(), key=lambda kv: -kv[1])[:a.rules]:
        rules.append((x, y, x + y))
    tok.merge_history = rules
    return tok, lines


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def kernel_leg(a, tok, lines, dev):
    from hyptokenizer_amd.tokenizer import corpus_stats as CS
    enc = tok._batch_encoder()
    attr, wordmap = CS._device_tables(tok, enc)
    start, stop = next(CS._slabs(lines, CS.DEFAULT_BATCH_LINES, CS.SLAB_CODE_POINTS))
    sym_h, off_h = enc.symbols(lines[start:stop])
    sym, off = torch.from_numpy(sym_h).to(dev), torch.from_numpy(off_h).to(dev)
    lens = off[1:] - off[:-1]

    def encode():
        order = torch.argsort(lens, descending=True, stable=True)
        return enc.run(sym, off, order)

    out, out_len, _ = encode()
    out_len = out_len.contiguous()
    n_bytes = out.numel() * 4 + off.numel() * 8 + out_len.numel() * 4
    src = torch.empty(n_bytes, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    forms = {
        "stats": lambda: CS.token_statistics(out, off, out_len, attr, wordmap),
        "copy": lambda: dst.copy_(src),
        "stats_per_line": lambda: CS.token_statistics(out, off, out_len, attr, wordmap, per_line=True),
        "stats_one_block_per_cu": lambda: CS.token_statistics(out, off, out_len, attr, wordmap,
                                                              max_blocks=torch.cuda.get_device_properties(dev).multi_processor_count),
        "encoder": encode,
    }
    ms = {k: [] for k in forms}
    for r in range(a.warmup + a.repeats):          # interleaved: every round times every form once
        for k, fn in forms.items():
            t, _ = timed(fn)
            if r >= a.warmup:
                ms[k].append(t)
    totals = CS.token_statistics(out, off, out_len, attr, wordmap)[0].cpu().tolist()
    res = {"slab_lines": stop - start, "positions": int(out.numel()), "tokens": totals[0], "bytes_read": n_bytes,
           "attr_table_bytes": int(attr.numel()) * 4}
    for k, v in ms.items():
        res[k + "_ms"] = spread(v)
    res["stats_GBps_read"] = round(n_bytes / statistics.median(ms["stats"]) / 1e6, 1)
    res["copy_GBps_read_plus_written"] = round(2 * n_bytes / statistics.median(ms["copy"]) / 1e6, 1)
    res["stats_over_copy_time"] = round(statistics.median(ms["stats"]) / statistics.median(ms["copy"]), 3)
    return res


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--cps", type=int, default=100_000_000)
    ap.add_argument("--lines", type=int, default=1_000_000)
    ap.add_argument("--corpus-vocab", type=int, default=3000)
    ap.add_argument("--rules", type=int, default=5000)
    ap.add_argument("--parent-lines", type=int, default=100_000)
    ap.add_argument("--host-lines", type=int, default=5_000)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from hyptokenizer_amd.tokenizer import corpus_stats as CS
    dev = torch.device("cuda:0")
    note("building the corpus")
    tok, lines = build(a, dev)
    res = {"probe": "corpus_stats", "device": torch.cuda.get_device_name(0), "lines": len(lines),
           "code_points": sum(map(len, lines)), "rules": len(tok.merge_history)}
    note("kernel leg")
    res["kernel"] = kernel_leg(a, tok, lines, dev)

    note("whole call")
    walls, timing = [], {}
    for c in range(a.calls + 1):                    # the first call is the warm-up (tables, allocator)
        timing = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st = CS.corpus_statistics_device(tok, lines, timing=timing)
        torch.cuda.synchronize()
        if c:
            walls.append((time.perf_counter() - t0) * 1e3)
    res["corpus_statistics"] = {"wall_ms": spread(walls), "encode_kernel_ms": round(timing["encode_kernel_ms"], 3),
                                "stats_kernel_ms": round(timing["stats_kernel_ms"], 3), "slabs": timing["slabs"],
                                "statistics": st.__dict__}

    note("tokenize_batch, then the host loop")
    sub = lines[:a.parent_lines]
    scale = len(lines) / len(sub)
    tok.tokenize_batch(sub[:1000])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    toks = tok.tokenize_batch(sub)
    t1 = time.perf_counter()
    by_line = iter(toks)
    parent = CS.corpus_statistics_host(lambda _text: next(by_line), sub)
    t2 = time.perf_counter()
    want = CS.corpus_statistics_device(tok, sub)
    res["tokenize_batch_then_host_loop"] = {
        "lines": len(sub), "tokenize_batch_ms": round((t1 - t0) * 1e3, 1), "host_loop_ms": round((t2 - t1) * 1e3, 1),
        "scaled_to_all_lines_ms": round((t2 - t0) * 1e3 * scale, 1), "same_integers": parent == want}
    del toks

    note("per-line tokenize")
    sub = lines[:a.host_lines]
    t0 = time.perf_counter()
    host = CS.corpus_statistics_host(tok.tokenize, sub)
    t1 = time.perf_counter()
    res["per_line_tokenize"] = {"lines": len(sub), "ms": round((t1 - t0) * 1e3, 1),
                                "scaled_to_all_lines_ms": round((t1 - t0) * 1e3 * len(lines) / len(sub), 1),
                                "same_integers": host == CS.corpus_statistics_device(tok, sub)}
    note("small corpora")
    small = []
    for n in (1, 10, 100, 1000, 10000):
        sub = lines[:n]
        dev_ms, host_ms = [], []
        for r in range(6):                          # interleaved, first round dropped
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            CS.corpus_statistics_device(tok, sub)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if n <= 1000:
                CS.corpus_statistics_host(tok.tokenize, sub)
            t2 = time.perf_counter()
            if r:
                dev_ms.append((t1 - t0) * 1e3)
                host_ms.append((t2 - t1) * 1e3)
        small.append({"lines": n, "device_path_ms": spread(dev_ms), "per_line_host_ms": spread(host_ms) if n <= 1000 else None})
    res["small_corpora"] = small
    new = res["corpus_statistics"]["wall_ms"]["median"]
    res["speedup_vs_tokenize_batch_then_host_loop"] = round(res["tokenize_batch_then_host_loop"]["scaled_to_all_lines_ms"] / new, 1)
    res["speedup_vs_per_line_tokenize"] = round(res["per_line_tokenize"]["scaled_to_all_lines_ms"] / new, 1)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
