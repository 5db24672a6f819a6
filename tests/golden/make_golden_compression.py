#!/usr/bin/env python
"""Generate tests/golden/g8_compression_{reference,lorentz}.{json,npz} by running the REFERENCE's
``tokenizer/compression_aware_tokenizer.py`` itself.

Like make_golden.py it runs only where the reference is present (it is imported, never copied) and applies
the same two sign patches:
  reference : the modules exactly as shipped (every distance is 0.0: every pair is a candidate)
  lorentz   : ``minkowski_dot`` negated and ``batch_distance`` invoked as ``orig(x, -y, c)``

Per mode and per table size (n = 150: the fp32-compare search branch, n = 60: the double-compare branch),
d = 8, over a corpus of 8 lines built from near-pair concatenations (two of them share their first 20
characters, one is a duplicate, one holds a non-BMP character and characters outside the vocabulary), runs
  s100     sample_size=100, 8 steps (log every 3)
  s5       sample_size=5, 8 steps (the remainder's 1 / (1 + d) scores matter)
  nocorpus no corpus sample: the plain nearest pair, 4 steps
  none     a threshold no pair passes: "No more merge candidates found after 0 steps"
and records for each: one direct _find_merge_candidates() (npz: i, j, -score) and the tokenize_cache after it, then the merge
sequence, the per-step (i, j, score), the log lines, the tokenize_cache after optimize_merges, and what save()
writes.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_compression.py [reference|lorentz|all]
"""
from __future__ import annotations

import json
import logging
import os
import random
import sys
import tempfile
import warnings

REF = "/root/reference"
if not os.path.isdir(REF):
    sys.exit("make_golden_compression.py: /root/reference is not present; golden vectors can only be regenerated "
             "in the build container.")

os.environ.setdefault("TQDM_DISABLE", "1")
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, REF)
warnings.filterwarnings("ignore")

import numpy as np  # noqa: E402
import torch  # noqa: E402

import embedding.lorentz_model as L  # noqa: E402  (reference)
import tokenizer.hyperbolic_merge as HM  # noqa: E402  (reference)
import tokenizer.compression_aware_tokenizer as CA  # noqa: E402  (reference)

from hyptokenizer_amd.synthetic import cjk_vocab, lorentz_table  # noqa: E402  (ours: inputs only)

_ORIG = {"minkowski_dot": L.minkowski_dot, "batch_distance": L.batch_distance}

D, THR, SEED, SCALE = 8, 0.1, 7, 0.05
SIZES = (150, 60)


def set_mode(mode: str) -> None:
    """Install / remove the two sign patches (make_golden.py set_mode)."""
    if mode == "reference":
        L.minkowski_dot = _ORIG["minkowski_dot"]
        bd = _ORIG["batch_distance"]
    elif mode == "lorentz":
        L.minkowski_dot = lambda a, b: -_ORIG["minkowski_dot"](a, b)
        bd = lambda x, y, c=1.0: _ORIG["batch_distance"](x, -y, c)  # noqa: E731
    else:
        raise ValueError(mode)
    L.batch_distance = bd
    HM.batch_distance = bd
    HM.batch_distance_compiled = bd


def seed_all(seed: int) -> None:
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)


def corpus_for(vocab, cands, seed=11, lines=6, chunks=12):
    """Lines in which the concatenations of near pairs occur, plus the cache-key edge cases: a line that shares
    its first 20 characters with line 0, a duplicate of line 2, non-BMP and out-of-vocabulary characters."""
    rs = np.random.RandomState(seed)
    n = len(vocab)
    top = sorted(cands, key=lambda c: c[2])[:40]
    out = []
    for _ in range(lines):
        parts = []
        for _ in range(chunks):
            if top and rs.rand() < 0.5:
                i, j, _d = top[int(rs.randint(0, len(top)))]
                parts.append(vocab[i] + vocab[j])
            else:
                parts.append(vocab[int(rs.randint(0, n))])
        out.append("".join(parts))
    out[3] = out[3][:7] + "\U0001F600x" + out[3][7:]
    out.append(out[0][:20] + "".join(reversed(out[1]))[:9])
    out.append(out[2])
    return out


class _Logs(logging.Handler):
    def __init__(self):
        super().__init__(logging.INFO)
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


def _mk(X, thr, corpus, **kw):
    n = X.shape[0]
    return CA.CompressionAwareTokenizer(vocab=cjk_vocab(n), embeddings=torch.nn.Parameter(X.clone()), corpus_sample=corpus,
                                        curvature=1.0, merge_threshold=thr, device=torch.device("cpu"),
                                        max_vocab_size=n + 24, use_approximate_search=False, **kw)


def run(X, thr, corpus, steps, log_every, **kw):
    tok = _mk(X, thr, corpus, **kw)
    rec = {}
    direct = tok._find_merge_candidates()
    direct = (np.array([c[0] for c in direct], np.int32), np.array([c[1] for c in direct], np.int32),
              np.array([c[2] for c in direct], np.float64))
    rec["cache_after_direct"] = dict(tok.tokenize_cache)
    picks = []
    orig_find = tok._find_merge_candidates

    def find():
        c = orig_find()
        if c:
            picks.append([int(c[0][0]), int(c[0][1]), -float(c[0][2])])
        return c

    tok._find_merge_candidates = find
    logger = logging.getLogger(CA.__name__)
    h = _Logs()
    logger.addHandler(h)
    logger.setLevel(logging.INFO)
    try:
        tok.optimize_merges(steps=steps, log_every=log_every)
    finally:
        logger.removeHandler(h)
    del tok._find_merge_candidates
    rec["picks"] = picks
    rec["logs"] = h.lines
    rec["merge_history"] = [list(m) for m in tok.merge_history]
    rec["cache_after_loop"] = dict(tok.tokenize_cache)
    rec["merge_threshold"] = tok.merge_threshold
    rows = tok.embeddings.data[X.shape[0]:tok.current_vocab_size].numpy().copy()
    with tempfile.TemporaryDirectory() as td:
        tok.save(td)
        rec["save_files"] = sorted(os.listdir(td))
        rec["save_json"] = {fn: json.load(open(os.path.join(td, fn), encoding="utf-8"))
                            for fn in rec["save_files"] if fn.endswith(".json")}
        emb = torch.load(os.path.join(td, "embeddings.pt"), weights_only=True)
        rec["save_embeddings_shape"] = list(emb.shape)
        try:
            CA.CompressionAwareTokenizer.load(td, device=torch.device("cpu"))
            rec["reference_load"] = "ok"
        except Exception as exc:         # see tests/test_compression_golden.py: the reference's load raises here
            rec["reference_load"] = f"raises {type(exc).__name__}"
    return rec, rows, direct


def g8(mode: str) -> None:
    out, meta = {}, {"d": D, "thr": THR, "seed": SEED, "scale": SCALE, "sizes": list(SIZES)}
    for n in SIZES:
        X = lorentz_table(n, D, seed=SEED, scale=SCALE)
        out[f"n{n}_X"] = X.numpy()
        probe = HM.HyperbolicTokenizer(vocab=cjk_vocab(n), embeddings=torch.nn.Parameter(X.clone()), curvature=1.0,
                                       merge_threshold=THR, device=torch.device("cpu"), max_vocab_size=n + 24,
                                       use_approximate_search=False)
        corpus = corpus_for(cjk_vocab(n), probe._find_merge_candidates())
        meta[f"n{n}_corpus"] = corpus
        runs = {
            "s100": (THR, corpus, 8, 3, {}),
            "s5": (THR, corpus, 8, 2, {"sample_size": 5}),
            "nocorpus": (THR, None, 4, 1, {}),
            "none": (0.0 if mode == "reference" else 1e-9, corpus, 3, 1, {}),
        }
        for name, (thr, corp, steps, log_every, kw) in runs.items():
            seed_all(42)
            rec, rows, direct = run(X, thr, corp, steps, log_every, **kw)
            rec.update({"thr": thr, "steps": steps, "log_every": log_every, "kwargs": kw, "corpus": corp is not None})
            meta[f"n{n}_{name}"] = rec
            out[f"n{n}_{name}_rows"] = rows
            for fld, arr in zip(("i", "j", "negscore"), direct):
                out[f"n{n}_{name}_direct_{fld}"] = arr
            print(f"[{mode}] n={n} {name}: {len(rec['merge_history'])} merges, {len(direct[0])} candidates", flush=True)
        if mode == "lorentz":
            # the compression term must change the merge sequence: a class that ignores it cannot pass
            seed_all(42)
            plain = HM.HyperbolicTokenizer(vocab=cjk_vocab(n), embeddings=torch.nn.Parameter(X.clone()), curvature=1.0,
                                           merge_threshold=THR, device=torch.device("cpu"), max_vocab_size=n + 24,
                                           use_approximate_search=False)
            plain.optimize_merges(steps=8, log_every=10 ** 9)
            plain_hist = [list(m) for m in plain.merge_history]
            meta[f"n{n}_plain_merge_history"] = plain_hist
            assert plain_hist != meta[f"n{n}_s100"]["merge_history"], "compression term left the merges unchanged"
    np.savez_compressed(os.path.join(HERE, f"g8_compression_{mode}.npz"), **out)
    with open(os.path.join(HERE, f"g8_compression_{mode}.json"), "w", encoding="utf-8") as f:
        json.dump(meta, f, indent=1, ensure_ascii=False)


def main() -> None:
    which = sys.argv[1] if len(sys.argv) > 1 else "all"
    for mode in (("reference", "lorentz") if which == "all" else (which,)):
        set_mode(mode)
        g8(mode)
    set_mode("reference")


if __name__ == "__main__":
    main()
