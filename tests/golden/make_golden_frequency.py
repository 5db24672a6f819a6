#!/usr/bin/env python
"""Generate tests/golden/g9_frequency_{reference,lorentz}.{json,npz} by running the REFERENCE's
``tokenizer/frequency_aware_hyperbolic_merge.py`` itself.

Like make_golden_compression.py it runs only where the reference is present (it is imported, never copied) and
applies the same two sign patches:
  reference : the modules exactly as shipped (every distance is 0.0: every pair is a candidate)
  lorentz   : ``minkowski_dot`` negated and ``batch_distance`` invoked as ``orig(x, -y, c)``

Per mode and per table size (n = 150: the fp32-compare search branch, n = 60: the double-compare branch), d = 8, one
vocabulary entry replaced by "|" (a key of frequencies.json with more than one "|"), over a corpus of about 12 lines
written with "\\r\\n" and "\\r" line ends, "\\x0c" / "\\u2028" / "\\x85" inside lines, leading and trailing whitespace, a
non-BMP character, characters outside the vocabulary and empty lines, runs
  corpus      built with corpus_path, 6 steps (log every 3)
  merged      3 unscored steps without a corpus, then optimize_merges(corpus_path=...): the counts see merged tokens
  accumulate  built with corpus_path, 2 steps, then optimize_merges(corpus_path=...) again: the counts add up
  unscored    beta > 0 and no corpus: the first row-major candidate, 4 steps
  gamma0      gamma = 0 (the coherence still draws its permutations), 4 steps
  none        a threshold no pair passes, 14 steps: the x1.5 growth twice
and records for each: the per-step picks (``_find_merge_candidates()[0]``: (i, j, -score) or unscored (i, j, d)), the
log lines, the merges, the new rows, hashes of the torch and Python RNG states, SHA-256 digests of pair_frequencies (as
an ordered JSON list) after construction and at the end, and of the bytes of every json file save() writes
(config.json also parsed).  Two ordered lists are kept in full per size: the counts of the plain corpus and those of
the "merged" run.  The json file holds one line per key, so that it stays small enough to read.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_frequency.py [reference|lorentz|all]
"""
from __future__ import annotations

import hashlib
import json
import logging
import os
import random
import sys
import tempfile
import warnings

REF = "/root/reference"
if not os.path.isdir(REF):
    sys.exit("make_golden_frequency.py: /root/reference is not present; golden vectors can only be regenerated "
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
import tokenizer.frequency_aware_hyperbolic_merge as FA  # noqa: E402  (reference)

from hyptokenizer_amd.synthetic import cjk_vocab, lorentz_table  # noqa: E402  (ours: inputs only)

_ORIG = {"minkowski_dot": L.minkowski_dot, "batch_distance": L.batch_distance}

D, THR, SEED, SCALE = 8, 0.1, 7, 0.05
SIZES = (150, 60)
PIPE = 5                                   # vocab[PIPE] = "|"


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


def vocab_for(n):
    v = cjk_vocab(n)
    v[PIPE] = "|"
    return v


def corpus_text(vocab, cands, seed=11):
    """About 12 lines of text, as bytes-exact str (newlines included): near pairs, the first row-major candidates'
    concatenations (merged by the unscored steps), "|", and the line-reading edge cases."""
    rs = np.random.RandomState(seed)
    n = len(vocab)
    near = sorted(cands, key=lambda c: c[2])[:30]
    first = cands[:3]

    def chunk(k):
        parts = []
        for _ in range(k):
            r = rs.rand()
            if near and r < 0.45:
                i, j, _d = near[int(rs.randint(0, len(near)))]
                parts.append(vocab[i] + vocab[j])
            elif first and r < 0.65:
                i, j, _d = first[int(rs.randint(0, len(first)))]
                parts.append(vocab[i] + vocab[j])
            else:
                parts.append(vocab[int(rs.randint(0, n))])
        return "".join(parts)

    lines = [
        chunk(10) + "\r\n",
        "  " + chunk(6) + "\t \n",
        chunk(5) + "\x0c" + chunk(5) + "\n",
        "\n",
        chunk(4) + " " + chunk(4) + "\r\n",
        chunk(3) + "|" + vocab[0] + "|" + chunk(3) + "\n",
        "\U0001F600" + chunk(4) + "xyz" + chunk(2) + "\r",
        "   \n",
        chunk(6) + "\x85" + chunk(2) + "\x0b" + chunk(2) + "\n",
        vocab[1] + "\n",
        chunk(8) + "　\n",
        chunk(7) + " " + chunk(7),                      # no final newline
    ]
    return "".join(lines)


class _Logs(logging.Handler):
    def __init__(self):
        super().__init__(logging.INFO)
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


def _hash_state():
    return {"torch": hashlib.sha256(torch.get_rng_state().numpy().tobytes()).hexdigest(),
            "python": hashlib.sha256(repr(random.getstate()).encode()).hexdigest()}


def _freqs(tok):
    return [[list(k), v] for k, v in tok.pair_frequencies.items()]


def _digest(obj) -> str:
    """SHA-256 of ``obj`` as JSON text (a str is taken as the text itself)."""
    text = obj if isinstance(obj, str) else json.dumps(obj, ensure_ascii=False)
    return hashlib.sha256(text.encode("utf-8")).hexdigest()


def compact_record(rec: dict) -> dict:
    """The run record as committed: digests instead of the pair lists and of save()'s json files."""
    out = {k: v for k, v in rec.items() if k not in ("freq_after_init", "freq_final", "save_text")}
    out["freq_after_init_sha256"] = _digest(rec["freq_after_init"])
    out["freq_final_sha256"] = _digest(rec["freq_final"])
    out["freq_final_len"] = len(rec["freq_final"])
    out["save_sha256"] = {fn: _digest(text) for fn, text in rec["save_text"].items()}
    out["save_config"] = json.loads(rec["save_text"]["config.json"])
    return out


def write_meta(meta: dict, path: str) -> None:
    """One line per top-level key."""
    body = ",\n".join(f"{json.dumps(k)}: {json.dumps(v, ensure_ascii=False)}" for k, v in meta.items())
    with open(path, "w", encoding="utf-8") as f:
        f.write("{\n" + body + "\n}\n")


def run(X, vocab, thr, corpus_path, plan, **kw):
    """plan: list of (steps, log_every, corpus_path or None) optimize_merges calls; corpus_path: the constructor's."""
    rec = {}
    logger = logging.getLogger(FA.__name__)
    h = _Logs()
    logger.addHandler(h)
    logger.setLevel(logging.INFO)
    try:
        tok = FA.FrequencyAwareHyperbolicTokenizer(vocab=list(vocab), embeddings=torch.nn.Parameter(X.clone()),
                                                   corpus_path=corpus_path, curvature=1.0, merge_threshold=thr,
                                                   device=torch.device("cpu"), max_vocab_size=X.shape[0] + 24,
                                                   use_approximate_search=False, **kw)
        rec["freq_after_init"] = _freqs(tok)
        picks = []
        orig_find = tok._find_merge_candidates

        def find():
            c = orig_find()
            picks.append(None if not c else [int(c[0][0]), int(c[0][1]), float(c[0][2]), len(c)])
            return c

        tok._find_merge_candidates = find
        for steps, log_every, cp in plan:
            tok.optimize_merges(steps=steps, log_every=log_every, corpus_path=cp)
        del tok._find_merge_candidates
    finally:
        logger.removeHandler(h)
    rec["picks"] = picks
    rec["logs"] = h.lines
    rec["freq_final"] = _freqs(tok)
    rec["merge_history"] = [list(m) for m in tok.merge_history]
    rec["merge_threshold"] = tok.merge_threshold
    rec["rng"] = _hash_state()
    rows = tok.embeddings.data[X.shape[0]:tok.current_vocab_size].numpy().copy()
    with tempfile.TemporaryDirectory() as td:
        tok.save(td)
        rec["save_files"] = sorted(os.listdir(td))
        rec["save_text"] = {fn: open(os.path.join(td, fn), encoding="utf-8").read()
                            for fn in rec["save_files"] if fn.endswith(".json")}
        emb = torch.load(os.path.join(td, "embeddings.pt"), weights_only=True)
        rec["save_embeddings_shape"] = list(emb.shape)
        try:
            FA.FrequencyAwareHyperbolicTokenizer.load(td, device=torch.device("cpu"))
            rec["reference_load"] = "ok"
        except Exception as exc:         # the reference's load raises on its own files (module docstring of ours)
            rec["reference_load"] = f"raises {type(exc).__name__}"
    return rec, rows


def g9(mode: str) -> None:
    out, meta = {}, {"d": D, "thr": THR, "seed": SEED, "scale": SCALE, "sizes": list(SIZES), "pipe": PIPE}
    ref_mode = mode == "reference"
    for n in SIZES:
        X = lorentz_table(n, D, seed=SEED, scale=SCALE)
        vocab = vocab_for(n)
        out[f"n{n}_X"] = X.numpy()
        probe = HM.HyperbolicTokenizer(vocab=list(vocab), embeddings=torch.nn.Parameter(X.clone()), curvature=1.0,
                                       merge_threshold=THR, device=torch.device("cpu"), max_vocab_size=n + 24,
                                       use_approximate_search=False)
        text = corpus_text(vocab, probe._find_merge_candidates())
        meta[f"n{n}_corpus_text"] = text
        with tempfile.TemporaryDirectory() as td:
            cp = os.path.join(td, "corpus.txt")
            with open(cp, "w", encoding="utf-8", newline="") as f:
                f.write(text)
            s = 3 if ref_mode else 6              # the reference scores every pair in its own sign mode: keep it short
            runs = {
                "corpus": (THR, True, [(s, 3, None)], {}),
                "merged": (THR, False, [(3, 1, None), (3, 3, cp)], {}),
                "accumulate": (THR, True, [(2, 3, None), (2, 3, cp)], {}),
                "unscored": (THR, False, [(4, 1, None)], {}),
                "gamma0": (THR, True, [(3, 1, None)], {"gamma": 0.0}),
                "none": (0.0 if ref_mode else 1e-9, True, [(14, 1, None)], {}),
            }
            for name, (thr, with_corpus, plan, kw) in runs.items():
                seed_all(42)
                rec, rows = run(X, vocab, thr, cp if with_corpus else None,
                                [(st, le, (cp if c else None)) for st, le, c in plan], **kw)
                rec.update({"thr": thr, "corpus": with_corpus, "plan": [[st, le, bool(c)] for st, le, c in plan],
                            "kwargs": kw})
                if name == "corpus":
                    meta[f"n{n}_freq_corpus"] = rec["freq_after_init"]
                elif name == "merged":
                    meta[f"n{n}_freq_merged"] = rec["freq_final"]
                meta[f"n{n}_{name}"] = compact_record(rec)
                out[f"n{n}_{name}_rows"] = rows
                print(f"[{mode}] n={n} {name}: {len(rec['merge_history'])} merges, "
                      f"{len(rec['freq_final'])} pairs", flush=True)
    np.savez_compressed(os.path.join(HERE, f"g9_frequency_{mode}.npz"), **out)
    write_meta(meta, os.path.join(HERE, f"g9_frequency_{mode}.json"))


def main() -> None:
    which = sys.argv[1] if len(sys.argv) > 1 else "all"
    for mode in (("reference", "lorentz") if which == "all" else (which,)):
        set_mode(mode)
        g9(mode)
    set_mode("reference")


if __name__ == "__main__":
    main()
