#!/usr/bin/env python
"""Generate tests/golden/g10_hierarchical_{reference,lorentz}.{json,npz} by running the REFERENCE's
``tokenizer/hierarchical_hyperbolic_merge.py`` itself (its branch without nltk, which is not installed).

Like make_golden_frequency.py it runs only where the reference is present (it is imported, never copied) and applies the
same two sign patches (reference: as shipped, every distance 0.0 and merged rows NaN; lorentz: sign-corrected).

Phase lengths.  The reference's phases run 2000 / 5000 / 10000 iterations, each building the O(N^2) candidate list in
Python.  The goldens shorten them the same way in both codes: here ``tqdm.tqdm`` is replaced while the reference runs by a
wrapper that cuts the phase's ``range`` to PHASE_STEPS (the reference imports tqdm inside the method, so the wrapper is what
it gets); the tests set ``HierarchicalHyperbolicTokenizer.PHASE_STEPS`` to the same numbers.  Nothing else changes: the
thresholds, the floors (500 / 2000 / 5000) and the relaxation rule are the reference's own.

Per mode and per table size (n = 150: fp32-compare search branch; n = 60: double-compare branch), d = 8, a vocabulary of
ASCII letters, digrams, trigrams, 4-grams, a non-BMP character and accented letters, and a generated corpus of about 40
lines (non-ASCII and non-BMP words, mixed case), the corpus runs are
  phases    with the corpus, all three phases (PHASE_STEPS = (40, 40, 40))
  target    with the corpus, target_vocab_size = n + 12 (returns inside phase 1)
These merge one cluster of near rows (rows are never removed, so a pair that is nearest stays near).  Inside such a
cluster the midpoints make many pairs equidistant up to rounding, where the canonical fp32 distances and the reference's
torch ones may order a near-tie differently; the scenarios below therefore stop three merges after their decisive step.  The SCENARIOS
drive one phase at a time (the other ranges cut to 0, so a phase starts on a table built for it): a table of far-apart
rows (every distance above 1.2) with planted near pairs of chosen distance and chosen token strings, and string sets set
directly on the object in both codes:
  p1        phase 1: the <= 2 filter decides against two nearer pairs (lengths 2 + 3, and 4 + 5)
  p1break   phase 1: candidates, but none of length <= 3 after the relaxation: break; then 3 steps of phase 2
  p2        phase 2: no candidate at 0.1 -> x1.2 -> continue twice, then the 0.8 boost of a common morpheme wins
  p2df      phase 2: the same with a string in >= 5 common words (the substring rule) instead
  p3        phase 3: x1.2 four times, then a common word (S3, outside the boosted classes) wins over a heuristic-boosted
            pair and a nearer unboosted pair
  p3cap     phase 3: no pair below 1.0: x1.2 until the threshold passes 1.0, then break
and records for each: the log lines, the merge history, the final threshold, the new rows; and per size: the statistics
(token_frequencies as an ordered list, the two sets sorted), both predicates on probe strings, the parsed
hierarchical_data.json of a saved directory (lists compared as sets: the reference writes set order), and the exception
an empty corpus raises.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_hierarchical.py [reference|lorentz|all]
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
    sys.exit("make_golden_hierarchical.py: /root/reference is not present; golden vectors can only be regenerated "
             "in the build container.")

os.environ.setdefault("TQDM_DISABLE", "1")
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, REF)
warnings.filterwarnings("ignore")
logging.getLogger().setLevel(logging.ERROR)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import tqdm as _tqdm_mod  # noqa: E402

import embedding.lorentz_model as L  # noqa: E402  (reference)
import tokenizer.hyperbolic_merge as HM  # noqa: E402  (reference)
import tokenizer.hierarchical_hyperbolic_merge as HH  # noqa: E402  (reference)

from hyptokenizer_amd.synthetic import lorentz_table  # noqa: E402  (ours: inputs only)

_ORIG = {"minkowski_dot": L.minkowski_dot, "batch_distance": L.batch_distance}
_TQDM = _tqdm_mod.tqdm

D, SEED, SCALE = 8, 7, 0.05
SIZES = (150, 60)
RUNS = {
    "phases": dict(corpus=True, steps=(40, 40, 40), target=None),
    "target": dict(corpus=True, steps=(40, 40, 40), target=12),
}
# planted pairs: (left token, right token, distance); sets: common_morphemes, common_words
SCENARIOS = {
    "p1": dict(steps=(8, 0, 0), pairs=[("x", "z", 0.03), ("pq", "rst", 0.02), ("klmn", "vwxyz", 0.01)],
               morphemes=[], words=[]),
    "p1break": dict(steps=(8, 3, 0), pairs=[("klmn", "vwxyz", 0.01), ("bcdf", "g", 0.02)], morphemes=[], words=[]),
    "p2": dict(steps=(0, 6, 0), pairs=[("k", "v", 0.15), ("m", "nt", 0.17)], morphemes=["mnt", "zz"], words=[]),
    "p2df": dict(steps=(0, 6, 0), pairs=[("k", "v", 0.15), ("gh", "t", 0.165)], morphemes=["zz"],
                 words=["light", "night", "fight", "sight", "might", "tight"]),
    "p3": dict(steps=(0, 0, 7), pairs=[("x", "z", 0.38), ("b", "ca", 0.40), ("q", "rs", 0.39)], morphemes=[],
               words=["qrs", "hello"]),
    "p3cap": dict(steps=(0, 0, 15), pairs=[], morphemes=[], words=["qrs"]),
}
BASE_SCALE = 2.0
PROBES = ["", "a", "th", "the", "he", "ing", "xyz", "qq", "thing", "thingsx", "é", "éa", "\U0001D518a", "zzzz", "bcd",
          "ou", "ea", "in", "an", "ant", "tha", "hea", "ring", "str", "bb", "aa"]


def set_mode(mode: str) -> None:
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


class _ShortBar:
    def __init__(self, it):
        self._it = it

    def __iter__(self):
        return iter(self._it)

    def set_postfix(self, *a, **k):
        pass


def shorten(steps):
    caps = {"Phase 1: Character merges": steps[0], "Phase 2: Subword merges": steps[1], "Phase 3: Word merges": steps[2]}

    def fake(it, desc=None, **kw):
        if desc in caps:
            return _ShortBar(range(min(len(it), caps[desc])))
        return _ShortBar(it)
    return fake


def vocab_for(n):
    letters = [chr(ord("a") + k) for k in range(26)]
    extra = ["th", "he", "in", "er", "an", "re", "on", "ou", "é", "ñ", "\U0001D518", "中", "ing", "the", "and", "ion",
             "tion", "ment", "st", "nd", "ea", "ch", "sh", "qu", "ss", "ll", "x1", "zz", "ab", "ly"]
    v = letters + extra
    rs = np.random.RandomState(3)
    pool = letters + ["é", "ñ"]
    while len(v) < n:
        k = int(rs.randint(1, 5))
        v.append("".join(pool[int(rs.randint(0, len(pool)))] for _ in range(k)))
    return v[:n]


def corpus_text(seed=11):
    rs = np.random.RandomState(seed)
    stems = ["the", "then", "there", "thing", "ring", "sing", "string", "and", "hand", "stand", "ion", "nation", "station",
             "mention", "ment", "moment", "ly", "only", "early", "chess", "shell", "quest", "ab", "abc", "éclair", "niño",
             "中文", "\U0001D518nit", "x1y", "zz"]
    lines = []
    for k in range(40):
        words = [stems[int(rs.randint(0, len(stems)))] for _ in range(int(rs.randint(3, 9)))]
        if k % 7 == 0:
            words = [w.upper() for w in words]
        lines.append(" ".join(words) + (", ok.\n" if k % 3 else "\r\n"))
    lines.append("Σίσυφος ΣΊΣΥΦΟΣ straße İstanbul\n")
    return "".join(lines)


class _Logs(logging.Handler):
    def __init__(self):
        super().__init__(logging.INFO)
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


def plant(S, a, b, target):
    """Row b := row a moved orthogonally to its spatial vector by the step whose hyperbolic distance is `target`."""
    rs = np.random.RandomState(a * 7919 + b)
    sa = S[a].astype(np.float64)
    u = rs.randn(len(sa))
    u -= sa * (u @ sa) / (sa @ sa)
    u /= np.linalg.norm(u)
    r2 = sa @ sa
    lo, hi = 0.0, 10.0
    for _ in range(200):
        mid = (lo + hi) / 2
        if np.arccosh(np.sqrt(1 + r2) * np.sqrt(1 + r2 + mid * mid) - r2) < target:
            lo = mid
        else:
            hi = mid
    S[b] = (sa + lo * u).astype(np.float32)


def scenario(n, spec):
    """(table [n, D + 1] fp32, vocab) of a scenario: far-apart rows, planted pairs on rows (2k, 2k + 1) from row 10 on."""
    g = torch.Generator().manual_seed(1000 + n)
    S = (torch.randn(n, D, generator=g) * BASE_SCALE).numpy()
    rs = np.random.RandomState(n)
    cons = "bcdfghjklmnpqrstvwxz"
    vocab = ["".join(cons[k] for k in rs.randint(0, len(cons), 4)) for _ in range(n)]
    for k, (left, right, dist) in enumerate(spec["pairs"]):
        a, b = 10 + 2 * k, 11 + 2 * k
        plant(S, a, b, dist)
        vocab[a], vocab[b] = left, right
    x0 = np.sqrt(1.0 + (S.astype(np.float64) ** 2).sum(-1)).astype(np.float32)
    X = np.concatenate([x0[:, None], S], axis=1).astype(np.float32)
    X64 = X.astype(np.float64)
    G = X64[:, :1] @ X64[:, :1].T - X64[:, 1:] @ X64[:, 1:].T
    dist = np.arccosh(np.maximum(G, 1.0))
    planted = {(10 + 2 * k, 11 + 2 * k) for k in range(len(spec["pairs"]))}
    for i in range(n):
        for j in range(i + 1, n):
            if (i, j) not in planted:
                assert dist[i, j] > 1.2, (i, j, dist[i, j])
    return X, vocab


def make(n, mode, corpus_path, kwargs):
    X = lorentz_table(n, D, seed=SEED, scale=SCALE)
    return HH.HierarchicalHyperbolicTokenizer(vocab_for(n), torch.nn.Parameter(X.clone()),
                                              corpus_path=corpus_path, device=torch.device("cpu"),
                                              max_vocab_size=n + 200, use_approximate_search=False, **kwargs)


def run_mode(mode):
    set_mode(mode)
    meta = {"mode": mode, "D": D, "SEED": SEED, "SCALE": SCALE, "sizes": list(SIZES), "runs": RUNS, "probes": PROBES,
            "scenarios": SCENARIOS}
    arrays = {}
    tmp = tempfile.mkdtemp()
    corpus = os.path.join(tmp, "corpus.txt")
    text = corpus_text()
    with open(corpus, "w", encoding="utf-8", newline="") as f:
        f.write(text)
    meta["corpus_text"] = text
    empty = os.path.join(tmp, "empty.txt")
    open(empty, "w").close()
    try:
        make(SIZES[1], mode, empty, {})
        meta["empty_corpus_error"] = None
    except Exception as exc:  # noqa: BLE001
        meta["empty_corpus_error"] = [type(exc).__name__, str(exc)]
    for n in SIZES:
        arrays[f"n{n}_X"] = lorentz_table(n, D, seed=SEED, scale=SCALE).numpy()
        tok = make(n, mode, corpus, {})
        meta[f"n{n}_stats"] = {
            "token_frequencies": [[k, v] for k, v in tok.token_frequencies.items()],
            "common_morphemes": sorted(tok.common_morphemes),
            "common_words": sorted(tok.common_words),
            "is_potential_morpheme": [bool(tok._is_potential_morpheme(p)) for p in PROBES],
            "is_valid_word": [bool(tok._is_valid_word(p)) for p in PROBES],
        }
        for run, spec in RUNS.items():
            random.seed(42)
            np.random.seed(42)
            torch.manual_seed(42)
            tok = make(n, mode, corpus if spec["corpus"] else None, {})
            h = _Logs()
            lg = logging.getLogger(HH.__name__)
            lg.addHandler(h)
            lg.setLevel(logging.INFO)
            _tqdm_mod.tqdm = shorten(spec["steps"])
            try:
                tok.optimize_merges(target_vocab_size=(n + spec["target"]) if spec["target"] else None)
            finally:
                _tqdm_mod.tqdm = _TQDM
                lg.removeHandler(h)
            rows = tok.embeddings.data[n:tok.current_vocab_size].detach().cpu().numpy()
            arrays[f"n{n}_{run}_rows"] = rows
            rec = {"logs": h.lines, "merge_history": [list(m) for m in tok.merge_history],
                   "merge_threshold": tok.merge_threshold, "vocab_size": tok.current_vocab_size}
            if run == "phases":
                out = os.path.join(tmp, f"saved_{n}")
                tok.save(out)
                with open(os.path.join(out, "hierarchical_data.json")) as f:
                    rec["hierarchical_data"] = json.load(f)
                rec["hierarchical_data"]["common_morphemes"].sort()
                rec["hierarchical_data"]["common_words"].sort()
            meta[f"n{n}_{run}"] = rec
            print(mode, n, run, "merges", len(tok.merge_history), "thr", tok.merge_threshold, "phases",
                  [ln for ln in h.lines if ln.startswith("Completed")])
        for name, spec in SCENARIOS.items():
            X, vocab = scenario(n, spec)
            arrays[f"n{n}_{name}_X"] = X
            random.seed(42)
            np.random.seed(42)
            torch.manual_seed(42)
            tok = HH.HierarchicalHyperbolicTokenizer(list(vocab), torch.nn.Parameter(torch.from_numpy(X.copy())),
                                                     device=torch.device("cpu"), max_vocab_size=n + 200,
                                                     use_approximate_search=False)
            tok.common_morphemes = set(spec["morphemes"])
            tok.common_words = set(spec["words"])
            h = _Logs()
            lg = logging.getLogger(HH.__name__)
            lg.addHandler(h)
            lg.setLevel(logging.INFO)
            _tqdm_mod.tqdm = shorten(spec["steps"])
            try:
                tok.optimize_merges()
            finally:
                _tqdm_mod.tqdm = _TQDM
                lg.removeHandler(h)
            arrays[f"n{n}_{name}_rows"] = tok.embeddings.data[n:tok.current_vocab_size].detach().cpu().numpy()
            meta[f"n{n}_{name}"] = {"logs": h.lines, "merge_history": [list(m) for m in tok.merge_history],
                                    "merge_threshold": tok.merge_threshold, "vocab_size": tok.current_vocab_size,
                                    "vocab": vocab}
            print(mode, n, name, "merges", tok.merge_history[:4], "thr", tok.merge_threshold,
                  [ln for ln in h.lines if ln.startswith(("Completed", "Increasing"))])
    np.savez_compressed(os.path.join(HERE, f"g10_hierarchical_{mode}.npz"), **arrays)
    with open(os.path.join(HERE, f"g10_hierarchical_{mode}.json"), "w", encoding="utf-8") as f:
        json.dump(meta, f, ensure_ascii=False, indent=0)


if __name__ == "__main__":
    which = sys.argv[1] if len(sys.argv) > 1 else "all"
    for m in (("reference", "lorentz") if which == "all" else (which,)):
        run_mode(m)
