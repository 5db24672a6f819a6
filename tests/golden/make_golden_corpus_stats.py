#!/usr/bin/env python
"""Generate tests/golden/g15_corpus_stats.json by running the REFERENCE's own corpus evaluation.

Runs only in the build container: it imports the reference's modules from /root/reference (never copied, never shipped)
and records, per case, the rules, the lines, the reference's ``tokenize`` of every line and the dictionaries its three
functions return (scripts/compare_tokenizers.py: benchmark_hyperbolic_tokenizer, evaluate_linguistic_quality,
evaluate_compression_efficiency, the last two with is_hyperbolic=True).

``scripts.compare_tokenizers`` does not import as shipped; two shims are applied IN MEMORY, nothing is written:
  * ``seaborn`` (not installed; used only by the plots) is replaced by an empty module object;
  * ``embedding.lorentz_model`` gets ``poincare_to_lorentz`` / ``lorentz_to_poincare`` from ``embedding.poincare_ball``,
    the two names tokenizer/enhanced_fast_hyperbolic_merge.py imports from the wrong module (as make_golden.py
    does); neither is called here.

Cases:
  wikitext  the rules of g6_tokenize_lorentz.json (trained by the reference's CLI function, plus multi-level hand-made
            rules) on 200 non-empty lines of the reference's data/processed/wikitext103/test.txt, truncated;
  handmade  the same rules plus left-to-right chains for every alternative of the suffix pattern and a few others, on
            hand-made lines: empty, one character, punctuation only, digits and '_', non-ASCII letters, characters outside
            the vocabulary, a bare suffix as a whole token, every suffix class at a token's end, a prefix as a whole token,
            a text with a trailing newline.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_corpus_stats.py
"""
from __future__ import annotations

import json
import os
import sys
import types
import warnings

REF = "/root/reference"
if not os.path.isdir(REF):
    sys.exit("make_golden_corpus_stats.py: /root/reference is not present; golden vectors can only be regenerated "
             "in the build container.")

os.environ.setdefault("TQDM_DISABLE", "1")
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, REF)
warnings.filterwarnings("ignore")

import torch  # noqa: E402

import embedding.lorentz_model as L  # noqa: E402  (reference)
import embedding.poincare_ball as P  # noqa: E402  (reference)

# shim 1: the plots' only dependency that is missing here
sys.modules.setdefault("seaborn", types.ModuleType("seaborn"))
# shim 2: SURVEY F8
L.poincare_to_lorentz = P.poincare_to_lorentz
L.lorentz_to_poincare = P.lorentz_to_poincare

import scripts.compare_tokenizers as CT  # noqa: E402  (reference)
import tokenizer.hyperbolic_merge as HM  # noqa: E402  (reference)
import tokenizer.fast_hyperbolic_merge as FM  # noqa: E402  (reference)

from hyptokenizer_amd.synthetic import lorentz_table  # noqa: E402  (ours: inputs only)

import logging  # noqa: E402

logging.disable(logging.CRITICAL)

SUFFIXES = ["ion", "tion", "ation", "ment", "ance", "ence", "ly", "ish", "less", "ful", "ness", "ing", "ed", "er", "est",
            "pre", "un", "re", "de", "dis"]
TIMING_KEYS = ("avg_tokenization_time", "tokens_per_second")


def chain(word):
    """left-to-right rules that build ``word`` from its characters"""
    return [(word[:k], word[k], word[:k + 1]) for k in range(1, len(word))]


def make_tokenizer(cls, vocab, merges):
    vocab = list(vocab)
    for (_a, _b, ab) in merges:
        if ab not in vocab:
            vocab.append(ab)
    X = lorentz_table(len(vocab), 5, seed=1, scale=0.05)
    tok = cls(vocab=list(vocab), embeddings=torch.nn.Parameter(X), device=torch.device("cpu"),
              max_vocab_size=len(vocab) + 8, use_approximate_search=False)
    tok.merge_history = [tuple(m) for m in merges]
    return tok


def record(name, vocab, merges, lines):
    tok = make_tokenizer(HM.HyperbolicTokenizer, vocab, merges)
    tokens = [tok.tokenize(t) for t in lines]
    bench = CT.benchmark_hyperbolic_tokenizer(tok, lines, num_runs=3)
    bench1 = CT.benchmark_hyperbolic_tokenizer(tok, lines, num_runs=1)
    ling = CT.evaluate_linguistic_quality(tok, lines, is_hyperbolic=True)
    comp = CT.evaluate_compression_efficiency(tok, lines, is_hyperbolic=True)
    fast = make_tokenizer(FM.FastHyperbolicTokenizer, vocab, merges)
    fast_type = CT.benchmark_hyperbolic_tokenizer(fast, lines[:3], num_runs=1)["tokenizer_type"]
    return {"name": name, "vocab": list(tok.vocab), "merges": [list(m) for m in merges], "lines": lines, "tokens": tokens,
            "benchmark": bench, "benchmark_one_run": bench1, "linguistic": ling, "compression": comp,
            "timing_keys": list(TIMING_KEYS), "fast_tokenizer_type": fast_type}


def main():
    with open(os.path.join(HERE, "g6_tokenize_lorentz.json"), encoding="utf-8") as f:
        g6 = json.load(f)
    vocab, merges = g6["vocab"], [tuple(m) for m in g6["merges"]]

    wiki = []
    with open(os.path.join(REF, "data/processed/wikitext103/test.txt"), encoding="utf-8") as f:
        for line in f:
            line = line.strip()
            if line:
                wiki.append(line[:96])
            if len(wiki) == 200:
                break
    cases = [record("wikitext", vocab, merges, wiki)]

    extra = []
    for w in SUFFIXES + ["café", "ed\n", "a_1"]:
        for r in chain(w):
            if r not in extra and r not in merges:
                extra.append(r)
    extra += [("x", s, "x" + s) for s in SUFFIXES]        # a longer token that ends in the suffix
    hand = ["", "a", "Q", "?", ".,;:!? ...", "2024_01_02 __init__ 007", "naïve café 中文 über straße Δx",
            "QWZ☃\U0001F600X", "ed", "Q ed Q", "un", "re Q un", "the thing"]
    hand += [f"Q{s}Q" for s in SUFFIXES] + [f"{s}" for s in SUFFIXES] + [f"X{s} {s}X" for s in SUFFIXES] + [f"Qx{s}Q x{s}" for s in SUFFIXES]
    hand += ["walked\n", "Qed\n", "\n", "a_1 a_1a_1", "", "nation station fulness dislessly unprereded", "  ", "\t x"]
    cases.append(record("handmade", vocab, merges + extra, hand))

    # what the fixture promises (checked here, so that a change of the rules cannot silently lose a case)
    flat = [t for toks in cases[1]["tokens"] for t in toks]
    for s in SUFFIXES:
        assert any(t.endswith(s) for t in flat), s
        assert s in flat and "x" + s in flat, s
    assert "ed\n" in flat and "café" in flat and any(len(t) == 1 and ord(t) > 0xFFFF for t in flat)
    assert {"the", "ing", "tion", " the"} <= {t for toks in cases[0]["tokens"] for t in toks}     # multi-level rules fire
    assert all(c["fast_tokenizer_type"] == "standard" and c["benchmark"]["tokenizer_type"] == "standard" for c in cases)

    # a corpus without tokens: the reference divides by zero in all three functions
    tok = make_tokenizer(HM.HyperbolicTokenizer, vocab, merges)
    zero = {}
    for fn_name, call in (("benchmark", lambda: CT.benchmark_hyperbolic_tokenizer(tok, ["", ""], 3)),
                          ("linguistic", lambda: CT.evaluate_linguistic_quality(tok, ["", ""], True)),
                          ("compression", lambda: CT.evaluate_compression_efficiency(tok, ["", ""], True))):
        try:
            call()
            zero[fn_name] = None
        except Exception as exc:        # noqa: BLE001
            zero[fn_name] = type(exc).__name__
    out = {"cases": cases, "zero_token_corpus": {"lines": ["", ""], "raises": zero}}
    path = os.path.join(HERE, "g15_corpus_stats.json")
    with open(path, "w", encoding="utf-8") as f:
        json.dump(out, f, ensure_ascii=False)
    print(path, os.path.getsize(path), "bytes;", [(c["name"], len(c["lines"]), sum(map(len, c["tokens"]))) for c in cases], zero)


if __name__ == "__main__":
    main()
