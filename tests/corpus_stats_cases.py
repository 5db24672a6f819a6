"""Shared by the corpus-statistics tests: a plain-Python truth and a seeded generator of small cases.

``truth`` restates what scripts/compare_tokenizers.py of the reference counts (:177-185, :254-278, :311-320) from token
lists, one character test at a time -- no compiled pattern is shared with the code under test.  The golden test checks it
against the reference's own dictionaries."""
import json
import os
import re

import numpy as np

SUFFIXES = ("ion", "tion", "ation", "ment", "ance", "ence", "ly", "ish", "less", "ful", "ness", "ing", "ed", "er", "est",
            "pre", "un", "re", "de", "dis")
FIELDS = ("tokens", "token_chars", "word_boundary", "morpheme", "subword")
TIMING_KEYS = ("avg_tokenization_time", "tokens_per_second")


def is_word(ch):
    return re.fullmatch(r"\w", ch) is not None


def ends_in_suffix(token):
    body = token[:-1] if token.endswith("\n") else token          # `$` also matches before ONE trailing newline
    return any(body.endswith(s) or token.endswith(s) for s in SUFFIXES)


def line_truth(tokens):
    """(tokens, token_chars, word_boundary, morpheme, subword) of one line's token list"""
    n = len(tokens)
    sub = 0
    for i, t in enumerate(tokens):
        left = i > 0 and is_word(tokens[i - 1][-1]) and is_word(t[0])
        right = i < n - 1 and is_word(t[-1]) and is_word(tokens[i + 1][0])
        sub += bool(left or right)
    return (n, sum(len(t) for t in tokens), sum(any(not is_word(ch) for ch in t) for t in tokens),
            sum(ends_in_suffix(t) for t in tokens), sub)


def truth(token_lists, texts):
    """The CorpusStatistics integers as a dict, and the per-line table"""
    rows = [line_truth(toks) for toks in token_lists]
    out = {"lines": len(texts), "chars": sum(len(t) for t in texts)}
    for k, name in enumerate(FIELDS):
        out[name] = sum(r[k] for r in rows)
    return out, np.array(rows, dtype=np.int64).reshape(len(rows), len(FIELDS))


def dictionaries(st, vocab_size, num_runs=3):
    """The reference's three result dictionaries from the integers (timing keys left out), int / int like it"""
    total_tokens = num_runs * st["tokens"]
    return ({"tokenizer_type": "standard", "vocab_size": vocab_size, "avg_tokens_per_text": total_tokens / st["lines"],
             "avg_token_length": (num_runs * st["token_chars"]) / total_tokens},
            {"word_boundary_ratio": st["word_boundary"] / st["tokens"], "morpheme_ratio": st["morpheme"] / st["tokens"],
             "subword_ratio": st["subword"] / st["tokens"]},
            {"chars_per_token": st["chars"] / st["tokens"], "compression_ratio": st["chars"] / (st["tokens"] * 2)})


def without_timing(d):
    return {k: v for k, v in d.items() if k not in TIMING_KEYS}


def load_golden(golden_dir):
    with open(os.path.join(golden_dir, "g15_corpus_stats.json"), encoding="utf-8") as f:
        return json.load(f)


def py_tokenize(rules, text):
    """HyperbolicTokenizer.tokenize of the reference (hyperbolic_merge.py:414-446) over a rule dict"""
    toks = list(text)
    again = True
    while again:
        again = False
        k = 0
        while k < len(toks) - 1:
            new = rules.get((toks[k], toks[k + 1]))
            if new is None:
                k += 1
            else:
                toks[k:k + 2] = [new]
                again = True
    return toks


def make_tokenizer(vocab, merges, device, cls=None):
    """One of the project's tokenizers holding the rules; on the CPU it gets the oracle-backed engine double"""
    import torch
    from hyptokenizer_amd.tokenizer.hyperbolic_merge import HyperbolicTokenizer
    cls = cls or HyperbolicTokenizer
    emb = torch.zeros(len(vocab), 6)
    emb[:, 0] = 1.0
    kw = {}
    if torch.device(device).type == "cpu":
        from helpers import OracleEngine
        kw["engine"] = OracleEngine(len(vocab) + 1, 6, "lorentz")
    tok = cls(vocab=list(vocab), embeddings=torch.nn.Parameter(emb), max_vocab_size=len(vocab) + 1,
              device=torch.device(device), **kw)
    tok.merge_history = [tuple(m) for m in merges]
    return tok


ALPHABET = list("acdefghilmnoprstuy") + ["_", "7", " ", " ", ".", "-", "\n", "é", "中"]
OUTSIDE = ["Q", "Z", "!", "ß", "\U0001F600", "\t", "٣"]          # never in a vocabulary: travel as negative symbols


def random_case(rng):
    """(vocab, merges, lines): a small rule set with chains and suffix-shaped results, lines of 0..45 characters"""
    pool = list(ALPHABET)
    merges = []
    for _ in range(int(rng.integers(0, 14))):
        if rng.random() < 0.4:                      # a suffix, built from its characters left to right
            s = SUFFIXES[int(rng.integers(0, len(SUFFIXES)))]
            for k in range(1, len(s) - 1):
                merges.append((s[:k], s[k], s[:k + 1]))
                pool.append(s[:k + 1])
            a, b = s[:-1], s[-1]
        else:
            a, b = pool[int(rng.integers(0, len(pool)))], pool[int(rng.integers(0, len(pool)))]
        if len(a) + len(b) > 6:
            continue
        merges.append((a, b, a + b))
        pool.append(a + b)
    vocab = ["<pad>", "<bos>", "<eos>", "<unk>"] + sorted(set(ALPHABET))
    for m in merges:
        for s in m:
            if s not in vocab:
                vocab.append(s)
    chars = ALPHABET + OUTSIDE[: int(rng.integers(0, len(OUTSIDE) + 1))]
    lines = []
    for _ in range(int(rng.integers(0, 9))):
        n = int(rng.integers(0, 41)) if rng.random() < 0.8 else int(rng.integers(0, 3))
        text = ""
        while len(text) < n:                        # single characters, and the rules' own strings so that they fire
            text += pool[int(rng.integers(0, len(pool)))] if rng.random() < 0.3 else chars[int(rng.integers(0, len(chars)))]
        lines.append(text)
    return vocab, merges, lines
