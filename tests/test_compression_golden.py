"""CompressionAwareTokenizer against the G8 goldens captured from the REFERENCE (tests/golden/make_golden_compression.py:
tokenizer/compression_aware_tokenizer.py under the two sign patches), plus the pieces it is built from.

CPU tests: the class on the oracle-backed engine double with the host matcher (``HostGreedyMatcher``): candidate
order and scores of a direct ``_find_merge_candidates()``, the ``tokenize_cache`` it leaves, merge sequences, per-step
picks and scores, log lines, the cache after ``optimize_merges``, ``save()`` files and load round trips.
``select_row_major`` against brute force, the host matcher against the reference's literal sorted-vocabulary loop.
``tests/test_gpu_compression.py`` runs the same G8 checks through the HIP matcher.
Bar: (i, j) sequences, cache keys and counts, log lines and files identical; scores within 1e-6 (the distances come
from the canonical fp32 arithmetic, the reference's from torch)."""
import json
import logging
import os
import random

import numpy as np
import pytest
import torch

from helpers import OracleEngine

SCORE_ATOL = 1e-6
RUNS = {"s100": {}, "s5": {"sample_size": 5}, "nocorpus": {}, "none": {}}


def load_g8(golden_dir, mode):
    z = np.load(os.path.join(golden_dir, f"g8_compression_{mode}.npz"))
    with open(os.path.join(golden_dir, f"g8_compression_{mode}.json"), encoding="utf-8") as f:
        return z, json.load(f)


def make_tok(z, meta, mode, n, run, make_engine, device="cpu"):
    from hyptokenizer_amd.synthetic import cjk_vocab
    from hyptokenizer_amd.tokenizer.compression_aware_tokenizer import CompressionAwareTokenizer
    rec = meta[f"n{n}_{run}"]
    X = torch.from_numpy(z[f"n{n}_X"])
    rows = n + 24
    corpus = list(meta[f"n{n}_corpus"]) if rec["corpus"] else None
    return CompressionAwareTokenizer(vocab=cjk_vocab(n), embeddings=torch.nn.Parameter(X.clone()), corpus_sample=corpus,
                                     curvature=1.0, merge_threshold=rec["thr"], device=torch.device(device),
                                     max_vocab_size=rows, use_approximate_search=False, sign_convention=mode,
                                     engine=make_engine(rows, X.shape[1], mode), **rec["kwargs"])


def oracle_engine(rows, d1, mode):
    return OracleEngine(rows, d1, mode, fast=False)


class _Logs(logging.Handler):
    def __init__(self):
        super().__init__(logging.INFO)
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


def check_run(z, meta, mode, n, run, make_engine, tmp_path, device="cpu"):
    """One G8 run: direct candidates + cache, loop (picks, scores, logs, history, cache), save files, load."""
    from hyptokenizer_amd.tokenizer import compression_aware_tokenizer as CA
    rec = meta[f"n{n}_{run}"]
    random.seed(42)
    tok = make_tok(z, meta, mode, n, run, make_engine, device)
    direct = tok._find_merge_candidates()
    want_i, want_j, want_s = (z[f"n{n}_{run}_direct_{f}"] for f in ("i", "j", "negscore"))
    assert [c[0] for c in direct] == want_i.tolist() and [c[1] for c in direct] == want_j.tolist()
    assert np.allclose([c[2] for c in direct], want_s, rtol=0, atol=SCORE_ATOL)
    assert tok.tokenize_cache == rec["cache_after_direct"]
    assert list(tok.tokenize_cache) == list(rec["cache_after_direct"])          # insertion order as well

    picks = []
    best_scored = tok._best_scored

    def spy():
        hit = best_scored()
        if hit is not None:
            picks.append(hit)
        return hit

    tok._best_scored = spy
    h = _Logs()
    lg = logging.getLogger(CA.__name__)
    old_level = lg.level
    lg.addHandler(h)
    lg.setLevel(logging.INFO)
    try:
        tok.optimize_merges(steps=rec["steps"], log_every=rec["log_every"])
    finally:
        lg.removeHandler(h)
        lg.setLevel(old_level)
    del tok._best_scored
    assert [(p[0], p[1]) for p in picks] == [(p[0], p[1]) for p in rec["picks"]]
    assert np.allclose([p[2] for p in picks], [p[2] for p in rec["picks"]], rtol=0, atol=SCORE_ATOL)
    assert h.lines == rec["logs"]
    assert [list(m) for m in tok.merge_history] == rec["merge_history"]
    assert tok.tokenize_cache == rec["cache_after_loop"]
    assert tok.merge_threshold == rec["merge_threshold"]
    got_rows = tok.embeddings.data[n:tok.current_vocab_size].detach().cpu().numpy()
    want_rows = z[f"n{n}_{run}_rows"]
    assert got_rows.shape == want_rows.shape
    assert np.allclose(np.nan_to_num(got_rows, nan=7.0), np.nan_to_num(want_rows, nan=7.0), rtol=0, atol=1e-5)

    out = tmp_path / f"{mode}_{n}_{run}"
    tok.save(str(out))
    assert sorted(os.listdir(out)) == rec["save_files"]
    for fn, want in rec["save_json"].items():
        with open(out / fn, encoding="utf-8") as f:
            assert json.load(f) == want, fn
    emb = torch.load(out / "embeddings.pt", weights_only=True)
    assert list(emb.shape) == rec["save_embeddings_shape"]
    # the reference's own load raises on these files; this package's load returns the tokenizer that was saved
    assert rec["reference_load"].startswith("raises")
    back = CA.CompressionAwareTokenizer.load(str(out), device=torch.device(device), sign_convention=mode,
                                             engine=make_engine(n + 24, emb.shape[1], mode))
    assert back.vocab == tok.vocab and [list(m) for m in back.merge_history] == rec["merge_history"]
    assert (back.compression_weight, back.distance_weight, back.sample_size) == \
        (tok.compression_weight, tok.distance_weight, tok.sample_size)
    assert back.current_vocab_size == tok.current_vocab_size and back.max_vocab_size == tok.max_vocab_size
    k = tok.current_vocab_size
    assert np.array_equal(back.embeddings.data[:k].cpu().numpy().view(np.uint32),
                          tok.embeddings.data[:k].cpu().numpy().view(np.uint32))
    return tok


@pytest.mark.parametrize("run", list(RUNS))
@pytest.mark.parametrize("n", [150, 60])
@pytest.mark.parametrize("mode", ["reference", "lorentz"])
def test_g8_on_oracle_engine(golden_dir, mode, n, run, tmp_path):
    z, meta = load_g8(golden_dir, mode)
    check_run(z, meta, mode, n, run, oracle_engine, tmp_path)


@pytest.mark.parametrize("n", [150, 60])
def test_g8_compression_term_changes_the_merges(golden_dir, n):
    _z, meta = load_g8(golden_dir, "lorentz")
    assert meta[f"n{n}_plain_merge_history"] != meta[f"n{n}_s100"]["merge_history"]


def test_overridden_find_merge_candidates_is_honoured(golden_dir):
    """An instance override of _find_merge_candidates drives the loop (the reference calls it every step)."""
    z, meta = load_g8(golden_dir, "lorentz")
    tok = make_tok(z, meta, "lorentz", 60, "s100", oracle_engine)
    calls = []

    def last_first():
        cands = type(tok)._find_merge_candidates(tok)
        calls.append(len(cands))
        return cands[::-1]

    tok._find_merge_candidates = last_first
    tok.optimize_merges(steps=2, log_every=10 ** 9)
    assert len(calls) == 2 and len(tok.merge_history) == 2
    assert tok.merge_history[0] != tuple(meta["n60_s100"]["merge_history"][0])


def test_constructor_refuses_shard_and_incremental():
    from hyptokenizer_amd.synthetic import cjk_vocab, lorentz_table
    from hyptokenizer_amd.tokenizer.compression_aware_tokenizer import CompressionAwareTokenizer
    X = lorentz_table(10, 4)
    for kw in ({"incremental": True}, {"shard": object()}):
        with pytest.raises(ValueError):
            CompressionAwareTokenizer(cjk_vocab(10), torch.nn.Parameter(X), device=torch.device("cpu"), max_vocab_size=20,
                                      engine=OracleEngine(20, 5, "lorentz"), **kw)


# ----------------------------------------------------------------------------------------------
# row-major selection
# ----------------------------------------------------------------------------------------------
def brute_select(eng, c, thr, k):
    i, j, d, total = eng.candidates(c, thr)
    assert total == len(i)
    order = np.lexsort((j, i))
    i, j, d = i[order], j[order], d[order]
    first = list(zip(i[:k].tolist(), j[:k].tolist(), [float(x) for x in d[:k].tolist()]))
    if len(i) <= k:
        return first, None
    t = np.lexsort((j[k:], i[k:], d[k:]))[0] + k
    return first, (int(i[t]), int(j[t]), float(d[t]))


@pytest.mark.parametrize("mode,n,thr", [("lorentz", 300, 0.1), ("lorentz", 200, 0.05), ("lorentz", 120, 1e-9),
                                        ("reference", 150, 0.1)])
@pytest.mark.parametrize("k", [0, 1, 5, 100, 5000])
@pytest.mark.parametrize("fit", [0, 1 << 16])
def test_select_row_major_equals_brute_force(mode, n, thr, k, fit):
    from hyptokenizer_amd.synthetic import lorentz_table
    from hyptokenizer_amd.tokenizer.compression_aware_tokenizer import select_row_major
    X = lorentz_table(n, 6, seed=n + k, scale=0.05)
    eng = OracleEngine(n, 7, mode)
    eng.set_table(X, n)
    got = select_row_major(eng, 1.0, thr, k, fit=fit)
    assert got == brute_select(eng, 1.0, thr, k)


def test_select_row_major_all_pairs_prefix():
    """Reference sign mode: every pair is a candidate at distance 0 -> (0, 1..k) and the remainder's best (0, k + 1)."""
    from hyptokenizer_amd.synthetic import lorentz_table
    from hyptokenizer_amd.tokenizer.compression_aware_tokenizer import select_row_major
    n = 400
    eng = OracleEngine(n, 5, "reference")
    eng.set_table(lorentz_table(n, 4), n)
    for k in (100, 399, 450):
        first, rest = select_row_major(eng, 1.0, 0.1, k, fit=0)
        want = [(i, j) for i in range(n) for j in range(i + 1, n)][:k]
        assert [(a, b) for a, b, _ in first] == want and all(d == 0.0 for _, _, d in first)
        nxt = [(i, j) for i in range(n) for j in range(i + 1, n)][k]
        assert rest == (nxt[0], nxt[1], 0.0)


# ----------------------------------------------------------------------------------------------
# greedy longest match
# ----------------------------------------------------------------------------------------------
def reference_tokenize_with_vocab(text, vocab):
    """compression_aware_tokenizer.py:91-120, literally (empty entries would loop forever: the callers drop them)."""
    sorted_vocab = sorted(vocab, key=len, reverse=True)
    tokens = []
    i = 0
    while i < len(text):
        matched = False
        for token in sorted_vocab:
            if text[i:].startswith(token):
                tokens.append(token)
                i += len(token)
                matched = True
                break
        if not matched:
            tokens.append(text[i])
            i += 1
    return tokens


EDGE_VOCAB = ["a", "b", "ab", "abc", "bca", "c", "\U0001F600", "\U0001F600a", "xyz", "abcabc", "ab", "", "caba"]
EDGE_LINES = ["", "a", "q", "abcabcabca", "abcabcabca", "cabab\U0001F600aab", "zzzz\U00010348\U00010348",
              "abcabcabcabcabcabcabcabc-tail-1", "abcabcabcabcabcabcabcabc-tail-2", "bcabcaxyzab"]
EDGE_CANDS = ["ab", "abcab", "\U0001F600aab", "zz", "\U00010348\U00010348", "caba" + "b", "-tail-", "q", "a" * 70, "abc"]


def test_host_matcher_equals_literal_reference_loop():
    from hyptokenizer_amd.tokenizer.greedy_matcher import HostGreedyMatcher
    m = HostGreedyMatcher()
    vocab = list(EDGE_VOCAB)
    m.sync(vocab)
    mult = np.arange(1, len(EDGE_LINES) + 1)
    m.set_corpus(EDGE_LINES, mult)
    totals, counts = m.count(EDGE_CANDS, per_line=True)
    nonempty = [t for t in vocab if t]
    for c, cand in enumerate(EDGE_CANDS):
        want = [len(reference_tokenize_with_vocab(t, nonempty + [cand])) for t in EDGE_LINES]
        assert counts[c].tolist() == want, cand
        assert totals[c] == int(np.dot(want, mult))
    # the vocabulary grows in place: only the new strings are added; another list is loaded from scratch
    vocab.append("qzz")
    m.sync(vocab)
    assert m.count(["zz"], per_line=True)[1][0].tolist() == \
        [len(reference_tokenize_with_vocab(t, [v for v in vocab if v] + ["zz"])) for t in EDGE_LINES]
    m.sync(["a"])
    assert m.count(["ab"], per_line=True)[1][0].tolist() == \
        [len(reference_tokenize_with_vocab(t, ["a", "ab"])) for t in EDGE_LINES]


def test_tokenize_with_vocab_equals_literal_reference_loop(golden_dir):
    z, meta = load_g8(golden_dir, "lorentz")
    tok = make_tok(z, meta, "lorentz", 60, "s100", oracle_engine)
    for text in EDGE_LINES:
        for vocab in (EDGE_VOCAB, EDGE_VOCAB + ["abca"], ["a"]):
            assert tok._tokenize_with_vocab(text, vocab) == reference_tokenize_with_vocab(text, [v for v in vocab if v])
