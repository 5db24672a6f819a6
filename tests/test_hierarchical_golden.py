"""HierarchicalHyperbolicTokenizer against the G10 goldens captured from the REFERENCE
(tests/golden/make_golden_hierarchical.py: tokenizer/hierarchical_hyperbolic_merge.py under the two sign patches, phase
ranges shortened the same way in both codes).

CPU tests: the class on the oracle-backed engine double, with the host restatements of the n-gram counter and of the class
minima: corpus statistics, both predicates, log lines, merges, thresholds, new rows, hierarchical_data.json, the empty
corpus error; the list path (a subclass overriding a filter) against the same goldens; the selection pieces.
``tests/test_gpu_hierarchical.py`` runs the same G10 checks through HIP."""
import json
import logging
import os

import numpy as np
import pytest
import torch

from helpers import OracleEngine

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MODES = ("reference", "lorentz")
RUNS = ("phases", "target", "p1", "p1break", "p2", "p2df", "p3", "p3cap")


def load_g10(mode):
    z = np.load(os.path.join(GOLDEN, f"g10_hierarchical_{mode}.npz"))
    with open(os.path.join(GOLDEN, f"g10_hierarchical_{mode}.json"), encoding="utf-8") as f:
        return z, json.load(f)


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


class _Logs(logging.Handler):
    def __init__(self):
        super().__init__(logging.INFO)
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


def write_corpus(meta, tmp_path):
    p = tmp_path / "corpus.txt"
    p.write_bytes(meta["corpus_text"].encode("utf-8"))
    return str(p)


def make(cls, z, meta, n, mode, corpus, device, engine):
    X = torch.from_numpy(z[f"n{n}_X"])
    rows = n + 200
    return cls(vocab_for(n), torch.nn.Parameter(X.clone()), corpus_path=corpus, device=torch.device(device),
               max_vocab_size=rows, use_approximate_search=False, sign_convention=mode,
               engine=engine(rows, X.shape[1], mode) if engine else None)


def check_stats(tok, meta, n):
    st = meta[f"n{n}_stats"]
    assert [[k, v] for k, v in tok.token_frequencies.items()] == st["token_frequencies"]
    assert sorted(tok.common_morphemes) == st["common_morphemes"]
    assert sorted(tok.common_words) == st["common_words"]
    assert [bool(tok._is_potential_morpheme(p)) for p in meta["probes"]] == st["is_potential_morpheme"]
    assert [bool(tok._is_valid_word(p)) for p in meta["probes"]] == st["is_valid_word"]


def check_run(cls, z, meta, n, run, mode, tmp_path, device="cpu", engine=None):
    from hyptokenizer_amd.tokenizer import hierarchical_hyperbolic_merge as HH
    rec = meta[f"n{n}_{run}"]
    if run in meta["scenarios"]:                 # a table built for one phase, string sets set on the object
        spec = dict(meta["scenarios"][run], target=None)
        X = torch.from_numpy(z[f"n{n}_{run}_X"])
        rows = n + 200
        tok = cls(list(rec["vocab"]), torch.nn.Parameter(X.clone()), device=torch.device(device), max_vocab_size=rows,
                  use_approximate_search=False, sign_convention=mode,
                  engine=engine(rows, X.shape[1], mode) if engine else None)
        tok.common_morphemes = set(spec["morphemes"])
        tok.common_words = set(spec["words"])
    else:
        spec = meta["runs"][run]
        corpus = write_corpus(meta, tmp_path) if spec["corpus"] else None
        tok = make(cls, z, meta, n, mode, corpus, device, engine)
    tok.PHASE_STEPS = tuple(spec["steps"])
    h = _Logs()
    lg = logging.getLogger(HH.__name__)
    old = lg.level
    lg.addHandler(h)
    lg.setLevel(logging.INFO)
    try:
        tok.optimize_merges(target_vocab_size=(n + spec["target"]) if spec["target"] else None)
    finally:
        lg.removeHandler(h)
        lg.setLevel(old)
    assert [list(m) for m in tok.merge_history] == rec["merge_history"]
    assert h.lines == rec["logs"]
    assert tok.merge_threshold == rec["merge_threshold"]
    assert tok.current_vocab_size == rec["vocab_size"]
    got = tok.embeddings.data[n:tok.current_vocab_size].detach().cpu().numpy()
    want = z[f"n{n}_{run}_rows"]
    assert got.shape == want.shape
    # the scenario tables hold rows of norm ~6 (far apart), where 1e-5 relative is the midpoint's parity with torch
    assert np.allclose(np.nan_to_num(got, nan=7.0), np.nan_to_num(want, nan=7.0), rtol=1e-5, atol=1e-5)
    if "hierarchical_data" in rec:
        out = tmp_path / f"saved_{n}_{run}"
        tok.save(str(out))
        with open(out / "hierarchical_data.json") as f:
            data = json.load(f)
        assert data == rec["hierarchical_data"]            # lists sorted on both sides
        back = cls.load(str(out), device=torch.device(device), sign_convention=mode,
                        engine=engine(tok.max_vocab_size, tok.embeddings.shape[1], mode) if engine else None)
        assert back.common_words == tok.common_words and back.common_morphemes == tok.common_morphemes
        assert back.vocab == tok.vocab and back.language == "english"
    return tok


def oracle(rows, d1, mode):
    return OracleEngine(rows, d1, mode, fast=False)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", (150, 60))
def test_g10_statistics_and_predicates(mode, n, tmp_path):
    from hyptokenizer_amd.tokenizer import HierarchicalHyperbolicTokenizer
    z, meta = load_g10(mode)
    tok = make(HierarchicalHyperbolicTokenizer, z, meta, n, mode, write_corpus(meta, tmp_path), "cpu", oracle)
    check_stats(tok, meta, n)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", (150, 60))
@pytest.mark.parametrize("run", RUNS)
def test_g10_runs_class_minima(mode, n, run, tmp_path):
    from hyptokenizer_amd.tokenizer import HierarchicalHyperbolicTokenizer
    z, meta = load_g10(mode)
    check_run(HierarchicalHyperbolicTokenizer, z, meta, n, run, mode, tmp_path, engine=oracle)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("run", ("phases", "p1", "p1break", "p2", "p2df", "p3", "p3cap"))
def test_g10_runs_list_path(mode, run, tmp_path):
    """A subclass that overrides a filter takes the reference's list code: the same goldens."""
    from hyptokenizer_amd.tokenizer import HierarchicalHyperbolicTokenizer

    class Listed(HierarchicalHyperbolicTokenizer):
        def _filter_word_valid(self, candidates):
            return super()._filter_word_valid(candidates)

    z, meta = load_g10(mode)
    tok = check_run(Listed, z, meta, 60, run, mode, tmp_path, engine=oracle)
    assert tok._cm is None                     # the class minima were never built


@pytest.mark.parametrize("mode", MODES)
def test_g10_empty_corpus_fails_like_the_reference(mode, tmp_path):
    from hyptokenizer_amd.tokenizer import HierarchicalHyperbolicTokenizer
    z, meta = load_g10(mode)
    p = tmp_path / "empty.txt"
    p.write_text("")
    with pytest.raises(Exception) as ei:
        make(HierarchicalHyperbolicTokenizer, z, meta, 60, mode, str(p), "cpu", oracle)
    assert [type(ei.value).__name__, str(ei.value)] == meta["empty_corpus_error"]


def test_refuses_shard_and_incremental():
    from hyptokenizer_amd.tokenizer import HierarchicalHyperbolicTokenizer
    X = torch.nn.Parameter(torch.zeros(4, 3))
    with pytest.raises(ValueError):
        HierarchicalHyperbolicTokenizer(list("abcd"), X, device=torch.device("cpu"), max_vocab_size=8,
                                        engine=oracle(8, 3, "lorentz"), incremental=True)
    with pytest.raises(ValueError):
        HierarchicalHyperbolicTokenizer(list("abcd"), X, device=torch.device("cpu"), max_vocab_size=8,
                                        engine=oracle(8, 3, "lorentz"), shard=object())


def test_g10_scenarios_make_the_rules_decide():
    """The scenario goldens are not degenerate: in the sign-corrected mode each one's first pick is decided by the rule it
    was built for, and the threshold transitions are in the logs."""
    _, meta = load_g10("lorentz")
    for n in (150, 60):
        first = {run: meta[f"n{n}_{run}"]["merge_history"][:1] for run in ("p1", "p2", "p2df", "p3")}
        assert first == {"p1": [["x", "z", "xz"]], "p2": [["m", "nt", "mnt"]], "p2df": [["gh", "t", "ght"]],
                         "p3": [["q", "rs", "qrs"]]}
        assert meta[f"n{n}_p1break"]["logs"][2].startswith("Completed Phase 1 with 0 merges")
        assert sum(ln.startswith("Increasing threshold") for ln in meta[f"n{n}_p2"]["logs"]) == 3
        cap = meta[f"n{n}_p3cap"]
        assert cap["merge_threshold"] >= 1.0 and cap["logs"][-2].startswith("Completed Phase 3 with 0 merges")


def test_classes_cover_the_phase_rules():
    from hyptokenizer_amd.tokenizer.class_minima import (N_CLASSES, P1_LE2, P1_LE3, P3_BOOSTED, class_of, token_code)
    toks = ["", "a", "b", "ab", "bc", "abc", "bcd", "abcd", "bcdf", "éé", "\U0001D518"]
    assert len({class_of(a, b) for a in range(10) for b in range(10)}) == N_CLASSES
    for s in toks:
        for t in toks:
            q = class_of(token_code(s), token_code(t))
            assert (q in P1_LE2) == (len(s) <= 2 and len(t) <= 2)
            assert (q in P1_LE3) == (len(s) <= 3 and len(t) <= 3)
            m = s + t
            heur = len(m) >= 3 and any(ch in "aeiou" for ch in m)
            assert (q in P3_BOOSTED) == heur


def test_ngram_host_counts_match_the_reference_loop():
    from collections import Counter
    from hyptokenizer_amd.tokenizer.ngram_counter import ngram_counts_host
    words = ["", "a", "ab", "abcabc", "\U0001D518\U0001D518x", "ééééé"]
    weights = [3, 1, 2, 5, 7, 1]
    want = Counter()
    for w, k in zip(words, weights):
        for _ in range(k):
            for n in range(2, min(6, len(w) + 1)):
                for i in range(len(w) - n + 1):
                    want[w[i:i + n]] += 1
    assert ngram_counts_host(words, weights) == dict(want)
    df = ngram_counts_host(words, None, distinct=True)
    assert df["ab"] == 2 and df["bc"] == 1 and df["éé"] == 1
