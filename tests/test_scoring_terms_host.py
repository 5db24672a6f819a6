"""The scoring terms that EnhancedFastHyperbolicTokenizer shares with the stand-alone classes (tokenizer/scoring.py),
each against a truth written here: the frequency score against a scalar ``np.log1p`` loop, the coherence of both classes
against each other on the oracle-backed engine double, the greedy tokenisation against the reference's sorted-vocabulary
loop restated, the morpheme predicate against the brute-force scan of the common words, the representative lines of a
corpus sample, and the import rule (a class module imports from its base class and from scoring.py only).  No GPU."""
import ast
import os
import random

import numpy as np
import pytest
import torch

from helpers import OracleEngine

TOKENIZER_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hyptokenizer_amd", "tokenizer")
CLASS_MODULES = {"hyperbolic_merge", "fast_hyperbolic_merge", "enhanced_fast_hyperbolic_merge",
                 "frequency_aware_hyperbolic_merge", "hierarchical_hyperbolic_merge", "compression_aware_tokenizer"}
ALLOWED_BASES = {"frequency_aware_hyperbolic_merge": {"hyperbolic_merge"},
                 "hierarchical_hyperbolic_merge": {"hyperbolic_merge"},
                 "compression_aware_tokenizer": {"hyperbolic_merge"},
                 "enhanced_fast_hyperbolic_merge": {"hyperbolic_merge", "fast_hyperbolic_merge"},
                 "scoring": set()}


def _table(n, d, seed=3):
    from hyptokenizer_amd.synthetic import lorentz_table
    return lorentz_table(n, d, seed=seed, scale=0.1)


def _vocab(n):
    from hyptokenizer_amd.synthetic import cjk_vocab
    return cjk_vocab(n)


def _frequency_aware(n=40, d=8, **kw):
    from hyptokenizer_amd.tokenizer.frequency_aware_hyperbolic_merge import FrequencyAwareHyperbolicTokenizer
    rows = n + 8
    return FrequencyAwareHyperbolicTokenizer(_vocab(n), torch.nn.Parameter(_table(n, d)), merge_threshold=0.7, device=torch.device("cpu"),
                                             max_vocab_size=rows, sign_convention="lorentz",
                                             engine=OracleEngine(rows, d + 1, "lorentz", fast=False), **kw)


def _enhanced(n=40, d=8, frequency=False, hierarchical=False, compression=False, **kw):
    from hyptokenizer_amd.tokenizer.enhanced_fast_hyperbolic_merge import EnhancedFastHyperbolicTokenizer
    rows = n + 8
    return EnhancedFastHyperbolicTokenizer(_vocab(n), torch.nn.Parameter(_table(n, d)), merge_threshold=0.7, device=torch.device("cpu"),
                                           max_vocab_size=rows, sign_convention="lorentz",
                                           engine=OracleEngine(rows, d + 1, "lorentz", fast=False),
                                           use_frequency_aware=frequency, use_hierarchical=hierarchical,
                                           use_adaptive_curvature=False, use_compression_aware=compression, **kw)


# ----------------------------------------------------------------------------------------------
# frequency
# ----------------------------------------------------------------------------------------------
def _frequency_truth(tok, ii, jj):
    pf = tok.pair_frequencies
    top = max(pf.values()) if pf else 1
    out = []
    for a, b in zip(ii.tolist(), jj.tolist()):
        c = pf.get((tok.vocab[a], tok.vocab[b]), 0)
        out.append(np.log1p(c) / np.log1p(top) if top > 0 else 0.0)
    return np.array(out, np.float64)


def test_frequency_scores_equal_scalar_log1p_in_both_classes():
    n = 40
    toks = [_frequency_aware(n), _enhanced(n, frequency=True)]
    rs = np.random.RandomState(5)
    ii = rs.randint(0, n, 300).astype(np.int32)
    jj = rs.randint(0, n, 300).astype(np.int32)
    v = toks[0].vocab

    def table(count, high):
        return {(v[int(a)], v[int(b)]): int(c) for a, b, c in zip(ii[:count], jj[:count], rs.randint(0, high, count))}

    def check(what):
        got = [t._frequency_scores(ii, jj) for t in toks]
        want = _frequency_truth(toks[0], ii, jj)
        for g in got:
            assert g.dtype == np.float64 and np.array_equal(g.view(np.uint64), want.view(np.uint64)), what
        return want

    def assign(d):
        for t in toks:
            t.pair_frequencies = d

    assign({})
    assert not check("empty").any()                                     # max_freq = 1, every count 0
    assign({(v[0], v[1]): 0, (v[2], v[3]): 0})
    assert not check("maximum 0").any()
    shared = table(200, 2 ** 40)                                        # pairs 200.. of the candidates are missing
    assign(shared)
    first = check("filled")
    assert first[:200].any() and not first[np.array([(v[int(a)], v[int(b)]) not in shared for a, b in zip(ii, jj)])].any()
    k = next(k for k in range(200, 300) if (v[int(ii[k])], v[int(jj[k])]) not in shared)
    shared[(v[int(ii[k])], v[int(jj[k])])] = 2 ** 41                    # grown by one pair (the cache key is identity + size): a new maximum
    grown = check("grown")
    assert grown[k] == 1.0 and not np.array_equal(grown, first)
    assign(table(120, 1000))                                            # replaced by another dict
    check("replaced")
    for t in toks:                                                      # one candidate, the scalar entry points
        t.pair_frequencies = {(v[1], v[2]): 3, (v[4], v[5]): 7}
    want = np.log1p(3) / np.log1p(7)
    assert toks[0]._frequency_scores(np.array([1]), np.array([2]))[0] == want
    assert toks[1]._compute_frequency_score(1, 2) == want


def test_frequency_term_switched_off_scores_zero():
    tok = _enhanced(frequency=False)
    assert not tok._frequency_scores(np.array([0, 1]), np.array([2, 3])).any()
    assert not tok._semantic_coherence_batch(np.array([0, 1]), np.array([2, 3])).any()


def test_coherence_is_one_computation_in_both_classes(oracle):
    n, count = 40, 12
    rs = np.random.RandomState(9)
    ii = rs.randint(0, n, count).astype(np.int32)
    jj = (ii + 1 + rs.randint(0, n - 1, count)).astype(np.int32) % n
    runs = []
    for make in (_frequency_aware, lambda: _enhanced(frequency=True)):
        tok = make()
        tok.vocab[3] = tok.vocab[3] * 3                                 # unequal token lengths: the weight is not 1/2
        tok._lens = None
        torch.manual_seed(77)
        coh = tok._semantic_coherence_batch(ii, jj)
        one = tok._compute_semantic_coherence(int(ii[0]), int(jj[0]))
        runs.append((coh, one, torch.get_rng_state().numpy().tobytes()))
    (a, a1, sa), (b, b1, sb) = runs
    assert a.shape == (count,) and np.isfinite(a).all() and (a > 0).all() and (a < 1).all()
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64)) and a1 == b1 and sa == sb
    torch.manual_seed(77)                                               # one randperm(n)[:50] per candidate, in order
    for _ in range(count + 1):
        torch.randperm(n)
    assert torch.get_rng_state().numpy().tobytes() == sa


# ----------------------------------------------------------------------------------------------
# greedy tokenisation
# ----------------------------------------------------------------------------------------------
def _sorted_vocabulary_loop(text, vocab):
    """The reference's loop: the vocabulary sorted by length, longest first; at every position the first entry that
    the rest of the text starts with, else the character.  An empty entry never matches."""
    ordered = sorted(vocab, key=len, reverse=True)
    out, k = [], 0
    while k < len(text):
        piece = next((t for t in ordered if t and text.startswith(t, k)), text[k])
        out.append(piece)
        k += len(piece)
    return out


def test_greedy_tokens_equal_the_sorted_vocabulary_loop():
    from hyptokenizer_amd.tokenizer.scoring import greedy_tokens
    rnd = random.Random(11)

    def word(lo, hi):
        return "".join(rnd.choice("abcd") for _ in range(rnd.randint(lo, hi)))

    cases = [([], "abcabc"), (["ab", "abc"], ""), (["a", "b", "c", "d"], "abcdabcd"), (["", "ab"], "abab"), ([""], "ba"), ([], "")]
    for _ in range(1200):
        vocab = [word(0 if rnd.random() < 0.2 else 1, 4) for _ in range(rnd.randint(0, 9))]
        cases.append((vocab, word(0, 24)))
    assert sum("" in v for v, _ in cases) > 50 and sum(not v for v, _ in cases) > 20
    for vocab, text in cases:
        want = _sorted_vocabulary_loop(text, vocab)
        assert greedy_tokens(text, vocab) == want, (vocab, text)
        assert "".join(want) == text and "" not in want
    from hyptokenizer_amd.tokenizer.compression_aware_tokenizer import CompressionAwareTokenizer
    from hyptokenizer_amd.tokenizer.enhanced_fast_hyperbolic_merge import EnhancedFastHyperbolicTokenizer
    assert CompressionAwareTokenizer._tokenize_with_vocab is EnhancedFastHyperbolicTokenizer._tokenize_with_vocab   # one method behind both
    tok = _enhanced(compression=True, corpus_sample=["abab"])
    assert tok._tokenize_with_vocab("abcab", ["ab", "", "c"]) == ["ab", "c", "ab"]
    tok.use_compression_aware = False                                   # the enhanced guard: plain tokenize
    assert tok._tokenize_with_vocab("abcab", ["ab"]) == tok.tokenize("abcab")


# ----------------------------------------------------------------------------------------------
# morphology
# ----------------------------------------------------------------------------------------------
def _word_set(seed, count=60):
    rnd = random.Random(seed)
    syllables = ["an", "ber", "co", "dis", "ing", "le", "ment", "o", "re", "st", "tion", "un"]
    words = set()
    while len(words) < count:
        words.add("".join(rnd.choice(syllables) for _ in range(rnd.randint(1, 4))))
    return words


def _grams(words, lo=1, hi=6):
    return sorted({w[k:k + n] for w in words for n in range(lo, hi + 1) for k in range(len(w) - n + 1)})


@pytest.mark.parametrize("kind", ["hierarchical", "enhanced"])
def test_potential_morpheme_equals_the_scan_of_the_common_words(kind):
    if kind == "hierarchical":
        from hyptokenizer_amd.tokenizer.hierarchical_hyperbolic_merge import HierarchicalHyperbolicTokenizer
        n, d = 30, 6
        tok = HierarchicalHyperbolicTokenizer(_vocab(n), torch.nn.Parameter(_table(n, d)), device=torch.device("cpu"), max_vocab_size=n + 4,
                                              sign_convention="lorentz", engine=OracleEngine(n + 4, d + 1, "lorentz", fast=False))
    else:
        tok = _enhanced(hierarchical=True)
        tok._wordnet = None                                             # (with nltk installed the class also consults WordNet)
    for seed in (1, 2):                                                 # the second round replaces the set objects
        words = _word_set(seed)
        tok.common_words = words
        tok.common_morphemes = set()
        tokens = _grams(words)
        want = [2 <= len(t) <= 5 and sum(t in w for w in words) >= 5 for t in tokens]
        assert 20 < sum(want) < len(want)
        assert [tok._is_potential_morpheme(t) for t in tokens] == want
    rare = next(t for t, w in zip(tokens, want) if not w)
    tok.common_morphemes = {rare}
    assert tok._is_potential_morpheme(rare)
    assert tok._is_valid_word("xyz") is False and tok._is_valid_word("xaz") and tok._is_valid_word(next(iter(words)))
    if kind == "enhanced":
        tok.use_hierarchical = False
        assert tok._is_potential_morpheme("zzzzzzz") and tok._is_valid_word("zz")


# ----------------------------------------------------------------------------------------------
# compression: representative lines
# ----------------------------------------------------------------------------------------------
def test_representative_lines_and_multiplicities():
    from hyptokenizer_amd.tokenizer.compression_aware_tokenizer import CompressionAwareTokenizer
    stem = "the same twenty chars"[:20]
    texts = [stem + " first", "short", "", stem + " second", "short", stem, "", "another line of text that is long", "x",
             "y", "z", stem + " eleventh", "w"]
    n, d = 20, 6
    ca = CompressionAwareTokenizer(_vocab(n), torch.nn.Parameter(_table(n, d)), corpus_sample=list(texts), device=torch.device("cpu"),
                                   max_vocab_size=n + 4, sign_convention="lorentz", engine=OracleEngine(n + 4, d + 1, "lorentz", fast=False))
    en = _enhanced(compression=True, corpus_sample=list(texts))
    for tok, used in ((ca, texts), (en, texts[:10])):
        _, index, reps, mult = tok._corpus()
        assert int(mult.sum()) == len(used) and len(reps) == len(mult) == len(index)
        assert reps == [t for k, t in enumerate(used) if t[:20] not in {u[:20] for u in used[:k]}]
        assert reps[index[stem]] == stem + " first" and reps[index[""]] == "" and index[""] != index["short"]
        assert mult[index[stem]] == sum(t[:20] == stem for t in used) and mult[index[""]] == 2
        assert tok._corpus() is tok._corpus_state                      # cached while the texts stay the same
    ca.corpus_sample = texts[:4]
    assert int(ca._corpus()[3].sum()) == 4


def test_enhanced_cache_entries_come_from_the_shared_counts():
    """the entries the shared owner leaves are the host loop's: same keys, same order, same counts"""
    texts = ["abab cdcd abab", "", "abab cdcd abab", "dcba" * 6 + " one", "dcba" * 6 + " two"] + ["ab cd " * k for k in range(1, 8)]
    pairs = [(0, 1), (2, 3), (0, 1), (1, 0)]
    filled, looped = _enhanced(compression=True, corpus_sample=texts), _enhanced(compression=True, corpus_sample=texts)
    for tok in (filled, looped):
        tok.vocab[:4] = ["a", "b", "c", "d"]
    filled._original_tokens()
    filled._cached_merge_counts(pairs)
    scores = [looped._compute_compression_score(a, b) for a, b in pairs]
    assert list(filled.tokenize_cache.items()) == list(looped.tokenize_cache.items()) and len(filled.tokenize_cache) > 20
    assert [filled._compute_compression_score(a, b) for a, b in pairs] == scores


# ----------------------------------------------------------------------------------------------
# import direction
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("module", sorted(ALLOWED_BASES))
def test_class_modules_import_only_their_base_and_the_shared_module(module):
    with open(os.path.join(TOKENIZER_DIR, module + ".py"), encoding="utf-8") as f:
        tree = ast.parse(f.read())
    seen = set()
    for node in ast.walk(tree):
        names = []
        if isinstance(node, ast.ImportFrom):
            base = (node.module or "").split(".")
            if node.level == 1 or base[:2] == ["hyptokenizer_amd", "tokenizer"]:
                tail = base if node.level == 1 else base[2:]
                names = [tail[0]] if tail and tail[0] else [a.name for a in node.names]
        elif isinstance(node, ast.Import):
            names = [a.name.split(".")[2] for a in node.names if a.name.startswith("hyptokenizer_amd.tokenizer.")]
        seen.update(names)
    assert not (seen & CLASS_MODULES) - ALLOWED_BASES[module], seen
    if module != "scoring":
        assert "scoring" in seen
