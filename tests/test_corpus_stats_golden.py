"""Corpus statistics without a GPU: the plain-Python truth against the reference's recorded dictionaries
(tests/golden/g15_corpus_stats.json, written by make_golden_corpus_stats.py from the reference's own three functions), the
two tables of the kernel against ``re``, the host-loop paths, and the argument checks of ``hm_tokstats``."""
import ctypes as C
import re

import numpy as np
import pytest

import corpus_stats_cases as K


@pytest.fixture(scope="module")
def g15(golden_dir):
    return K.load_golden(golden_dir)


def test_truth_reproduces_the_reference_dictionaries(g15):
    assert [c["name"] for c in g15["cases"]] == ["wikitext", "handmade"]
    for case in g15["cases"]:
        st, rows = K.truth(case["tokens"], case["lines"])
        assert rows.shape == (len(case["lines"]), 5)
        bench, ling, comp = K.dictionaries(st, len(case["vocab"]), num_runs=3)
        assert bench == K.without_timing(case["benchmark"]) and list(bench) == list(K.without_timing(case["benchmark"]))
        assert ling == case["linguistic"] and list(ling) == list(case["linguistic"])
        assert comp == case["compression"] and list(comp) == list(case["compression"])
        assert K.dictionaries(st, len(case["vocab"]), num_runs=1)[0] == K.without_timing(case["benchmark_one_run"])
        assert list(case["benchmark"]) == ["tokenizer_type", "vocab_size", "avg_tokenization_time", "tokens_per_second",
                                           "avg_tokens_per_text", "avg_token_length"]
        # merges conserve characters
        assert st["token_chars"] == st["chars"]
        assert K.py_tokenize({(a, b): ab for a, b, ab in case["merges"]}, case["lines"][0]) == case["tokens"][0]
    assert g15["zero_token_corpus"]["raises"] == {k: "ZeroDivisionError" for k in ("benchmark", "linguistic", "compression")}


def test_fixture_holds_the_promised_lines(g15):
    wiki, hand = g15["cases"]
    assert len(wiki["lines"]) == 200 and all(wiki["lines"])
    flat = [t for toks in hand["tokens"] for t in toks]
    for s in K.SUFFIXES:
        assert s in flat and any(t.endswith(s) and t != s for t in flat), s
    assert "" in hand["lines"] and "a" in hand["lines"] and "walked\n" in hand["lines"] and "ed\n" in flat
    assert any(t and all(not K.is_word(ch) for ch in t) for t in hand["lines"])
    assert any(len(t) == 1 and ord(t) > 127 for t in flat)
    assert {"the", "ing", "tion", " the"} <= {t for toks in wiki["tokens"] for t in toks}


def test_attribute_builder_agrees_with_re(g15):
    from hyptokenizer_amd import _lib
    from hyptokenizer_amd.tokenizer import corpus_stats as CS
    nonword = re.compile(r'[^\w]')
    morpheme = re.compile(r'(ion|tion|ation|ment|ance|ence|ly|ish|less|ful|ness|ing|ed|er|est|pre|un|re|de|dis)$')
    strings = sorted({t for c in g15["cases"] for toks in c["tokens"] for t in toks} |
                     {s for c in g15["cases"] for m in c["merges"] for s in m} | {"x\n\n", "ed\n\n", "_", "é", "ly\n"})
    table = CS.attribute_table(strings)
    assert table.dtype == np.uint32 and table.shape == (len(strings),)
    for s, word in zip(strings, table.tolist()):
        assert word >> _lib.TOKSTATS_LEN_SHIFT == len(s)
        assert bool(word & _lib.TOKSTATS_NONWORD) == (nonword.search(s) is not None), s
        assert bool(word & _lib.TOKSTATS_MORPHEME) == (morpheme.search(s) is not None), s
        assert bool(word & _lib.TOKSTATS_FIRST_WORD) == (nonword.search(s[0]) is None), s
        assert bool(word & _lib.TOKSTATS_LAST_WORD) == (nonword.search(s[-1]) is None), s
        assert word & 0xF0 == 0
        assert K.ends_in_suffix(s) == (morpheme.search(s) is not None), s
    assert CS.token_attribute("") == 0

    class Long(str):                      # a token too long for the length field, without building one
        def __len__(self):
            return _lib.TOKSTATS_MAX_LEN + 1
    with pytest.raises(ValueError):
        CS.token_attribute(Long("x"))


def test_bitmap_agrees_with_re_on_every_code_point():
    from hyptokenizer_amd.tokenizer import corpus_stats as CS
    bitmap = CS.word_bitmap()
    assert bitmap.dtype == np.uint32 and bitmap.shape == (0x110000 // 32,)
    bits = np.unpackbits(bitmap.view(np.uint8), bitorder="little").astype(bool)
    every = "".join(map(chr, range(0x110000)))
    want = np.zeros(0x110000, dtype=bool)
    want[[m.start() for m in re.finditer(r"\w", every)]] = True
    assert np.array_equal(bits, want)
    assert 100000 < int(want.sum()) < 0x110000
    for cp in (ord("a"), ord("_"), ord("7"), ord("é"), 0x4E2D, 0x0663):
        assert CS.is_word_codepoint(cp)
    for cp in (0, ord(" "), ord("-"), 0xD800, 0x1F600, 0x10FFFF):
        assert not CS.is_word_codepoint(cp)


def test_truth_and_host_loop_agree(g15):
    from hyptokenizer_amd.tokenizer import corpus_stats as CS
    for case in g15["cases"]:
        st, rows = K.truth(case["tokens"], case["lines"])
        assert [CS.token_list_counts(toks) for toks in case["tokens"]] == [tuple(r) for r in rows.tolist()]
    rng = np.random.default_rng(15)
    for _ in range(100):
        vocab, merges, lines = K.random_case(rng)
        rules = {(a, b): ab for a, b, ab in merges}
        toks = [K.py_tokenize(rules, t) for t in lines]
        got = CS.corpus_statistics_host(lambda t: K.py_tokenize(rules, t), lines)
        st, _rows = K.truth(toks, lines)
        assert {k: getattr(got, k) for k in st} == st


def test_argument_errors_without_a_device():
    from hyptokenizer_amd import _lib
    L = _lib.load()
    p = C.c_void_p(16)                       # never dereferenced: the checks come first
    ok = [p, p, p, 1, 4, p, 1, p, p, None, 0, None]

    def call(**change):
        a = list(ok)
        for k, v in change.items():
            a[int(k[1:])] = v
        return L.hm_tokstats(*a)

    assert call(a3=-1) == _lib.HM_E_ARG and call(a4=-1) == _lib.HM_E_ARG and call(a6=-1) == _lib.HM_E_ARG
    assert call(a10=-1) == _lib.HM_E_ARG
    for k in ("a0", "a1", "a2", "a5", "a7", "a8"):
        assert call(**{k: None}) == _lib.HM_E_ARG, k
    assert call(a3=0) == _lib.HM_E_ARG                          # positions without lines
    assert call(a4=1 << 40) == _lib.HM_E_ARG and call(a6=(1 << 21) + 1) == _lib.HM_E_ARG
    assert b"hm_tokstats" in L.hm_last_error(None)


def test_cpu_tensors_raise_unavailable(g15):
    import torch
    from hyptokenizer_amd import _lib
    from hyptokenizer_amd.tokenizer import corpus_stats as CS
    z32 = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(_lib.HypMergeUnavailable):
        CS.token_statistics(z32, torch.zeros(2, dtype=torch.int64), z32[:1], z32, torch.zeros(0x110000 // 32, dtype=torch.int32))
    case = g15["cases"][1]
    tok = K.make_tokenizer(case["vocab"], case["merges"], "cpu")
    with pytest.raises(_lib.HypMergeUnavailable):               # an unmodified tokenizer has no host path
        tok.corpus_statistics(case["lines"])


def test_host_loop_paths_equal_the_truth(g15):
    """is_hyperbolic=False (the loop over .encode(text).tokens) and a tokenizer whose tokenize is customised"""
    from hyptokenizer_amd.scripts import compare_tokenizers as CT
    from hyptokenizer_amd.tokenizer.hyperbolic_merge import HyperbolicTokenizer

    class Encoding:
        def __init__(self, tokens):
            self.tokens = tokens

    for case in g15["cases"]:
        by_text = dict(zip(case["lines"], case["tokens"]))
        st, _rows = K.truth(case["tokens"], case["lines"])
        _bench, ling, comp = K.dictionaries(st, len(case["vocab"]))

        class Baseline:
            def encode(self, text):
                return Encoding(by_text[text])
        assert CT.evaluate_linguistic_quality(Baseline(), case["lines"]) == ling == case["linguistic"]
        assert CT.evaluate_compression_efficiency(Baseline(), case["lines"]) == comp == case["compression"]

        class Custom(HyperbolicTokenizer):
            def tokenize(self, text):
                return list(by_text[text])
        tok = K.make_tokenizer(case["vocab"], case["merges"], "cpu", cls=Custom)
        got = tok.corpus_statistics(case["lines"])
        assert {k: getattr(got, k) for k in st} == st
        assert CT.evaluate_linguistic_quality(tok, case["lines"], is_hyperbolic=True) == case["linguistic"]
        assert CT.evaluate_compression_efficiency(tok, case["lines"], is_hyperbolic=True) == case["compression"]
        bench = CT.benchmark_hyperbolic_tokenizer(tok, case["lines"])
        assert K.without_timing(bench) == K.without_timing(case["benchmark"]) and list(bench) == list(case["benchmark"])
        assert bench["avg_tokenization_time"] > 0 and bench["tokens_per_second"] > 0
        # customised on the instance
        plain = K.make_tokenizer(case["vocab"], case["merges"], "cpu")
        plain.tokenize = lambda text: list(by_text[text])
        assert plain.corpus_statistics(case["lines"]) == got


def test_zero_token_corpus_divides_by_zero(g15):
    from hyptokenizer_amd.scripts import compare_tokenizers as CT
    from hyptokenizer_amd.tokenizer.hyperbolic_merge import HyperbolicTokenizer

    class Custom(HyperbolicTokenizer):
        def tokenize(self, text):
            return list(text)
    case = g15["cases"][0]
    tok = K.make_tokenizer(case["vocab"], case["merges"], "cpu", cls=Custom)
    lines = g15["zero_token_corpus"]["lines"]
    for fn in (lambda: CT.benchmark_hyperbolic_tokenizer(tok, lines), lambda: CT.evaluate_linguistic_quality(tok, lines, True),
               lambda: CT.evaluate_compression_efficiency(tok, lines, True)):
        with pytest.raises(ZeroDivisionError):
            fn()


def test_load_corpus_and_cli(tmp_path, g15):
    from hyptokenizer_amd.scripts import compare_tokenizers as CT
    p = tmp_path / "corpus.txt"
    p.write_text("  one \n\n two\n   \nthree", encoding="utf-8")
    assert CT.load_corpus(str(p)) == ["one", "two", "three"] and CT.load_corpus(str(p), 2) == ["one", "two"]
    with pytest.raises(ValueError):
        CT.load_hyperbolic_tokenizer(str(tmp_path), "bogus")
    # directories that hold no tokenizer are logged and left out, the file is still written (reference :437-443)
    out = CT.compare_tokenizers(str(p), {"standard": str(tmp_path / "none")}, str(tmp_path / "out"))
    assert out == {"baseline": {}, "hyperbolic": {}} and (tmp_path / "out" / "tokenizer_comparison.json").exists()
