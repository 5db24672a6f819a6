"""Corpus statistics on the GPU (hm_tokstats.hip through tokenizer/corpus_stats.py) against the plain-Python truth of
corpus_stats_cases.py and the reference's recorded dictionaries (tests/golden/g15_corpus_stats.json).  Everything is an
integer: every comparison is exact."""
import numpy as np
import pytest
import torch

import corpus_stats_cases as K

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
TILE = 1024

# a small symbol table for the direct calls: word tokens, non-word tokens, mixed ones, suffixes
STRINGS = ["ab", " ", "ing", "a.", ".a", "-", "ed", "x_1", "é", "un ", " re", "ation", "q\n", "ed\n", "中文", "..."]
WORD, SPACE = 0, 1


def sym_string(s):
    return STRINGS[s] if s >= 0 else chr(-s - 2)


@pytest.fixture(scope="module")
def tables():
    from hyptokenizer_amd.tokenizer import corpus_stats as CS
    attr = torch.from_numpy(CS.attribute_table(STRINGS).view(np.int32)).to(DEV)
    wordmap = torch.from_numpy(CS.word_bitmap().view(np.int32).copy()).to(DEV)
    return attr, wordmap


@pytest.fixture(scope="module")
def g15(golden_dir):
    return K.load_golden(golden_dir)


def run_direct(tables, lines, gaps=None, fill=WORD, **kw):
    """lines: lists of symbols.  gaps[l] slots behind line l's tokens are filled with the valid-looking symbol `fill`."""
    from hyptokenizer_amd.tokenizer import corpus_stats as CS
    gaps = gaps if gaps is not None else [0] * len(lines)
    flat, off = [], [0]
    for line, g in zip(lines, gaps):
        flat += list(line) + [fill] * g
        off.append(len(flat))
    tok = torch.tensor(flat, dtype=torch.int32, device=DEV)
    offsets = torch.tensor(off, dtype=torch.int64, device=DEV)
    lens = torch.tensor([len(x) for x in lines], dtype=torch.int32, device=DEV)
    totals, rows = CS.token_statistics(tok, offsets, lens, tables[0], tables[1], per_line=True, **kw)
    totals2, none = CS.token_statistics(tok, offsets, lens, tables[0], tables[1], per_line=False, **kw)
    assert none is None and torch.equal(totals, totals2)
    return totals.cpu().numpy(), rows.cpu().numpy()


def check_direct(tables, lines, gaps=None, **kw):
    want, want_rows = K.truth([[sym_string(s) for s in line] for line in lines], [""] * len(lines))
    totals, rows = run_direct(tables, lines, gaps, **kw)
    assert totals.tolist() == [want[f] for f in K.FIELDS]
    assert np.array_equal(rows, want_rows)
    return want


def random_line(rng, n, negatives=True):
    line = rng.integers(0, len(STRINGS), n)
    if negatives:
        cps = np.array([ord("Q"), ord("!"), 0x1F600, ord("ß"), 0x10FFFF, 0])
        neg = -(2 + cps[rng.integers(0, len(cps), n)])
        line = np.where(rng.random(n) < 0.15, neg, line)
    return [int(x) for x in line]


def test_golden_cases_exact_totals_and_lines(g15):
    from hyptokenizer_amd.tokenizer import corpus_stats as CS
    for case in g15["cases"]:
        want, want_rows = K.truth(case["tokens"], case["lines"])
        tok = K.make_tokenizer(case["vocab"], case["merges"], DEV)
        st, rows = CS.corpus_statistics_device(tok, case["lines"], per_line=True)
        assert {k: getattr(st, k) for k in want} == want
        assert np.array_equal(rows, want_rows)
        assert st.token_chars == st.chars
        assert tok.corpus_statistics(case["lines"]) == st
        # slabs of 7 lines, of one line, and a slab cut by code points give the single-slab result
        assert CS.corpus_statistics(tok, case["lines"], batch_lines=7) == st
        st1, rows1 = CS.corpus_statistics_device(tok, case["lines"][:40], batch_lines=1, per_line=True)
        assert np.array_equal(rows1, want_rows[:40]) and st1.tokens == int(want_rows[:40, 0].sum())
        assert CS.corpus_statistics_device(tok, case["lines"], slab_code_points=500) == st
        assert CS.corpus_statistics(tok, []) == CS.CorpusStatistics()
        assert tok._token_attributes[0] is tok._batch_encoder()           # built once per encoder state


def test_public_functions_return_the_recorded_dictionaries(g15):
    from hyptokenizer_amd.scripts import compare_tokenizers as CT
    for case in g15["cases"]:
        tok = K.make_tokenizer(case["vocab"], case["merges"], DEV)
        bench = CT.benchmark_hyperbolic_tokenizer(tok, case["lines"])
        assert list(bench) == list(case["benchmark"])
        assert K.without_timing(bench) == K.without_timing(case["benchmark"])
        assert bench["avg_tokenization_time"] > 0 and bench["tokens_per_second"] > 0
        assert K.without_timing(CT.benchmark_hyperbolic_tokenizer(tok, case["lines"], num_runs=1)) == \
            K.without_timing(case["benchmark_one_run"])
        ling = CT.evaluate_linguistic_quality(tok, case["lines"], is_hyperbolic=True)
        comp = CT.evaluate_compression_efficiency(tok, case["lines"], is_hyperbolic=True)
        assert ling == case["linguistic"] and list(ling) == list(case["linguistic"])
        assert comp == case["compression"] and list(comp) == list(case["compression"])
    lines = g15["zero_token_corpus"]["lines"]
    for fn in (lambda: CT.benchmark_hyperbolic_tokenizer(tok, lines), lambda: CT.evaluate_linguistic_quality(tok, lines, True),
               lambda: CT.evaluate_compression_efficiency(tok, lines, True)):
        with pytest.raises(ZeroDivisionError):
            fn()


def test_slots_behind_a_line_are_not_tokens(tables):
    rng = np.random.default_rng(3)
    lines = [random_line(rng, int(n)) for n in rng.integers(0, 12, 40)]
    gaps = [int(g) for g in rng.integers(0, 9, 40)]
    want = check_direct(tables, lines, gaps, fill=WORD)
    assert want == check_direct(tables, lines, gaps, fill=SPACE) == check_direct(tables, lines)
    # every line ends in a word token and the garbage behind it starts with one: nothing may become a sub-word
    totals, rows = run_direct(tables, [[SPACE, WORD]] * 30, [3] * 30, fill=WORD)
    assert totals.tolist() == [60, 90, 30, 0, 0] and rows[:, 4].sum() == 0


def test_empty_and_tiny_inputs(tables):
    from hyptokenizer_amd.tokenizer import corpus_stats as CS
    empty32 = torch.zeros(0, dtype=torch.int32, device=DEV)
    totals, rows = CS.token_statistics(empty32, torch.zeros(1, dtype=torch.int64, device=DEV), empty32, tables[0], tables[1],
                                       per_line=True)
    assert totals.tolist() == [0] * 5 and tuple(rows.shape) == (0, 5)
    for line in ([], [WORD], [WORD, WORD], [WORD, SPACE], [-(2 + ord("Q")), WORD]):
        check_direct(tables, [line])
        check_direct(tables, [line], [5])
    assert check_direct(tables, [[WORD, WORD]])["subword"] == 2 and check_direct(tables, [[WORD]])["subword"] == 0
    check_direct(tables, [[], [], [WORD], [], []])


@pytest.mark.parametrize("n", [TILE - 1, TILE, TILE + 1])
def test_one_line_around_one_tile(tables, n):
    rng = np.random.default_rng(n)
    check_direct(tables, [random_line(rng, n)])
    assert check_direct(tables, [[WORD] * n], [2])["subword"] == n
    check_direct(tables, [[WORD] * (n - 1), [WORD]])           # a line boundary on the last positions of the tile


def test_one_long_line_over_several_tiles(tables):
    n = 3 * TILE + 77
    rng = np.random.default_rng(7)
    line = random_line(rng, n)
    for edge in (TILE, 2 * TILE, 3 * TILE):                    # a sub-word pair straddles every tile edge ...
        line[edge - 2:edge + 2] = [SPACE, WORD, WORD, SPACE]
    want = check_direct(tables, [line])
    for blocks in (1, 2, 3):                                   # ... and every block edge of a smaller grid
        assert check_direct(tables, [line], max_blocks=blocks) == want
    for edge in (TILE, 2 * TILE, 3 * TILE):
        line[edge] = SPACE
    assert check_direct(tables, [line])["subword"] == want["subword"] - 6
    assert check_direct(tables, [[WORD] * n])["subword"] == n


def test_many_lines(tables):
    rng = np.random.default_rng(70)
    lines = [random_line(rng, int(n)) for n in rng.integers(0, 60, 70)]          # more than one wave of lines
    want = check_direct(tables, lines)
    assert check_direct(tables, lines, [int(g) for g in rng.integers(0, 5, 70)], max_blocks=1) == want
    lines = [random_line(rng, int(n)) for n in rng.integers(0, 4, 3000)]         # many lines per tile, empty ones among them
    check_direct(tables, lines)
    check_direct(tables, [random_line(rng, 700), [], random_line(rng, 2000), [WORD], random_line(rng, 1500)], max_blocks=2)


def test_line_of_negative_symbols_only(tables):
    cps = [ord("Q"), ord("z"), ord("!"), ord(" "), 0x4E2D, 0x1F600, ord("_"), 0x10FFFF, 0, ord("9")]
    line = [-(2 + cp) for cp in cps] * 130
    want = check_direct(tables, [line, [WORD, WORD], line[:5]])
    assert want["morpheme"] == 0 and want["token_chars"] == want["tokens"] - 2 + 4
    # neither a table symbol nor a code point: a token of length 0 without flags
    totals, _rows = run_direct(tables, [[len(STRINGS), -1, -(2 + 0x110000), WORD]])
    assert totals.tolist() == [4, 2, 0, 0, 0]


def test_neighbours_never_cross_a_line(tables):
    # word / non-word alternation at every line end: each line is ONE word token, packed without gaps, so a neighbour read
    # across a line boundary would make every token a sub-word
    totals, rows = run_direct(tables, [[WORD]] * 2100)
    assert totals.tolist() == [2100, 4200, 0, 0, 0] and not rows[:, 4].any()
    lines = [[SPACE, WORD], [WORD, SPACE]] * 600
    totals, rows = run_direct(tables, lines)
    assert totals[4] == 0 and not rows[:, 4].any()
    check_direct(tables, [[WORD] * (k % 3 + 1) for k in range(1500)])


def test_seeded_small_cases(tables):
    from hyptokenizer_amd.tokenizer import corpus_stats as CS
    from hyptokenizer_amd.tokenizer.batch_encoder import BatchEncoder

    class Holder:                       # what corpus_statistics_device needs of a tokenizer
        def __init__(self, enc):
            self.enc = enc

        def _batch_encoder(self):
            return self.enc

    rng = np.random.default_rng(2024)
    seen = 0
    for _ in range(300):
        vocab, merges, lines = K.random_case(rng)
        rules = {(a, b): ab for a, b, ab in merges}
        want, want_rows = K.truth([K.py_tokenize(rules, t) for t in lines], lines)
        holder = Holder(BatchEncoder(rules, {t: k for k, t in enumerate(vocab)}, DEV))
        st, rows = CS.corpus_statistics_device(holder, lines, per_line=True, batch_lines=int(rng.integers(1, 6)))
        assert {k: getattr(st, k) for k in want} == want
        assert np.array_equal(rows, want_rows)
        seen += want["subword"] > 0 and want["morpheme"] > 0
    assert seen > 100                   # a property of the seeded generator alone: 162 of these 300 cases hold both kinds
