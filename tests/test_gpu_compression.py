"""GPU: CompressionAwareTokenizer and the greedy longest-match counter (hm_greedy.hip) on the MI355X.

The G8 comparisons live in tests/test_compression_golden.py (they run there on the oracle double with the host
matcher); here they run through the HIP engine and the HIP matcher.  The counter itself is checked against the host
restatement (``HostGreedyMatcher``) on random corpora, including a 100 000-code-point line and candidates longer than
64 and 1 024 code points; the incrementally maintained lm against a rebuild; a scoring at V = 50 000 (d = 100,
lorentz, 200 lines); and the row-major selection in the reference sign mode at V = 20 000 (2 * 10^8 candidates)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_compression_golden import RUNS, check_run, load_g8  # noqa: E402


def hip_engine(rows, d1, mode):
    from hyptokenizer_amd.engine import MergeEngine
    return MergeEngine(rows, d1, mode, torch.device("cuda"))


@pytest.mark.parametrize("run", list(RUNS))
@pytest.mark.parametrize("n", [150, 60])
@pytest.mark.parametrize("mode", ["reference", "lorentz"])
def test_g8_through_hip(golden_dir, mode, n, run, tmp_path):
    from hyptokenizer_amd.tokenizer.greedy_matcher import GreedyMatcher
    z, meta = load_g8(golden_dir, mode)
    tok = check_run(z, meta, mode, n, run, hip_engine, tmp_path, device="cuda")
    if meta[f"n{n}_{run}"]["corpus"] and meta[f"n{n}_{run}"]["picks"]:
        assert isinstance(tok._matcher, GreedyMatcher)


def _random_strings(rng, alphabet, count, lo, hi):
    return ["".join(rng.choice(alphabet, int(rng.integers(lo, hi + 1)))) for _ in range(count)]


ALPHABET = np.array(list("abcde") + ["\U0001F600", "一"])


def _matchers(vocab, lines, mult):
    from hyptokenizer_amd.tokenizer.greedy_matcher import GreedyMatcher, HostGreedyMatcher
    dev, host = GreedyMatcher(torch.device("cuda")), HostGreedyMatcher()
    for m in (dev, host):
        m.sync(vocab)
        m.set_corpus(lines, mult)
    return dev, host


def test_count_equals_host_restatement_on_random_corpora():
    rng = np.random.default_rng(5)
    vocab = _random_strings(rng, ALPHABET, 300, 1, 6) + ["", "ab", "ab", "a" * 20]
    lines = _random_strings(rng, ALPHABET, 60, 0, 300) + ["", "a", "\U0001F600"]
    lines += [lines[5]]                                                    # a duplicate line
    mult = rng.integers(1, 5, len(lines))
    cands = [vocab[int(a)] + vocab[int(b)] for a, b in rng.integers(0, len(vocab), (150, 2))]
    cands += ["", "q", lines[3][:70], lines[7][10:80], "".join(lines)[:1100], lines[2] + lines[2]]
    dev, host = _matchers(vocab, lines, mult)
    t_dev, c_dev = dev.count(cands, per_line=True)
    t_host, c_host = host.count(cands, per_line=True)
    assert np.array_equal(c_dev, c_host) and np.array_equal(t_dev, t_host)
    assert np.array_equal(dev.count(cands)[0], t_host)                      # totals alone, counts not written


def test_count_on_a_100k_code_point_line_and_long_candidates():
    rng = np.random.default_rng(6)
    vocab = _random_strings(rng, ALPHABET, 200, 1, 5)
    long_line = "".join(rng.choice(ALPHABET, 100_000))
    lines = [long_line, long_line[:5000], "abc"]
    cands = [long_line[50_000:50_070], long_line[1000:2100], long_line[99_000:], vocab[0] + vocab[1], "abcab"]
    dev, host = _matchers(vocab, lines, [1, 2, 3])
    t_dev, c_dev = dev.count(cands, per_line=True)
    t_host, c_host = host.count(cands, per_line=True)
    assert np.array_equal(c_dev, c_host) and np.array_equal(t_dev, t_host)


def test_vocabulary_list_replaced_after_the_corpus_was_set():
    """Another list object is loaded from scratch: the matcher makes itself a fresh library handle, re-sends the corpus it
    holds and must then count like the host restatement given the same two lists."""
    rng = np.random.default_rng(8)
    first = _random_strings(rng, ALPHABET, 200, 1, 6)
    second = _random_strings(rng, ALPHABET, 150, 1, 7) + first[:20]
    lines = _random_strings(rng, ALPHABET, 50, 0, 300) + [""]
    mult = rng.integers(1, 4, len(lines))
    dev, host = _matchers(first, lines, mult)
    for m in (dev, host):
        m.sync(second)
    cands = [second[int(a)] + second[int(b)] for a, b in rng.integers(0, len(second), (100, 2))] + first[150:160]
    t_dev, c_dev = dev.count(cands, per_line=True)
    t_host, c_host = host.count(cands, per_line=True)
    assert np.array_equal(c_dev, c_host) and np.array_equal(t_dev, t_host)
    assert np.array_equal(dev.longest()[0], _host_lm(second, lines))


def _host_lm(vocab, lines):
    entries = {t for t in vocab if t}
    longest = max(map(len, entries))
    lm = []
    for text in lines:
        for p in range(len(text)):
            best = 1
            for w in range(min(longest, len(text) - p), 1, -1):
                if text[p:p + w] in entries:
                    best = w
                    break
            lm.append(best)
    return np.array(lm, np.int32)


def test_incremental_lm_equals_rebuild():
    from hyptokenizer_amd.tokenizer.greedy_matcher import GreedyMatcher
    rng = np.random.default_rng(7)
    vocab = _random_strings(rng, ALPHABET, 300, 1, 4)
    lines = _random_strings(rng, ALPHABET, 40, 0, 400)
    extra = _random_strings(rng, ALPHABET, 50, 2, 9) + [lines[0][:30]]
    inc = GreedyMatcher(torch.device("cuda"))
    inc.sync(vocab)
    inc.set_corpus(lines)
    grown = list(vocab)
    inc.sync(grown)
    for t in extra:                       # one string per call, the path of a merge loop
        grown.append(t)
        inc.sync(grown)
    batch = GreedyMatcher(torch.device("cuda"))
    batch.set_corpus(lines)
    b_list = list(vocab)
    batch.sync(b_list)
    b_list += extra                        # 51 strings in one call: the direct path, not a rebuild
    batch.sync(b_list)
    full = GreedyMatcher(torch.device("cuda"))
    full.set_corpus(lines)
    full.sync(vocab + extra)               # one rebuild through the hashed set
    want_lm = _host_lm(vocab + extra, lines)
    for m in (inc, batch, full):
        lm, base = m.longest()
        assert np.array_equal(lm, want_lm)
        assert np.array_equal(base, full.longest()[1])
    cands = extra[:10] + [lines[1][:12]]
    assert np.array_equal(inc.count(cands, per_line=True)[1], full.count(cands, per_line=True)[1])


def test_scoring_at_v50000_equals_host_restatement():
    """One scoring of the class at V = 50 000, d = 100, lorentz: the first 100 row-major candidates over 200 lines."""
    from hyptokenizer_amd.synthetic import cjk_vocab, lorentz_table
    from hyptokenizer_amd.tokenizer.compression_aware_tokenizer import CompressionAwareTokenizer, select_row_major
    from hyptokenizer_amd.tokenizer.greedy_matcher import HostGreedyMatcher
    V, d = 50_000, 100
    X = lorentz_table(V, d, seed=42, scale=0.05)
    vocab = cjk_vocab(V)
    tok = CompressionAwareTokenizer(vocab, torch.nn.Parameter(X), corpus_sample=None, max_vocab_size=V + 64,
                                    device=torch.device("cuda"), sign_convention="lorentz")
    eng = tok._get_engine()
    dd, _, _, _ = eng.topk(1.0, 10.0, 3000)
    tok.merge_threshold = float(dd[-1])
    first, rest = select_row_major(eng, 1.0, tok._search_threshold(), 100)
    assert len(first) == 100 and rest is not None
    rng = np.random.default_rng(8)
    near = [vocab[i] + vocab[j] for i, j, _ in first]
    lines = []
    for _ in range(200):
        parts, size = [], 0
        while size < 256:
            piece = near[int(rng.integers(len(near)))] if rng.random() < 0.5 else vocab[int(rng.integers(V))]
            parts.append(piece)
            size += len(piece)
        lines.append("".join(parts)[:256])
    tok.corpus_sample = lines
    tok.optimize_merges(steps=3, log_every=10 ** 9)                # the vocabulary now holds multi-character strings
    assert tok.current_vocab_size == V + 3
    first, _ = select_row_major(eng, 1.0, tok._search_threshold(), 100)
    vocab = tok.vocab
    pairs = [(i, j) for i, j, _ in first]
    totals, counts = tok._greedy_counts(pairs, per_line=True)
    host = HostGreedyMatcher()
    host.sync(vocab)
    host.set_corpus(lines)
    h_tot, h_counts = host.count([vocab[i] + vocab[j] for i, j in pairs], per_line=True)
    assert np.array_equal(counts, h_counts) and np.array_equal(totals, h_tot)
    assert (counts < 256).any()
    lm, _ = tok._matcher.longest()
    assert lm.max() >= 2
    best = tok._best_scored()
    assert best is not None and tok.last_timing["matcher_device_ms"] > 0


def test_selection_in_reference_mode_at_v20000():
    from hyptokenizer_amd.engine import MergeEngine
    from hyptokenizer_amd.synthetic import lorentz_table
    from hyptokenizer_amd.tokenizer.compression_aware_tokenizer import select_row_major
    V, d = 20_000, 16
    table = torch.zeros((V, d + 1), device="cuda")
    table[:] = lorentz_table(V, d, seed=3).cuda()
    eng = MergeEngine(V, d + 1, "reference", torch.device("cuda"))
    eng.set_table(table, V)
    assert eng.topk(1.0, 0.1, 0, count=True)[3] == V * (V - 1) // 2
    first, rest = select_row_major(eng, 1.0, 0.1, 100)
    assert first == [(0, j, 0.0) for j in range(1, 101)]
    assert rest == (0, 101, 0.0)
    first, rest = select_row_major(eng, 1.0, 0.1, V + 5)          # past the first row
    assert first[:V - 1] == [(0, j, 0.0) for j in range(1, V)] and first[V - 1:] == [(1, j, 0.0) for j in range(2, 8)]
    assert rest == (1, 8, 0.0)
