"""GPU: FrequencyAwareHyperbolicTokenizer and the adjacent-pair counter (hm_pairfreq.hip) on the MI355X.

The G9 comparisons live in tests/test_frequency_golden.py (they run there on the oracle double with the host counter);
here they run through the HIP engine, the tokenizer kernel and the pair counter.  The counter is checked against the
host restatement (the reference loop over ``tokenize``) on seeded random corpora -- lines of length 0 and 1, a line of
10^7 identical characters, non-BMP characters and characters outside the vocabulary, several slabs whose new pairs
first occur in later slabs -- and with a forced tiny table that has to grow; the enhanced class's corpus pass against
the host loop (dict order included); and a V = 50 000, d = 100 lorentz scoring step against a host restatement of that
step (picks, scores, torch RNG state)."""
import logging

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_frequency_golden import RUNS, check_run, load_g9  # noqa: E402


def hip_engine(rows, d1, mode):
    from hyptokenizer_amd.engine import MergeEngine
    return MergeEngine(rows, d1, mode, torch.device("cuda"))


@pytest.mark.parametrize("run", RUNS)
@pytest.mark.parametrize("n", [150, 60])
@pytest.mark.parametrize("mode", ["reference", "lorentz"])
def test_g9_through_hip(golden_dir, mode, n, run, tmp_path, monkeypatch):
    from hyptokenizer_amd.tokenizer import pair_counter
    calls = []
    real = pair_counter.count_lines_device
    monkeypatch.setattr(pair_counter, "count_lines_device", lambda *a, **k: calls.append(1) or real(*a, **k))
    z, meta = load_g9(golden_dir, mode)
    check_run(z, meta, mode, n, run, hip_engine, tmp_path, device="cuda")
    rec = meta[f"n{n}_{run}"]
    assert len(calls) == int(rec["corpus"]) + sum(1 for p in rec["plan"] if p[2])


def _tok(n=64, rules=()):
    from hyptokenizer_amd.synthetic import cjk_vocab, lorentz_table
    from hyptokenizer_amd.tokenizer.hyperbolic_merge import HyperbolicTokenizer
    tok = HyperbolicTokenizer(cjk_vocab(n), torch.nn.Parameter(lorentz_table(n, 4)), device=torch.device("cuda"),
                              max_vocab_size=n + 8, sign_convention="lorentz")
    v = tok.vocab
    tok.merge_history = [(v[a], v[b], v[a] + v[b]) for a, b in rules]
    return tok


def _random_lines(rng, alphabet, count, lo, hi):
    return ["".join(rng.choice(alphabet, int(rng.integers(lo, hi + 1)))) for _ in range(count)]


def _host(tok, lines):
    from hyptokenizer_amd.tokenizer.pair_counter import count_pair_frequencies_host
    d = {}
    total = count_pair_frequencies_host(tok, lines, d)
    return d, total


def _device(tok, lines, **kw):
    from hyptokenizer_amd.tokenizer.pair_counter import count_lines_device
    d, timing = {}, {}
    total = count_lines_device(tok, lines, d, timing=timing, **kw)
    return d, total, timing


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("with_rules", [False, True])
def test_counter_equals_host_restatement_on_random_corpora(seed, with_rules):
    rng = np.random.default_rng(seed)
    tok = _tok(rules=[(0, 1), (2, 3), (0, 2), (4, 4)] if with_rules else ())
    alphabet = np.array(tok.vocab[:8] + ["\U0001F600", "\U00010348", "x", "|"])
    lines = _random_lines(rng, alphabet, 400, 0, 40) + ["", tok.vocab[0], "x"] + _random_lines(rng, alphabet, 50, 0, 1)
    lines += ["".join(rng.choice(alphabet[:3], 3000))]
    want, want_total = _host(tok, lines)
    for slab in (1 << 26, 257, 1):                 # one slab, several, one line per slab
        got, total, _t = _device(tok, lines, slab_code_points=slab)
        assert list(got.items()) == list(want.items()) and total == want_total


def test_later_slabs_first_occurrences_and_a_hot_key():
    """Slabs whose new pairs first occur after others were seen: the dict order is that of first occurrence; a line of
    10^7 identical characters (one key) in the middle."""
    tok = _tok()
    v = tok.vocab
    lines = [v[0] + v[1]] * 20 + [v[2] * 10_000_000] + [v[1] + v[0], v[3] + "\U0001F600" + v[0] + v[1]] + [v[5] + v[6]] * 3
    want, want_total = _host(tok, lines)
    got, total, _t = _device(tok, lines, slab_code_points=1 << 20)
    assert list(got.items()) == list(want.items()) and total == want_total
    assert got[(v[2], v[2])] == 10_000_000 - 1
    # accumulation into an existing dict keeps its order and adds after it
    pre = {(v[5], v[6]): 7, ("q", "r"): 1}
    from hyptokenizer_amd.tokenizer.pair_counter import count_lines_device, count_pair_frequencies_host
    a, b = dict(pre), dict(pre)
    count_lines_device(tok, lines[:3] + lines[-3:], a)
    count_pair_frequencies_host(tok, lines[:3] + lines[-3:], b)
    assert list(a.items()) == list(b.items())


def test_forced_small_table_grows_and_recounts():
    rng = np.random.default_rng(7)
    tok = _tok(n=300)
    alphabet = np.array(tok.vocab[:300])
    lines = _random_lines(rng, alphabet, 300, 100, 400)
    want, want_total = _host(tok, lines)
    got, total, timing = _device(tok, lines, initial_capacity=4, slab_code_points=20_000)
    assert list(got.items()) == list(want.items()) and total == want_total
    assert timing["recounts"] > 0 and len(got) > 10_000


def test_one_slab_overflows_its_table_more_than_twice():
    """Initial capacity 4 and ONE slab with tens of thousands of distinct pairs: the count is repeated into tables of 16, 64,
    256, ... slots (a table of `cap` slots overflows above `cap / 2` keys) up to the size that cannot overflow."""
    rng = np.random.default_rng(11)
    tok = _tok(n=300)
    lines = _random_lines(rng, np.array(tok.vocab[:300]), 200, 200, 400)
    want, want_total = _host(tok, lines)
    assert len(want) > 20_000
    got, total, timing = _device(tok, lines, initial_capacity=4)
    assert list(got.items()) == list(want.items()) and total == want_total
    assert timing["recounts"] >= 2


def test_enhanced_corpus_pass_gpu_equals_host(tmp_path, caplog):
    from hyptokenizer_amd.synthetic import cjk_vocab, lorentz_table
    from hyptokenizer_amd.tokenizer.enhanced_fast_hyperbolic_merge import EnhancedFastHyperbolicTokenizer
    rng = np.random.default_rng(3)
    n = 80
    vocab = cjk_vocab(n)
    alphabet = np.array(vocab[:10] + ["\U0001F600", "z"])
    text = "\r\n".join(_random_lines(rng, alphabet, 300, 0, 30)) + "\n\x0c" + vocab[0] * 5 + " " + vocab[1] + "\n"
    path = tmp_path / "corpus.txt"
    path.write_bytes(text.encode("utf-8"))
    kw = dict(use_hierarchical=False, use_adaptive_curvature=False, use_compression_aware=False,
              device=torch.device("cuda"), max_vocab_size=n + 8, sign_convention="lorentz")
    with caplog.at_level(logging.INFO):
        gpu = EnhancedFastHyperbolicTokenizer(vocab, torch.nn.Parameter(lorentz_table(n, 4)), corpus_path=str(path), **kw)
    gpu_logs = [r.getMessage() for r in caplog.records if "pair" in r.getMessage()]
    caplog.clear()
    host = EnhancedFastHyperbolicTokenizer(vocab, torch.nn.Parameter(lorentz_table(n, 4)), **kw)
    host.tokenize = lambda s, _t=host: type(_t).tokenize(_t, s)      # an instance override: the host loop
    with caplog.at_level(logging.INFO):
        host._compute_pair_frequencies(str(path))
    host_logs = [r.getMessage() for r in caplog.records if "pair" in r.getMessage()]
    assert list(gpu.pair_frequencies.items()) == list(host.pair_frequencies.items())
    assert gpu_logs == host_logs and len(gpu_logs) == 2


def test_scoring_step_v50000_against_host_restatement():
    """One lorentz scoring step at V = 50 000, d = 100, about 1 000 candidates: picks, scores and the torch RNG state
    of the HIP path against the reference loop restated on the host (oracle distances, torch.randperm per
    candidate)."""
    from oracle import hm_oracle as O
    from hyptokenizer_amd.synthetic import cjk_vocab, lorentz_table
    from hyptokenizer_amd.tokenizer.frequency_aware_hyperbolic_merge import FrequencyAwareHyperbolicTokenizer
    n, d = 50_000, 100
    X = lorentz_table(n, d, seed=5, scale=0.02)
    tok = FrequencyAwareHyperbolicTokenizer(cjk_vocab(n), torch.nn.Parameter(X), merge_threshold=10.0,
                                            device=torch.device("cuda"), max_vocab_size=n + 8, sign_convention="lorentz")
    dist, _i, _j, _t = tok._get_engine().topk(1.0, 10.0, 1000)
    tok.merge_threshold = float(np.nextafter(np.float32(dist[-1]), np.float32(np.inf)))
    i, j, dd = tok._distance_candidates()
    assert 1000 <= len(i) < 1100
    rng = np.random.default_rng(0)
    v = tok.vocab
    tok.pair_frequencies = {(v[a], v[b]): int(rng.integers(1, 50)) for a, b in zip(i[::3].tolist(), j[::3].tolist())}
    tok.pair_frequencies[("x", "y")] = 77
    torch.manual_seed(123)
    scored = tok._find_merge_candidates()
    state_gpu = torch.get_rng_state()

    torch.manual_seed(123)
    Xn = X.numpy()
    top = max(tok.pair_frequencies.values())
    host = []
    for a, b, dist_ab in zip(i.tolist(), j.tolist(), [float(x) for x in dd.tolist()]):
        w = len(v[b]) / (len(v[a]) + len(v[b]))
        perm = torch.randperm(n)[:50]
        ds = O.coherence_distances(Xn, [a], [b], [np.float32(w)], perm.numpy()[None].astype(np.int32), 1.0, 1)[0]
        kept = [float(ds[k]) for k, idx in enumerate(perm.tolist()) if idx != a and idx != b]
        coh = 0.0 if not kept else 1.0 / (1.0 + np.exp(np.mean(kept) - tok.merge_threshold))
        freq = np.log1p(tok.pair_frequencies.get((v[a], v[b]), 0)) / np.log1p(top)
        host.append((a, b, -(tok.alpha * (1.0 / (1.0 + dist_ab)) + tok.beta * freq + tok.gamma * coh)))
    assert torch.equal(state_gpu, torch.get_rng_state())
    got = {(a, b): s for a, b, s in scored}
    assert set(got) == {(a, b) for a, b, _ in host}
    assert np.allclose([got[(a, b)] for a, b, _ in host], [s for _, _, s in host], rtol=0, atol=1e-6)
    host.sort(key=lambda x: x[2])
    assert scored[0][:2] == host[0][:2]
    torch.manual_seed(123)
    tok.optimize_merges(steps=1, log_every=10 ** 9)
    assert [tuple(m[:2]) for m in tok.merge_history] == [(v[scored[0][0]], v[scored[0][1]])]
