"""FrequencyAwareHyperbolicTokenizer against the G9 goldens captured from the REFERENCE
(tests/golden/make_golden_frequency.py: tokenizer/frequency_aware_hyperbolic_merge.py under the two sign patches), plus
the pieces it is built from.

CPU tests: the class on the oracle-backed engine double with the host pair counter: pair frequencies (contents and
order), per-step picks and scores, candidate counts in the log lines, merges, new rows, the torch RNG state, the bytes
save() writes, load round trips.  The corpus reader against a literal ``for line in open(...)`` loop, the NaN sort order,
the unscored-path selection.  ``tests/test_gpu_frequency.py`` runs the same G9 checks through HIP.
Bar: pairs, counts, (i, j) sequences, log lines and files identical; scores within 1e-6 (the distances come from the
canonical fp32 arithmetic, the reference's from torch)."""
import hashlib
import json
import logging
import os
import random

import numpy as np
import pytest
import torch

from helpers import OracleEngine

SCORE_ATOL = 1e-6
RUNS = ["corpus", "merged", "accumulate", "unscored", "gamma0", "none"]


def load_g9(golden_dir, mode):
    z = np.load(os.path.join(golden_dir, f"g9_frequency_{mode}.npz"))
    with open(os.path.join(golden_dir, f"g9_frequency_{mode}.json"), encoding="utf-8") as f:
        return z, json.load(f)


def oracle_engine(rows, d1, mode):
    return OracleEngine(rows, d1, mode, fast=False)


def write_corpus(meta, n, tmp_path):
    path = tmp_path / f"corpus_{n}.txt"
    path.write_bytes(meta[f"n{n}_corpus_text"].encode("utf-8"))
    return str(path)


class _Logs(logging.Handler):
    def __init__(self):
        super().__init__(logging.INFO)
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


def _freqs(tok):
    return [[list(k), v] for k, v in tok.pair_frequencies.items()]


def _digest(obj) -> str:
    """SHA-256 of ``obj`` as JSON text (a str is taken as the text itself): make_golden_frequency.py's digest."""
    text = obj if isinstance(obj, str) else json.dumps(obj, ensure_ascii=False)
    return hashlib.sha256(text.encode("utf-8")).hexdigest()


def _rng_hash():
    return hashlib.sha256(torch.get_rng_state().numpy().tobytes()).hexdigest()


def check_run(z, meta, mode, n, run, make_engine, tmp_path, device="cpu"):
    """One G9 run: construction (with the corpus pass), the optimize_merges plan, then every recorded output."""
    from hyptokenizer_amd.synthetic import cjk_vocab
    from hyptokenizer_amd.tokenizer import frequency_aware_hyperbolic_merge as FA
    rec = meta[f"n{n}_{run}"]
    corpus = write_corpus(meta, n, tmp_path)
    X = torch.from_numpy(z[f"n{n}_X"])
    vocab = cjk_vocab(n)
    vocab[meta["pipe"]] = "|"
    rows = n + 24
    random.seed(42)
    np.random.seed(42)
    torch.manual_seed(42)
    h = _Logs()
    lg = logging.getLogger(FA.__name__)
    old_level = lg.level
    lg.addHandler(h)
    lg.setLevel(logging.INFO)
    picks = []
    try:
        tok = FA.FrequencyAwareHyperbolicTokenizer(
            vocab=vocab, embeddings=torch.nn.Parameter(X.clone()), corpus_path=corpus if rec["corpus"] else None,
            curvature=1.0, merge_threshold=rec["thr"], device=torch.device(device), max_vocab_size=rows,
            use_approximate_search=False, sign_convention=mode, engine=make_engine(rows, X.shape[1], mode), **rec["kwargs"])
        assert _digest(_freqs(tok)) == rec["freq_after_init_sha256"]
        step_pick = tok._step_pick

        def spy():
            count, best = step_pick()
            picks.append(None if best is None else [best[0], best[1], best[2], count])
            return count, best

        tok._step_pick = spy
        for steps, log_every, with_corpus in rec["plan"]:
            tok.optimize_merges(steps=steps, log_every=log_every, corpus_path=corpus if with_corpus else None)
        del tok._step_pick
    finally:
        lg.removeHandler(h)
        lg.setLevel(old_level)
    want = rec["picks"]
    assert [p is None for p in picks] == [p is None for p in want]
    got_p = [p for p in picks if p is not None]
    want_p = [p for p in want if p is not None]
    assert [(p[0], p[1], p[3]) for p in got_p] == [(p[0], p[1], p[3]) for p in want_p]
    assert np.allclose([p[2] for p in got_p], [p[2] for p in want_p], rtol=0, atol=SCORE_ATOL, equal_nan=True)
    assert h.lines == rec["logs"]
    assert len(tok.pair_frequencies) == rec["freq_final_len"]
    assert _digest(_freqs(tok)) == rec["freq_final_sha256"]
    assert [list(m) for m in tok.merge_history] == rec["merge_history"]
    assert tok.merge_threshold == rec["merge_threshold"]
    assert _rng_hash() == rec["rng"]["torch"]
    got_rows = tok.embeddings.data[n:tok.current_vocab_size].detach().cpu().numpy()
    want_rows = z[f"n{n}_{run}_rows"]
    assert got_rows.shape == want_rows.shape
    assert np.allclose(np.nan_to_num(got_rows, nan=7.0), np.nan_to_num(want_rows, nan=7.0), rtol=0, atol=1e-5)

    out = tmp_path / f"{mode}_{n}_{run}"
    tok.save(str(out))
    assert sorted(os.listdir(out)) == rec["save_files"]
    for fn, want in rec["save_sha256"].items():
        got_text = (out / fn).read_text(encoding="utf-8")
        if fn == "config.json":                             # same keys and values (this package writes them itself)
            assert json.loads(got_text) == rec["save_config"], fn
        else:
            assert _digest(got_text) == want, fn           # byte for byte
    assert rec["reference_load"].startswith("raises")
    back = FA.FrequencyAwareHyperbolicTokenizer.load(str(out), device=torch.device(device), sign_convention=mode,
                                                     engine=make_engine(rows, X.shape[1], mode))
    assert back.vocab == tok.vocab and [list(m) for m in back.merge_history] == rec["merge_history"]
    assert (back.alpha, back.beta, back.gamma) == (tok.alpha, tok.beta, tok.gamma)
    want_keys = [tuple(f"{k[0]}|{k[1]}".split("|")) for k in tok.pair_frequencies]
    assert list(back.pair_frequencies) == want_keys
    assert list(back.pair_frequencies.values()) == list(tok.pair_frequencies.values())
    return tok


@pytest.mark.parametrize("run", RUNS)
@pytest.mark.parametrize("n", [150, 60])
@pytest.mark.parametrize("mode", ["reference", "lorentz"])
def test_g9_on_oracle_engine(golden_dir, mode, n, run, tmp_path):
    z, meta = load_g9(golden_dir, mode)
    check_run(z, meta, mode, n, run, oracle_engine, tmp_path)


def test_g9_covers_what_it_claims(golden_dir):
    """The golden runs exercise the cases they are named after."""
    _z, meta = load_g9(golden_dir, "lorentz")
    for n in (150, 60):
        text = meta[f"n{n}_corpus_text"]
        for piece in ("\r\n", "\x0c", " " if " " in text else "\x85", "\U0001F600", "|", "\n\n"):
            assert piece in text
        plain, merged = meta[f"n{n}_freq_corpus"], meta[f"n{n}_freq_merged"]
        assert _digest(plain) == meta[f"n{n}_corpus"]["freq_after_init_sha256"]
        assert _digest(merged) == meta[f"n{n}_merged"]["freq_final_sha256"]
        merged_tokens = {m[2] for m in meta[f"n{n}_merged"]["merge_history"]}
        assert any(a in merged_tokens or b in merged_tokens for (a, b), _c in merged)
        doubled = [[k, 2 * c] for k, c in plain]
        assert _digest(doubled) == meta[f"n{n}_accumulate"]["freq_final_sha256"]
        assert any("Increasing threshold" in line for line in meta[f"n{n}_none"]["logs"])
        assert meta[f"n{n}_unscored"]["freq_final_len"] == 0 and len(meta[f"n{n}_unscored"]["merge_history"]) == 4
        assert any("|" in a or "|" in b for (a, b), _c in plain)          # a frequencies.json key with two "|"


def test_constructor_refuses_shard_and_incremental():
    from hyptokenizer_amd.synthetic import cjk_vocab, lorentz_table
    from hyptokenizer_amd.tokenizer.frequency_aware_hyperbolic_merge import FrequencyAwareHyperbolicTokenizer
    X = lorentz_table(10, 4)
    for kw in ({"incremental": True}, {"shard": object()}):
        with pytest.raises(ValueError):
            FrequencyAwareHyperbolicTokenizer(cjk_vocab(10), torch.nn.Parameter(X), device=torch.device("cpu"),
                                              max_vocab_size=20, engine=OracleEngine(20, 5, "lorentz"), **kw)


def _tok(n=40, mode="lorentz", thr=0.1, **kw):
    from hyptokenizer_amd.synthetic import cjk_vocab, lorentz_table
    from hyptokenizer_amd.tokenizer.frequency_aware_hyperbolic_merge import FrequencyAwareHyperbolicTokenizer
    X = lorentz_table(n, 6, seed=3, scale=0.05)
    return FrequencyAwareHyperbolicTokenizer(cjk_vocab(n), torch.nn.Parameter(X), merge_threshold=thr,
                                             device=torch.device("cpu"), max_vocab_size=n + 10, sign_convention=mode,
                                             engine=OracleEngine(n + 10, 7, mode), **kw)


# ----------------------------------------------------------------------------------------------
# corpus reading
# ----------------------------------------------------------------------------------------------
READ_CASES = [
    b"",
    b"\n",
    b"a\n",
    b"a",
    b"ab\r\ncd\rde\n\nx",
    b"  lead\ttrail \t\r\n\x0c\xe2\x80\xa8in\x0bside\x1c\x1d\x1e\xc2\x85end\xe2\x80\xa8\n",
    "\U0001F600　x　\r\r\n\n".encode("utf-8"),
]


@pytest.mark.parametrize("data", READ_CASES)
def test_read_corpus_lines_equals_literal_reference_loop(tmp_path, data):
    from hyptokenizer_amd.tokenizer.pair_counter import read_corpus_lines
    p = tmp_path / "c.txt"
    p.write_bytes(data)
    with open(p, "r", encoding="utf-8") as f:
        want = [line.strip() for line in f]
    assert read_corpus_lines(str(p)) == want


def test_read_corpus_lines_is_strict(tmp_path):
    from hyptokenizer_amd.tokenizer.pair_counter import read_corpus_lines
    p = tmp_path / "bad.txt"
    p.write_bytes(b"ok\n\xff\xfe\n")
    with pytest.raises(UnicodeDecodeError):
        read_corpus_lines(str(p))


def reference_count(tok, path):
    """frequency_aware_hyperbolic_merge.py:92-112, literally."""
    freq, total = {}, 0
    with open(path, "r", encoding="utf-8") as f:
        for line in f:
            tokens = tok.tokenize(line.strip())
            for i in range(len(tokens) - 1):
                pair = (tokens[i], tokens[i + 1])
                freq[pair] = freq.get(pair, 0) + 1
                total += 1
    return freq, total


def test_host_counter_equals_literal_reference_loop(tmp_path):
    from hyptokenizer_amd.tokenizer.pair_counter import count_pair_frequencies
    tok = _tok()
    v = tok.vocab
    tok.merge_history = [(v[0], v[1], v[0] + v[1]), (v[0] + v[1], v[2], v[0] + v[1] + v[2])]
    p = tmp_path / "c.txt"
    text = "".join(READ_CASES[5].decode("utf-8")) + (v[0] + v[1] + v[2] + "|" + v[3]) * 3 + "\r\n" + v[1] + v[0] + "\n"
    p.write_bytes(text.encode("utf-8"))
    got = {}
    total = count_pair_frequencies(tok, str(p), got)
    want, want_total = reference_count(tok, str(p))
    assert list(got.items()) == list(want.items()) and total == want_total
    assert (v[0] + v[1] + v[2], "|") in got


# ----------------------------------------------------------------------------------------------
# scoring and selection
# ----------------------------------------------------------------------------------------------
def test_nan_scores_sort_as_python_sorts_them():
    """In sign mode "reference" merged rows are NaN and so are the scores that touch them; the pick is the one
    Python's stable list.sort gives on those keys (np.argsort would put NaN last)."""
    tok = _tok(n=40, mode="lorentz", thr=0.1)
    tok.pair_frequencies = {(tok.vocab[0], tok.vocab[1]): 3}
    i, j, _d = tok._distance_candidates()
    rs = np.random.RandomState(1)
    coh = rs.rand(len(i))
    coh[rs.rand(len(i)) < 0.4] = np.nan
    tok._semantic_coherence_batch = lambda ii, jj: coh.copy()
    scored = tok._find_merge_candidates()
    raw = tok._scores(i, j, np.asarray([float(x) for x in _d.tolist()]))
    want = sorted(zip(i.tolist(), j.tolist(), (-raw).tolist()), key=lambda x: x[2])
    assert np.isnan(raw).any() and not np.isnan(raw).all()
    assert [(a, b) for a, b, _ in scored] == [(a, b) for a, b, _ in want]
    assert [(a, b) for a, b, _ in scored] != [(int(i[k]), int(j[k])) for k in np.argsort(-raw, kind="stable")]


def test_unscored_path_lists_one_candidate_and_counts():
    tok = _tok(n=60, mode="reference", thr=0.1)
    eng = tok._engine
    before = eng.calls["candidates"]
    count, best = tok._step_pick()
    assert count == 60 * 59 // 2 and best[:2] == (0, 1)
    full = tok._find_merge_candidates()
    assert len(full) == count and full[0] == best
    assert eng.calls["candidates"] - before <= 2


def test_gamma_zero_still_draws_one_permutation_per_candidate():
    tok = _tok(gamma=0.0)
    tok.pair_frequencies = {(tok.vocab[0], tok.vocab[1]): 2}
    n_cand = len(tok._distance_candidates()[0])
    torch.manual_seed(9)
    tok._find_merge_candidates()
    got = torch.get_rng_state()
    torch.manual_seed(9)
    for _ in range(n_cand):
        torch.randperm(tok.current_vocab_size)
    assert n_cand > 0 and torch.equal(got, torch.get_rng_state())


def test_is_valid_merge_override_is_called_per_candidate():
    tok = _tok()
    tok.pair_frequencies = {(tok.vocab[0], tok.vocab[1]): 2}
    seen = []

    def valid(a, b):
        seen.append((a, b))
        return a != tok.vocab[0]

    tok._is_valid_merge = valid
    i, j, _d = tok._distance_candidates()
    scored = tok._find_merge_candidates()
    assert len(seen) == len(i)
    assert len(scored) == sum(1 for a in i.tolist() if a != 0) and all(a != 0 for a, _, _ in scored)


def test_candidate_listing_cap_raises():
    tok = _tok(n=30, mode="reference")
    tok.pair_frequencies = {("a", "b"): 1}
    eng = tok._engine
    orig = eng.candidates
    eng.candidates = lambda c, thr, *a, **k: (lambda r: (r[0][:10], r[1][:10], r[2][:10], r[3]))(orig(c, thr))
    with pytest.raises(RuntimeError, match="merge candidates"):
        tok._find_merge_candidates()


def test_load_without_frequency_files(tmp_path):
    from hyptokenizer_amd.tokenizer.frequency_aware_hyperbolic_merge import FrequencyAwareHyperbolicTokenizer
    from hyptokenizer_amd.tokenizer.hyperbolic_merge import HyperbolicTokenizer
    from hyptokenizer_amd.synthetic import cjk_vocab, lorentz_table
    base = HyperbolicTokenizer(cjk_vocab(12), torch.nn.Parameter(lorentz_table(12, 4)), device=torch.device("cpu"),
                               max_vocab_size=20, engine=OracleEngine(20, 5, "lorentz"), sign_convention="lorentz")
    base.save(str(tmp_path))
    tok = FrequencyAwareHyperbolicTokenizer.load(str(tmp_path), device=torch.device("cpu"), sign_convention="lorentz",
                                                 engine=OracleEngine(20, 5, "lorentz"))
    assert (tok.alpha, tok.beta, tok.gamma) == (0.4, 0.4, 0.2) and tok.pair_frequencies == {}
    assert tok.vocab == base.vocab
