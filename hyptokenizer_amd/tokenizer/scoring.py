"""What the scoring tokenizer classes share: one owner for each term of a merge score.

``EnhancedFastHyperbolicTokenizer`` scores a candidate by pair frequency + coherence, morphology and compression; each
of those terms is also a stand-alone class of the reference (``FrequencyAwareHyperbolicTokenizer``,
``HierarchicalHyperbolicTokenizer``, ``CompressionAwareTokenizer``).  Both users of a term inherit it from the mixin
below, so no class module imports another one except its base class:

* ``FrequencyTerm``   -- ``pair_frequencies`` (the corpus pass of pair_counter.py), ``log1p(freq) / log1p(max freq)``,
  the coherence of a simulated merge (``coherence_batch``: one ``hm_coherence_batch`` launch), ``frequencies.json``;
* ``MorphologyTerm``  -- the corpus statistics (ngram_counter.py), the potential-morpheme and valid-word predicates;
* ``CompressionTerm`` -- greedy longest-match tokenisation, the representative lines of a corpus sample, the matcher
  (greedy_matcher.py) and the ``merge_{i}_{j}_{text[:20]}`` entries of ``tokenize_cache``.

A mixin has no ``__init__``: the tokenizer keeps ``pair_frequencies``, ``token_frequencies``, ``common_morphemes``,
``common_words``, ``corpus_sample`` and ``tokenize_cache`` as plain attributes (callers assign them), and the caches
here are keyed on the identity and size of those objects.  The enhanced class switches a term off with its
``use_*`` flag (always on in the stand-alone classes).  Nothing here owns a logger: a mixin logs through ``_logger``,
which every class sets to the logger of its own module.

Also here: the candidate selection ``select_row_major`` and the ``torch.randperm`` prefix helper.
"""
from __future__ import annotations

import ctypes as C
import json
import logging
import os
import re
import time
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import pair_counter
from .greedy_matcher import make_matcher
from .ngram_counter import corpus_statistics, frequent_substrings

COHERENCE_SAMPLES = 50       # sampled rows per candidate (reference enhanced :324, frequency-aware :144)
ROW_MAJOR_FIT = 1 << 16      # candidate totals up to this size are listed in one call
PREFIXES = {"re", "un", "in", "im", "il", "ir", "dis", "en", "em", "non", "de", "pre", "pro", "mis"}
SUFFIXES = {"ing", "ed", "er", "est", "ly", "ity", "ment", "ness", "able", "ible", "al", "ial"}
_VOWEL = re.compile(r"[aeiou]")


def now_ms() -> float:
    return time.perf_counter() * 1e3


# ----------------------------------------------------------------------------------------------
# torch.randperm prefixes
# ----------------------------------------------------------------------------------------------
_RANDPERM_HELPER_OK = None


def _randperm_helper_ok() -> bool:
    """One-time check of the library's MT19937 helper against THIS torch build's ``torch.randperm`` -- prefix values and
    the generator state left behind, at a small n and at n = 100 003 (the helper follows randperm's 32-bit draw and
    Fisher-Yates order; a build that changes either would otherwise sample other coherence rows than the reference).
    On a mismatch the helper is not used again: plain ``torch.randperm`` calls."""
    global _RANDPERM_HELPER_OK
    if _RANDPERM_HELPER_OK is None:
        _RANDPERM_HELPER_OK = True                    # (so that the calls below go through the helper)
        keep = torch.get_rng_state()
        ok = True
        try:
            for n, ns, count in ((37, 5, 3), (100003, COHERENCE_SAMPLES, 2)):
                torch.manual_seed(1234567 + n)
                want = np.stack([torch.randperm(n)[:ns].numpy() for _ in range(count)]).astype(np.int32)
                st_want = torch.get_rng_state()
                torch.manual_seed(1234567 + n)
                got = randperm_prefixes(n, ns, count)
                ok = ok and np.array_equal(got, want) and torch.equal(torch.get_rng_state(), st_want)
        except Exception:
            ok = False
        finally:
            torch.set_rng_state(keep)
        _RANDPERM_HELPER_OK = bool(ok)
        if not ok:
            logging.getLogger(__name__).warning(
                "hm_randperm_prefix disagrees with this torch build's randperm: using torch.randperm")
    return _RANDPERM_HELPER_OK


def randperm_prefixes(n: int, ns: int, count: int) -> np.ndarray:
    """``[torch.randperm(n)[:ns] for _ in range(count)]`` as an int32 ``[count, ns]`` array, consuming torch's
    CPU generator exactly as those calls do.  Served by the library's host helper ``hm_randperm_prefix`` (the
    generator's MT19937 state is read from and written back to ``torch.get/set_rng_state``); plain
    ``torch.randperm`` calls when that is not possible (n >= 2^32 / 20, an unexpected state layout)."""
    out = np.empty((count, ns), np.int32)
    if count == 0 or ns == 0:
        for _ in range(count):
            torch.randperm(n)
        return out
    st = torch.get_rng_state()
    if st.numel() == 5056 and n < (2 ** 32 - 1) // 20 and ns <= 4096 and _randperm_helper_ok():
        from .. import _lib
        raw = st.numpy().copy()
        # CPUGeneratorImplStateLegacy: u64 seed | i32 left | i32 seeded | u64 next | u64 state[624] | ...
        left = raw[8:12].view(np.int32)
        seeded = raw[12:16].view(np.int32)
        nxt = raw[16:24].view(np.uint64)
        words = raw[24:24 + 624 * 8].view(np.uint64)
        if seeded[0] == 1 and 1 <= left[0] <= 624:
            mt = words.astype(np.uint32)
            c_left, c_next = C.c_int32(int(left[0])), C.c_uint32(int(nxt[0]))
            rc = _lib.load().hm_randperm_prefix(C.c_void_p(mt.ctypes.data), C.byref(c_left), C.byref(c_next), int(n), int(ns),
                                                int(count), C.c_void_p(out.ctypes.data))
            if rc == 0:
                words[:] = mt
                left[0] = c_left.value
                nxt[0] = c_next.value
                torch.set_rng_state(torch.from_numpy(raw))
                return out
    for t in range(count):
        out[t] = torch.randperm(n)[:ns].numpy()
    return out


# ----------------------------------------------------------------------------------------------
# coherence of a simulated merge
# ----------------------------------------------------------------------------------------------
def _row_means(dist: np.ndarray, keep: np.ndarray) -> np.ndarray:
    """``np.mean`` of the kept entries of every row in float64 -- the value ``np.mean(list_of_floats)``
    gives the reference (``:340``), same summation order: full rows go through one reduction over the
    contiguous axis (numpy's pairwise sum, as for a 1-D array); rows with skipped samples one by one."""
    d64 = dist.astype(np.float64)
    out = np.empty(d64.shape[0], np.float64)
    full = keep.all(axis=1)
    if full.any():
        out[full] = np.add.reduce(np.ascontiguousarray(d64[full]), axis=1) / d64.shape[1]
    for r in np.nonzero(~full)[0].tolist():
        vals = d64[r][keep[r]]
        out[r] = np.mean(vals) if vals.size else np.nan       # empty: the caller returns 0.0 (:335-336)
    return out


def coherence_batch(eng, ii: np.ndarray, jj: np.ndarray, w: np.ndarray, draw, c: float, merge_threshold: float,
                    shard=None) -> np.ndarray:
    """``1 / (1 + exp(mean distance - merge_threshold))`` of every candidate's simulated merged embedding
    ``exp_map(x_i, w * log_map(x_i, x_j))`` to its sampled rows, 0.0 when no sample is kept (the reference's
    ``_compute_semantic_coherence`` of the enhanced class ``:291-346`` and of FrequencyAwareHyperbolicTokenizer
    ``:114-166``, which are the same arithmetic).  ``draw(k)`` returns the next ``k`` candidates' samples (one
    ``torch.randperm(n)[:50]`` each): the RNG calls happen in list order; midpoints and all ``count x 50`` distances
    are ONE kernel launch (two when the list is long: the second half's samples are drawn while the first half runs);
    mean / sigmoid in float64 as ``np.mean`` / ``np.exp`` give them."""
    count = len(ii)
    if count == 0:
        return np.zeros(0, np.float64)
    if shard is not None:
        from ..sharding import sharded_coherence
        samples = draw(count)          # (every rank draws the same samples: same seeded generator)
        dist = sharded_coherence(eng, shard, ii, jj, w.astype(np.float32), samples, c)
    elif count >= 64 and hasattr(eng, "coherence_distances_begin"):
        # two halves, samples drawn in candidate order as ever: while the first half's kernel and result copy run, the
        # host draws the second half's permutations (the long pole: one MT19937 pass over n draws per candidate)
        h = count // 2
        s0 = draw(h)
        pend = eng.coherence_distances_begin(ii[:h], jj[:h], w[:h].astype(np.float32), s0, c)
        s1 = draw(count - h)
        d1 = eng.coherence_distances(ii[h:], jj[h:], w[h:].astype(np.float32), s1, c)
        samples = np.concatenate([s0, s1])
        dist = np.concatenate([eng.coherence_distances_end(pend), d1])
    else:
        samples = draw(count)
        dist = eng.coherence_distances(ii, jj, w.astype(np.float32), samples, c)
    keep = (samples != ii[:, None]) & (samples != jj[:, None])
    avg = _row_means(dist, keep)
    with np.errstate(over="ignore", invalid="ignore"):
        coh = 1.0 / (1.0 + np.exp(avg - merge_threshold))
    coh[~keep.any(axis=1)] = 0.0
    return coh


# ----------------------------------------------------------------------------------------------
# candidate selection in row-major order
# ----------------------------------------------------------------------------------------------
def _best_of(i: np.ndarray, j: np.ndarray, d: np.ndarray) -> Optional[Tuple[int, int, float]]:
    """Smallest (d, i, j) of a candidate list, or None."""
    if len(i) == 0:
        return None
    t = np.lexsort((j, i, d))[0]
    return int(i[t]), int(j[t]), float(d[t])


def select_row_major(eng, c: float, thr: float, k: int, fit: int = ROW_MAJOR_FIT):
    """The first ``k`` candidates ``(i, j, d)`` in row-major order and the best ``(i, j, d)`` of the remaining ones by
    smallest d, then row-major (None when there is no remainder).  No candidates at all: ``([], None)``.

    Built only from ``eng.topk(..., k=0, count=True)`` row-range counts, ``eng.candidates(row_begin, row_end)`` and
    ``eng.argmin(row_begin, ...)``: when the total fits, one listing is sliced; otherwise the smallest ``r`` whose
    rows ``[0, r)`` hold at least ``k`` candidates is found (galloping, then bisection), rows ``[0, r)`` are listed,
    and the remainder's best is the better of that listing's leftover and ``argmin`` over rows ``[r, n)``."""
    k = max(int(k), 0)
    total = eng.topk(c, thr, 0, 0, -1, count=True)[3]
    if total == 0:
        return [], None
    if total <= max(k, fit):
        i, j, d, _ = eng.candidates(c, thr)
        first = list(zip(i[:k].tolist(), j[:k].tolist(), [float(x) for x in d[:k].tolist()]))
        return first, _best_of(i[k:], j[k:], d[k:])
    n = eng.n

    def count_rows(r: int) -> int:
        return eng.topk(c, thr, 0, 0, r, count=True)[3]

    lo, hi = 0, 1                          # count_rows(lo) < k (rows [0, 0) hold nothing)
    while hi < n and count_rows(hi) < k:
        lo, hi = hi, min(2 * hi, n)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if count_rows(mid) >= k:
            hi = mid
        else:
            lo = mid
    i, j, d, _ = eng.candidates(c, thr, 0, hi)
    first = list(zip(i[:k].tolist(), j[:k].tolist(), [float(x) for x in d[:k].tolist()]))
    best = _best_of(i[k:], j[k:], d[k:])
    hit = eng.argmin(c, thr, hi, n) if hi < n else None
    if hit is not None:
        cand = (hit[1], hit[2], float(hit[0]))
        if best is None or (cand[2], cand[0], cand[1]) < (best[2], best[0], best[1]):
            best = cand
    return first, best


# ----------------------------------------------------------------------------------------------
# frequency + coherence
# ----------------------------------------------------------------------------------------------
def write_frequencies(path: str, pair_frequencies: Dict[Tuple[str, str], int]) -> None:
    """``frequencies.json`` in directory ``path``: ``{"left|right": count}``."""
    with open(os.path.join(path, "frequencies.json"), "w") as f:
        json.dump({f"{a}|{b}": v for (a, b), v in pair_frequencies.items()}, f)


def read_frequencies(path: str) -> Dict[tuple, int]:
    """Keys are read back as ``tuple(k.split("|"))``, as the reference does: a token that contains ``|`` gives a key
    that is not a pair.  FileNotFoundError when the directory has no ``frequencies.json``."""
    with open(os.path.join(path, "frequencies.json"), "r") as f:
        return {tuple(k.split("|")): v for k, v in json.load(f).items()}


class FrequencyTerm:
    """Pair frequency and coherence of a candidate, over the tokenizer's ``pair_frequencies`` dict."""

    use_frequency_aware = True
    _freq_top = None               # ((id, len) of the dict, max count); reset to None where counts may have been edited

    def _c(self) -> float:
        return float(self.curvature)

    def _compute_pair_frequencies(self, corpus_path: str) -> None:
        """Adjacent-token pair counts over a corpus file, added to ``pair_frequencies`` (pair_counter.py)."""
        if not self.use_frequency_aware:
            return
        self._logger.info("Computing pair frequencies from corpus...")
        total_pairs = pair_counter.count_pair_frequencies(self, corpus_path, self.pair_frequencies)
        self._freq_top = None
        self._logger.info(f"Computed frequencies for {len(self.pair_frequencies)} unique token pairs "
                          f"from {total_pairs} total pairs")

    def _max_freq(self):
        """``max(values) if dict else 1`` (recomputed per candidate by the reference): once per dict state."""
        pf = self.pair_frequencies
        key = (id(pf), len(pf))
        cached = self._freq_top
        if cached is None or cached[0] != key:
            cached = self._freq_top = (key, max(pf.values()) if pf else 1)
        return cached[1]

    def _frequency_scores(self, ii: np.ndarray, jj: np.ndarray) -> np.ndarray:
        """``np.log1p(freq) / np.log1p(max freq)`` per candidate; 0 when the term is off or ``max freq <= 0`` (an
        empty table scores 0 too: ``log1p(0) / log1p(1)``)."""
        top = self._max_freq() if self.use_frequency_aware else 0
        if not top > 0:
            return np.zeros(len(ii), np.float64)
        pf, vocab = self.pair_frequencies, self.vocab
        counts = np.fromiter((pf.get((vocab[a], vocab[b]), 0) for a, b in zip(ii.tolist(), jj.tolist())),
                             dtype=np.float64, count=len(ii))
        return np.log1p(counts) / np.log1p(top)

    def _coherence_samples(self, count: int) -> np.ndarray:
        """``torch.randperm(n)[:50]`` once per candidate, in candidate order: the torch CPU generator is consumed
        exactly as by the reference.  A tokenizer that keeps ``last_timing`` gets the time in ``rng_ms``."""
        n = self.current_vocab_size
        t0 = now_ms()
        out = randperm_prefixes(n, min(COHERENCE_SAMPLES, n), count)
        timing = getattr(self, "last_timing", None)
        if timing is not None:
            timing["rng_ms"] = timing.get("rng_ms", 0.0) + (now_ms() - t0)
        return out

    def _semantic_coherence_batch(self, ii: np.ndarray, jj: np.ndarray) -> np.ndarray:
        """The reference's ``_compute_semantic_coherence`` for a list of candidates: weight
        ``len(tj) / (len(ti) + len(tj))`` (a Python double there), the float curvature, one RNG draw per candidate
        in list order (``coherence_batch``)."""
        ii = np.ascontiguousarray(ii, np.int32)
        jj = np.ascontiguousarray(jj, np.int32)
        if not self.use_frequency_aware or len(ii) == 0:
            return np.zeros(len(ii), np.float64)
        lens = self._token_lengths()
        li, lj = lens[ii], lens[jj]
        w = (lj / (li + lj)).astype(np.float64)
        return coherence_batch(self._get_engine(), ii, jj, w, self._coherence_samples, self._c(), self.merge_threshold,
                               self.shard)

    def _compute_semantic_coherence(self, i: int, j: int) -> float:
        return float(self._semantic_coherence_batch(np.array([i], np.int32), np.array([j], np.int32))[0])


# ----------------------------------------------------------------------------------------------
# morphology / word sets
# ----------------------------------------------------------------------------------------------
class MorphologyTerm:
    """Corpus statistics and the two string predicates over ``common_morphemes`` / ``common_words``."""

    use_hierarchical = True
    _wordnet = None                # nltk's WordNet corpus reader where a class consults it (the enhanced class, with nltk)
    _sets = None                   # ((id, len) of both sets, frequent substrings of the common words, ...what a class appends)

    def _compute_corpus_statistics(self, corpus_path: str) -> None:
        """Word counts, and the frequent ones of the 2..5-grams and of the words (ngram_counter.py)."""
        if not self.use_hierarchical:
            return
        self._logger.info("Computing corpus statistics for hierarchical merging...")
        word_counter, morphemes, words = corpus_statistics(corpus_path, self.device)
        self.token_frequencies = dict(word_counter)
        self.common_morphemes = morphemes
        self.common_words = words
        self._logger.info(f"Identified {len(self.common_morphemes)} common morphemes and "
                          f"{len(self.common_words)} common words")

    def _string_sets(self):
        """Cached on the identity and size of the two sets."""
        key = (id(self.common_morphemes), len(self.common_morphemes), id(self.common_words), len(self.common_words))
        if self._sets is None or self._sets[0] != key:
            self._sets = (key, frequent_substrings(self.common_words, self.device))
        return self._sets

    def _is_potential_morpheme(self, token: str) -> bool:
        if not self.use_hierarchical or token in self.common_morphemes:
            return True
        wordnet = self._wordnet
        if wordnet is not None:
            if token in PREFIXES or token in SUFFIXES:
                return True
            if len(token) > 2 and any(wordnet.synsets(token, pos=p)
                                      for p in (wordnet.NOUN, wordnet.VERB, wordnet.ADJ, wordnet.ADV)):
                return True
        # len 2..5 and a substring of at least 5 common words: exactly the set of such n-grams of the common words
        return 2 <= len(token) <= 5 and token in self._string_sets()[1]

    def _is_valid_word(self, token: str) -> bool:
        if not self.use_hierarchical or token in self.common_words:
            return True
        if self._wordnet is not None and self._wordnet.synsets(token):
            return True
        return len(token) >= 3 and _VOWEL.search(token) is not None


# ----------------------------------------------------------------------------------------------
# compression
# ----------------------------------------------------------------------------------------------
def greedy_tokens(text: str, vocab: List[str]) -> List[str]:
    """Greedy longest match over ``vocab``, single characters where nothing matches.  The longest matching entry is
    found by length instead of by scanning a sorted copy of the vocabulary at every position: two matching entries
    of the same length are the same string, so the tokens are the reference's.  Empty entries never match (the
    reference's loop does not terminate on one)."""
    entries = set(vocab)
    entries.discard("")
    longest = max((len(t) for t in entries), default=1)
    out, k = [], 0
    while k < len(text):
        piece = text[k]
        for width in range(min(longest, len(text) - k), 1, -1):
            if text[k:k + width] in entries:
                piece = text[k:k + width]
                break
        out.append(piece)
        k += len(piece)
    return out


class CompressionTerm:
    """Greedy token counts of the tokenizer's corpus sample under "vocabulary + one merged token", and the
    ``merge_{i}_{j}_{text[:20]}`` entries of ``tokenize_cache`` that hold them."""

    use_compression_aware = True
    _matcher = None                # make_matcher(device), created at the first count
    _corpus_state = None           # (copy of the texts, key -> representative index, representatives, multiplicities)

    def _tokenize_with_vocab(self, text: str, vocab: List[str]) -> List[str]:
        if not self.use_compression_aware:
            return self.tokenize(text)
        return greedy_tokens(text, vocab)

    def _compression_texts(self) -> List[str]:
        """The texts a candidate is counted on."""
        return self.corpus_sample

    def _corpus(self):
        """Representative lines: the first text of every cache key ``text[:20]`` (a later text with the same key
        reuses the first one's count, as the reference's cache makes it), with the number of texts that share the key."""
        texts = list(self._compression_texts())
        st = self._corpus_state
        if st is None or st[0] != texts:
            index, reps, mult = {}, [], []
            for text in texts:
                r = index.setdefault(text[:20], len(reps))
                if r == len(reps):
                    reps.append(text)
                    mult.append(0)
                mult[r] += 1
            st = self._corpus_state = (texts, index, reps, np.array(mult, np.int64))
            if self._matcher is not None:
                self._matcher.set_corpus(reps, st[3])
        return st

    def _greedy_counts(self, pairs: List[Tuple[int, int]], per_line: bool):
        """Counts of the representative lines under vocabulary + vocab[i] + vocab[j] for every pair: (totals over
        the texts, per-line counts or None)."""
        _, _, reps, mult = self._corpus()
        if self._matcher is None:
            self._matcher = make_matcher(self.device)
            self._matcher.set_corpus(reps, mult)
        self._matcher.sync(self.vocab)
        vocab = self.vocab
        return self._matcher.count([vocab[i] + vocab[j] for i, j in pairs], per_line=per_line)

    def _cached_merge_counts(self, pairs: List[Tuple[int, int]]) -> List[int]:
        """Leaves every ``merge_{i}_{j}_{text[:20]}`` entry of ``pairs`` in ``tokenize_cache`` (pair by pair, keys
        in text order; an entry that is there is kept) from one count call -> the sum over the texts per pair."""
        cache = self.tokenize_cache
        _, index, _, _ = self._corpus()
        _, counts = self._greedy_counts(pairs, per_line=True)
        keys = [text[:20] for text in self._compression_texts()]
        rows = [index[key] for key in keys]
        out = []
        for (i, j), line in zip(pairs, counts.tolist()):
            merged = 0
            for key, r in zip(keys, rows):
                name = f"merge_{i}_{j}_{key}"
                if name not in cache:
                    cache[name] = line[r]
                merged += cache[name]
            out.append(merged)
        return out
