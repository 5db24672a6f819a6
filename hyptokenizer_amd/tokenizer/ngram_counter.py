"""Character n-gram counts of a word list (``hm_ngram_*``, hm_ngram.hip) and the corpus statistics of the hierarchical
tokenizer.

The reference's statistics pass (hierarchical_hyperbolic_merge.py:110-156)::

    for line in f:
        words = re.findall(r'\\b\\w+\\b', line.lower())
        word_counter.update(words)
        for word in words:
            for n in range(2, min(6, len(word) + 1)):
                for i in range(len(word) - n + 1): subword_counter[word[i:i+n]] += 1

``corpus_statistics`` keeps the Unicode-exact parts on the host at C speed (the file iterator, ``str.lower``, the regex,
the word ``Counter``) and counts the n-grams of the DISTINCT words, each weighted by its multiplicity -- the same totals
as the per-occurrence loop.  On a HIP device the counter is ``hm_ngram_count``; ``ngram_counts_host`` restates it for other
devices.  The same counter in its distinct mode gives, for every n-gram, the number of distinct words that contain it
(the ``>= 5`` rule of ``_is_potential_morpheme``, :193-198).
"""
from __future__ import annotations

import ctypes as C
import re
from collections import Counter
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from tqdm import tqdm

# strict encoding: the words come out of a file read as strict UTF-8 (count_words), so they hold no lone surrogate; a
# caller's own word list that does is refused with UnicodeEncodeError, as before
from .._handle import DeviceHandle, code_points as words_to_code_points

WORD_RE = re.compile(r"\b\w+\b")


class NgramCounter(DeviceHandle):
    """One ``hm_ngram`` counter on a HIP device."""

    PREFIX = "hm_ngram"

    def __init__(self, device: torch.device, initial_capacity: int = 0):
        super().__init__(device, int(initial_capacity))
        self.recounts = 0

    def count(self, cps: np.ndarray, offsets: np.ndarray, weights: Optional[np.ndarray], distinct: bool = False):
        """-> (pos int64, len int32, count int64) of every distinct n-gram (n = 2..5) of the words, in no particular order."""
        cps = np.ascontiguousarray(cps, np.int32)
        offsets = np.ascontiguousarray(offsets, np.int64)
        n_words = len(offsets) - 1
        w = None if distinct else np.ascontiguousarray(weights, np.int64)
        nd = C.c_int64(0)
        stream = self._stream()
        self._check(self._L.hm_ngram_count(self._h, C.c_void_p(cps.ctypes.data), C.c_void_p(offsets.ctypes.data),
                                           None if w is None else C.c_void_p(w.ctypes.data), n_words,
                                           self._lib.NGRAM_DISTINCT if distinct else self._lib.NGRAM_WEIGHTED,
                                           C.byref(nd), stream))
        m = int(nd.value)
        pos = np.empty(m, np.int64)
        ln = np.empty(m, np.int32)
        cnt = np.empty(m, np.int64)
        rc = C.c_int64(0)
        if m:
            self._check(self._L.hm_ngram_read(self._h, C.c_void_p(pos.ctypes.data), C.c_void_p(ln.ctypes.data),
                                              C.c_void_p(cnt.ctypes.data), m, C.byref(rc), stream))
        else:
            self._check(self._L.hm_ngram_read(self._h, None, None, None, 0, C.byref(rc), stream))
        self.recounts = int(rc.value)
        return pos, ln, cnt


def ngram_counts_host(words: Sequence[str], weights: Optional[Sequence[int]], distinct: bool = False) -> Dict[str, int]:
    """Host restatement: ``{n-gram: sum of weights}`` or ``{n-gram: number of words containing it}``."""
    out: Dict[str, int] = {}
    for k, word in enumerate(words):
        grams = [word[i:i + n] for n in range(2, min(6, len(word) + 1)) for i in range(len(word) - n + 1)]
        if distinct:
            for g in set(grams):
                out[g] = out.get(g, 0) + 1
        else:
            wt = int(weights[k])
            for g in grams:
                out[g] = out.get(g, 0) + wt
    return out


def ngram_counts(words: Sequence[str], weights: Optional[Sequence[int]], device: torch.device, distinct: bool = False,
                 counter: Optional[NgramCounter] = None) -> Tuple[List[str], np.ndarray]:
    """(n-grams, counts int64) in no particular order; the HIP counter on a cuda device, the host loop otherwise."""
    if torch.device(device).type != "cuda":
        d = ngram_counts_host(words, weights, distinct)
        return list(d.keys()), np.fromiter(d.values(), np.int64, len(d))
    cps, offsets, flat = words_to_code_points(words)
    cnt_dev = counter if counter is not None else NgramCounter(device)
    pos, ln, cnt = cnt_dev.count(cps, offsets, None if distinct else np.asarray(weights, np.int64), distinct)
    return [flat[p:p + n] for p, n in zip(pos.tolist(), ln.tolist())], cnt


def select_at_least(words: Sequence[str], weights: Optional[Sequence[int]], device: torch.device, distinct: bool,
                    floor=None, percentile: Optional[float] = None):
    """n-grams whose count is ``>= floor`` (or ``>= np.percentile(counts, percentile)``) -> (set, all counts).  Strings are
    built only for the n-grams that pass.  With no n-gram at all, the percentile raises as the reference's does."""
    if torch.device(device).type != "cuda":
        d = ngram_counts_host(words, weights, distinct)
        counts = list(d.values())
        thr = np.percentile(counts, percentile) if percentile is not None else floor
        return {g for g, c in d.items() if c >= thr}, np.asarray(counts, np.int64)
    cps, offsets, flat = words_to_code_points(words)
    pos, ln, cnt = NgramCounter(device).count(cps, offsets, None if distinct else np.asarray(weights, np.int64), distinct)
    if percentile is not None:
        thr = np.percentile(cnt, percentile) if len(cnt) else np.percentile([], percentile)
    else:
        thr = floor
    keep = np.nonzero(cnt >= thr)[0]
    return {flat[p:p + n] for p, n in zip(pos[keep].tolist(), ln[keep].tolist())}, cnt


def count_words(corpus_path: str) -> Counter:
    """The reference's word loop: ``re.findall(r'\\b\\w+\\b', line.lower())`` per line of the text-mode file."""
    word_counter: Counter = Counter()
    with open(corpus_path, "r", encoding="utf-8") as f:
        for line in tqdm(f, desc="Analyzing corpus", disable=True):
            word_counter.update(WORD_RE.findall(line.lower()))
    return word_counter


def corpus_statistics(corpus_path: str, device: torch.device):
    """-> (word Counter, common_morphemes, common_words) as hierarchical_hyperbolic_merge.py:110-156 computes them."""
    word_counter = count_words(corpus_path)
    words = list(word_counter.keys())
    weights = np.fromiter(word_counter.values(), np.int64, len(words))
    common_morphemes, _ = select_at_least(words, weights, device, distinct=False, percentile=80)
    word_threshold = np.percentile(list(word_counter.values()), 70)
    common_words = {word for word, count in word_counter.items() if count >= word_threshold}
    return word_counter, common_morphemes, common_words


def frequent_substrings(common_words: Iterable[str], device: torch.device, floor: int = 5) -> set:
    """The 2..5-character strings that are substrings of at least ``floor`` distinct words of ``common_words``."""
    words = sorted(common_words)
    if not words:
        return set()
    out, _ = select_at_least(words, None, device, distinct=True, floor=floor)
    return out
