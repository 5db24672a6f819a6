"""Greedy longest-match token counts for compression-aware scoring (``hm_greedy_*``, hm_greedy.hip).

The reference scores a merge candidate ``m = vocab[i] + vocab[j]`` by re-tokenising its corpus sample with
"vocabulary + m" by greedy longest match (``CompressionAwareTokenizer._tokenize_with_vocab``,
compression_aware_tokenizer.py:91-120; the compression term of the enhanced class, enhanced...:813-899): at
position p the longest vocabulary entry that is a prefix of ``text[p:]``, else ``text[p]``.  A matcher holds a
corpus (lines with multiplicities) and the vocabulary, and answers "token count of every line under vocabulary +
{m_c}" for many candidates at once.

* ``GreedyMatcher(device)`` -- the HIP matcher (one per tokenizer); strings cross the C ABI as UTF-32 code points.
* ``HostGreedyMatcher()`` -- the same interface in host Python (the set-of-strings, longest-length-first loop the
  enhanced class uses), for non-HIP devices: the tests' engine doubles run the tokenizer classes through it.

Both treat an empty vocabulary string as never matching (the reference's loop does not terminate on one).  Both
track which prefix ``vocab[:k]`` of the caller's list they hold: when the same list has grown, ``sync`` appends
``vocab[k:]``; any other list is loaded from scratch.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from .._handle import DeviceHandle, code_points


def _code_points(strings: Sequence[str]) -> Tuple[np.ndarray, np.ndarray]:
    """Vocabulary entries, corpus lines and candidates are the caller's Python strings and may hold lone surrogates
    (a vocabulary built by ``chr``, text decoded with ``surrogateescape``): they cross the C ABI as code points."""
    return code_points(strings, "surrogatepass")[:2]


class _VocabTracker:
    """Which prefix of which list the matcher holds."""

    def __init__(self):
        self._list = None
        self._k = 0
        self._last = None

    def delta(self, vocab: List[str]) -> Tuple[bool, List[str]]:
        """-> (rebuild, strings to add)"""
        k = self._k
        same = (vocab is self._list and len(vocab) >= k and (k == 0 or vocab[k - 1] is self._last))
        new = vocab[k:] if same else list(vocab)
        self._list, self._k = vocab, len(vocab)
        self._last = vocab[-1] if vocab else None
        return not same, new


class HostGreedyMatcher:
    """Host restatement of ``GreedyMatcher`` (same results, no device)."""

    def __init__(self):
        self._vt = _VocabTracker()
        self._entries = set()
        self._longest = 0
        self._lines: List[str] = []
        self._mult = np.zeros(0, np.int64)
        self.last_device_ms = 0.0

    def sync(self, vocab: List[str]) -> None:
        rebuild, new = self._vt.delta(vocab)
        if rebuild:
            self._entries, self._longest = set(), 0
        for t in new:
            if t:
                self._entries.add(t)
                self._longest = max(self._longest, len(t))

    def set_corpus(self, lines: Sequence[str], mult: Optional[Sequence[int]] = None) -> None:
        self._lines = list(lines)
        self._mult = np.ones(len(self._lines), np.int64) if mult is None else np.asarray(mult, np.int64)

    def _count(self, text: str, extra: str) -> int:
        """Tokens of ``text`` under vocabulary + {extra}: the longest entry by length, then the extra string."""
        entries, longest = self._entries, self._longest
        n, k, count = len(text), 0, 0
        while k < n:
            step = 1
            for width in range(min(longest, n - k), 1, -1):
                if text[k:k + width] in entries:
                    step = width
                    break
            if len(extra) > step and text.startswith(extra, k):
                step = len(extra)
            k += step
            count += 1
        return count

    def count(self, candidates: Sequence[str], per_line: bool = False):
        """-> (totals int64[K], counts int32[K, lines] or None)"""
        counts = np.array([[self._count(t, m) for t in self._lines] for m in candidates], np.int64).reshape(
            len(candidates), len(self._lines))
        totals = counts @ self._mult if len(self._lines) else np.zeros(len(candidates), np.int64)
        return totals.astype(np.int64), (counts.astype(np.int32) if per_line else None)


class GreedyMatcher(DeviceHandle):
    """The HIP matcher on ``device`` (a HIP device)."""

    PREFIX = "hm_greedy"

    def __init__(self, device: torch.device):
        super().__init__(device)
        self._vt = _VocabTracker()
        self._n_lines = 0
        self._n_cp = 0
        self._corpus = None            # (code points, offsets, mult): re-sent after a vocabulary rebuild
        self.last_device_ms = 0.0

    def sync(self, vocab: List[str]) -> None:
        rebuild, new = self._vt.delta(vocab)
        if rebuild:
            self._recreate()
        if new:
            cps, off = _code_points(new)
            self._check(self._L.hm_greedy_add_strings(self._h, cps.ctypes.data, off.ctypes.data, len(new), self._stream()))

    def _recreate(self) -> None:
        """A fresh matcher (an empty vocabulary) holding the current corpus."""
        self._create()
        if self._corpus is not None:
            cps, off, mult = self._corpus
            self._check(self._L.hm_greedy_set_corpus(self._h, cps.ctypes.data, off.ctypes.data, mult.ctypes.data,
                                                     len(mult), self._stream()))

    def set_corpus(self, lines: Sequence[str], mult: Optional[Sequence[int]] = None) -> None:
        cps, off = _code_points(list(lines))
        mult = np.ones(len(lines), np.int64) if mult is None else np.ascontiguousarray(mult, np.int64)
        self._corpus = (cps, off, mult)
        self._n_lines, self._n_cp = len(mult), int(off[-1])
        self._check(self._L.hm_greedy_set_corpus(self._h, cps.ctypes.data, off.ctypes.data, mult.ctypes.data, len(mult),
                                                 self._stream()))

    def count(self, candidates: Sequence[str], per_line: bool = False):
        """-> (totals int64[K], counts int32[K, lines] or None); ``last_device_ms``: the call's time on the device."""
        k = len(candidates)
        cps, off = _code_points(list(candidates))
        totals = torch.empty(max(k, 1), dtype=torch.int64, device=self.device)
        counts = torch.empty((max(k, 1), max(self._n_lines, 1)), dtype=torch.int32, device=self.device) if per_line else None
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        self._check(self._L.hm_greedy_count(self._h, cps.ctypes.data, off.ctypes.data, k,
                                            C.c_void_p(counts.data_ptr()) if counts is not None else None,
                                            C.c_void_p(totals.data_ptr()), self._stream()))
        stop.record()
        stop.synchronize()
        self.last_device_ms = start.elapsed_time(stop)
        t = totals[:k].cpu().numpy()
        c = counts[:k, :self._n_lines].cpu().numpy() if counts is not None else None
        return t, c

    def longest(self) -> Tuple[np.ndarray, np.ndarray]:
        """(lm per corpus code point, base count per line) as the matcher holds them."""
        lm = torch.empty(max(self._n_cp, 1), dtype=torch.int32, device=self.device)
        base = torch.empty(max(self._n_lines, 1), dtype=torch.int32, device=self.device)
        self._check(self._L.hm_greedy_longest(self._h, C.c_void_p(lm.data_ptr()), C.c_void_p(base.data_ptr()), self._stream()))
        torch.cuda.current_stream(self.device).synchronize()
        return lm[:self._n_cp].cpu().numpy(), base[:self._n_lines].cpu().numpy()


def make_matcher(device: torch.device):
    """The HIP matcher on a HIP device, the host restatement elsewhere."""
    return GreedyMatcher(device) if torch.device(device).type == "cuda" else HostGreedyMatcher()
