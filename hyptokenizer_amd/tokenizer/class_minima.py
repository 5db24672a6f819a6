"""Per-class running minima of the pair distance (``hm_classmin_*``, hm_classmin.hip) for the hierarchical tokenizer.

Row code: ``2 * min(len(token), 4) + (1 if the token holds one of "aeiou" else 0)`` -- 10 codes; a pair's class is its
unordered code pair (55 classes, ``class_of``).  A class's minimum is the lexicographic minimum of ``(d, i, j)`` over its
pairs ``i < j`` (NaN distances excluded, no threshold).  Two exception minima are kept beside them: over the pairs whose
merged string ``vocab[i] + vocab[j]`` lies in a string set (list A, list B).

``ClassMinima`` holds the running state over rows ``[0, rows)``: one exact pass (``build``), then one fold per appended
row (that row against all earlier rows, plus its listed partners).  ``DeviceBackend`` runs both on the GPU;
``HostBackend`` restates them from the engine's own distance listing (``row_vs_all``) for engines without the kernels
(the oracle-backed test double).  DESIGN.md section 5.10 gives why the phase selections reduce to these minima.
"""
from __future__ import annotations

import bisect
import ctypes as C
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from .._handle import DeviceHandle

N_CODES, N_CLASSES = 10, 55
Best = Optional[Tuple[float, int, int]]
VOWELS = frozenset("aeiou")


def token_code(tok: str) -> int:
    return 2 * min(len(tok), 4) + (1 if not VOWELS.isdisjoint(tok) else 0)


def class_of(a: int, b: int) -> int:
    lo, hi = (a, b) if a <= b else (b, a)
    return lo * N_CODES - lo * (lo - 1) // 2 + (hi - lo)


def classes_where(pred) -> List[int]:
    """Classes whose code pairs satisfy pred(bucket_a, vowel_a, bucket_b, vowel_b) (length buckets 0..4, 4 = 4 or more)."""
    out = set()
    for a in range(N_CODES):
        for b in range(a, N_CODES):
            if pred(a // 2, a & 1, b // 2, b & 1):
                out.add(class_of(a, b))
    return sorted(out)


# phase 1: both tokens of length <= 2 / <= 3; phase 3: len_i + len_j >= 3 and a vowel in either (the heuristic of
# _is_valid_word, decided by the codes alone -- a bucket of 4 means 4 or more, and then the sum is >= 3 anyway)
P1_LE2 = classes_where(lambda la, va, lb, vb: la <= 2 and lb <= 2)
P1_LE3 = classes_where(lambda la, va, lb, vb: la <= 3 and lb <= 3)
P3_BOOSTED = classes_where(lambda la, va, lb, vb: la + lb >= 3 and (va or vb))
P3_OTHER = sorted(set(range(N_CLASSES)) - set(P3_BOOSTED))


def lexmin(*cands: Best) -> Best:
    best = None
    for c in cands:
        if c is not None and (best is None or c < best):
            best = c
    return best


def _records(out: np.ndarray, count: int) -> List[Best]:
    r = out.reshape(-1, 4)[:count]
    f32 = r[:, 1].astype(np.uint32).view(np.float32)
    return [(float(f32[q]), int(r[q, 2]), int(r[q, 3])) if r[q, 0] else None for q in range(count)]


class DeviceBackend(DeviceHandle):
    """``hm_classmin`` on a ``MergeEngine``."""

    PREFIX = "hm_classmin"

    def __init__(self, eng):
        super().__init__(engine=eng)
        self.eng = eng
        self._out = np.zeros(4 * self._lib.CM_SLOTS, np.uint32)
        self.calls = {"build": 0, "fold": 0}

    def set_codes(self, codes: np.ndarray, row_begin: int) -> None:
        a = np.ascontiguousarray(codes, np.uint8)
        self._check(self._L.hm_classmin_set_codes(self._h, C.c_void_p(a.ctypes.data), int(row_begin),
                                                  int(row_begin) + len(a), self._stream()))

    def build(self, c: float) -> List[Best]:
        self.calls["build"] += 1
        self._check(self._L.hm_classmin_build(self._h, float(c), C.c_void_p(self._out.ctypes.data), self._stream()))
        return _records(self._out, N_CLASSES)

    def fold(self, row: int, c: float, partners: np.ndarray) -> List[Best]:
        """55 class records over the pairs (i, row), then the records of list A and list B."""
        self.calls["fold"] += 1
        p = np.ascontiguousarray(partners, np.int32)
        self._check(self._L.hm_classmin_fold(self._h, int(row), float(c), C.c_void_p(p.ctypes.data) if len(p) else None,
                                             len(p), C.c_void_p(self._out.ctypes.data), self._stream()))
        return _records(self._out, N_CLASSES + 2)


class HostBackend:
    """The same records from the engine's ``row_vs_all`` listing (engines without the class-minimum kernels)."""

    def __init__(self, eng):
        self.eng = eng
        self.codes = np.zeros(0, np.int64)
        self.calls = {"build": 0, "fold": 0}

    def set_codes(self, codes: np.ndarray, row_begin: int) -> None:
        end = row_begin + len(codes)
        if len(self.codes) < end:
            self.codes = np.concatenate([self.codes, np.zeros(end - len(self.codes), np.int64)])
        self.codes[row_begin:end] = np.asarray(codes, np.int64)

    def _row(self, row: int, c: float, partners: Optional[np.ndarray]) -> List[Best]:
        d = np.asarray(self.eng.row_vs_all(row, row, c), np.float32)[:row]
        out: List[Best] = [None] * (N_CLASSES + 2)
        if row > 0:
            cls = np.asarray([class_of(int(self.codes[row]), int(a)) for a in self.codes[:row]], np.int64)
            ok = ~np.isnan(d)
            for q in np.unique(cls[ok]).tolist():
                idx = np.nonzero(ok & (cls == q))[0]
                k = idx[np.argmin(d[idx])]          # argmin returns the first minimum: the smallest i
                out[q] = (float(d[k]), int(k), row)
        if partners is not None:
            for slot, bit in ((N_CLASSES, 1 << 28), (N_CLASSES + 1, 1 << 29)):
                best = None
                for ent in partners.tolist():
                    if ent & bit:
                        i = ent & 0x0FFFFFFF
                        if not np.isnan(d[i]):
                            best = lexmin(best, (float(d[i]), i, row))
                out[slot] = best
        return out

    def build(self, c: float) -> List[Best]:
        self.calls["build"] += 1
        best: List[Best] = [None] * N_CLASSES
        for j in range(1, self.eng.n):
            rec = self._row(j, c, None)
            best = [lexmin(a, b) for a, b in zip(best, rec[:N_CLASSES])]
        return best

    def fold(self, row: int, c: float, partners: np.ndarray) -> List[Best]:
        self.calls["fold"] += 1
        return self._row(row, c, np.asarray(partners, np.int64))


def make_backend(eng):
    from ..engine import MergeEngine
    return DeviceBackend(eng) if isinstance(eng, MergeEngine) else HostBackend(eng)


class SplitIndex:
    """Pairs whose merged string lies in a set: every split ``s = prefix + suffix`` (the empty ones included) of every string
    of the set, indexed by suffix."""

    def __init__(self, strings):
        idx: Dict[str, List[str]] = {}
        for s in strings:
            for k in range(len(s) + 1):
                idx.setdefault(s[k:], []).append(s[:k])
        self.by_suffix = idx

    def partners(self, right: str, rows_of: Dict[str, List[int]], below: int) -> List[int]:
        """Rows i < below with ``vocab[i] + right`` in the set."""
        out: List[int] = []
        for prefix in self.by_suffix.get(right, ()):
            for i in rows_of.get(prefix, ()):
                if i < below:
                    out.append(i)
        return out


class ClassMinima:
    """Running per-class and exception minima over rows ``[0, rows)`` of one engine image."""

    def __init__(self, backend, c: float, vocab: Sequence[str], n: int, index_a: SplitIndex, index_b: SplitIndex):
        self.backend = backend
        self.c = float(c)
        self.index_a, self.index_b = index_a, index_b
        self.rows_of: Dict[str, List[int]] = {}
        codes = np.fromiter((token_code(t) for t in vocab[:n]), np.uint8, n)
        backend.set_codes(codes, 0)
        for r in range(n):
            self.rows_of.setdefault(vocab[r], []).append(r)
        self.cls = backend.build(self.c)
        self.exc = [self._exception_build(index, vocab, n) for index in (index_a, index_b)]
        self.rows = n

    def _exception_build(self, index: SplitIndex, vocab: Sequence[str], n: int) -> Best:
        """Lexmin over every pair i < j < n whose merged string is in the set: listed through the split index (row lists
        are ascending, so each is cut at j by bisection), distances in one gathered launch, the minimum by one lexsort."""
        ii: List[int] = []
        jj: List[int] = []
        rows_of = self.rows_of
        for j in range(n):
            for prefix in index.by_suffix.get(vocab[j], ()):
                rows = rows_of.get(prefix)
                if rows:
                    k = bisect.bisect_left(rows, j)
                    if k:
                        ii.extend(rows[:k])
                        jj.extend([j] * k)
        if not ii:
            return None
        d = np.asarray(self.backend.eng.pair_distance(ii, jj, self.c), np.float32)
        i_a, j_a = np.asarray(ii, np.int64), np.asarray(jj, np.int64)
        ok = np.nonzero(~np.isnan(d))[0]
        if len(ok) == 0:
            return None
        t = ok[np.lexsort((j_a[ok], i_a[ok], d[ok]))[0]]
        return float(d[t]), int(i_a[t]), int(j_a[t])

    def advance(self, vocab: Sequence[str], n: int) -> None:
        """Fold rows [rows, n)."""
        for m in range(self.rows, n):
            tok = vocab[m]
            self.backend.set_codes(np.array([token_code(tok)], np.uint8), m)
            pa = self.index_a.partners(tok, self.rows_of, m)
            pb = self.index_b.partners(tok, self.rows_of, m)
            flags: Dict[int, int] = {}
            for i in pa:
                flags[i] = flags.get(i, 0) | (1 << 28)
            for i in pb:
                flags[i] = flags.get(i, 0) | (1 << 29)
            rec = self.backend.fold(m, self.c, np.fromiter((i | f for i, f in flags.items()), np.int64, len(flags)))
            self.cls = [lexmin(a, b) for a, b in zip(self.cls, rec[:N_CLASSES])]
            self.exc = [lexmin(self.exc[0], rec[N_CLASSES]), lexmin(self.exc[1], rec[N_CLASSES + 1])]
            self.rows_of.setdefault(tok, []).append(m)
            self.rows = m + 1

    def union(self, classes: Sequence[int]) -> Best:
        return lexmin(*(self.cls[q] for q in classes))
