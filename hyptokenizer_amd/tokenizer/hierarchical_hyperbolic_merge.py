"""HierarchicalHyperbolicTokenizer on the MI355X merge engine.

Same class surface as the reference's ``tokenizer/hierarchical_hyperbolic_merge.py`` in the branch it takes without
nltk (``NLTK_AVAILABLE = False``; nltk is never imported here): constructor kwargs and defaults, ``language``,
``token_frequencies``, ``common_morphemes``, ``common_words``, the predicates and filters, the three-phase
``optimize_merges`` with its log lines, ``hierarchical_data.json``.

What runs where
* **GPU** -- the corpus statistics' n-gram histogram (``hm_ngram_count``: the distinct words weighted by their counts, and
  the distinct mode for the ``>= 5 common words`` rule), and the step selection: per-class running minima of the pair
  distance (``hm_classmin_build`` once per loop state, ``hm_classmin_fold`` per merge), DESIGN.md section 5.10.  No step
  builds the candidate list.
* **host** -- reading the file, ``str.lower``, the word regex and ``Counter`` (C-speed Python), the percentiles
  (``np.percentile``), the split index of the two string sets that lists the exception partners of each new row, and the
  phase logic.

A step of phase p picks what ``min`` over the reference's filtered candidate list picks (the first minimum in row-major
order): phase 1 the nearest pair of the classes "both tokens <= 2 characters" (relaxed to <= 3 while fewer than 500
merges), phase 2 ``lexmin{(d_A, A), (d_E * 0.8, E)}`` (A: the nearest pair; E: the nearest pair whose merged string is a
potential morpheme), phase 3 ``lexmin{(d_B * 0.7, B), (d_U, U)}`` (B: the nearest pair of the heuristic "valid word"
classes or whose merged string is a common word; U: the nearest of the other classes).  Candidates are the minima with
``d < _search_threshold()``.

The class-minimum path is used when none of ``_find_merge_candidates``, ``_is_potential_morpheme``, ``_is_valid_word``,
``_filter_morphologically_valid``, ``_filter_word_valid`` is overridden (by a subclass or an instance); otherwise each
step runs the reference's list code over ``_find_merge_candidates()``.  Engines without the kernels (the oracle-backed
test double) get a host restatement of both counters from their own distance listing.

Additive keyword-only arguments: ``sign_convention``, ``engine`` and ``prefilter`` as in ``HyperbolicTokenizer``;
``shard=`` and ``incremental=True`` are refused (ValueError).  More candidates than the engine's listing holds raise
(RuntimeError) in the list path.

Deviations, documented: ``hierarchical_data.json`` holds its two lists sorted (the reference writes set iteration order,
which depends on the interpreter's hash seed); ``load`` returns a working tokenizer built from the saved live rows and
``max_vocab_size`` (the reference's ``load`` rebuilds the class from the whole pre-allocated table with the default size).
"""
from __future__ import annotations

import json
import logging
import os
from typing import Dict, List, Optional, Set, Tuple

import torch
from tqdm import tqdm

from .class_minima import (N_CLASSES, P1_LE2, P1_LE3, P3_BOOSTED, P3_OTHER, ClassMinima, SplitIndex, lexmin,
                           make_backend)
from .hyperbolic_merge import TQDM_OFF, HyperbolicTokenizer, _loop_without_cyclic_gc
from .scoring import MorphologyTerm

logger = logging.getLogger(__name__)

NLTK_AVAILABLE = False             # the reference's branch without nltk is the one reproduced (MorphologyTerm._wordnet stays None)
_LIST_METHODS = ("_find_merge_candidates", "_is_potential_morpheme", "_is_valid_word", "_filter_morphologically_valid",
                 "_filter_word_valid")


class HierarchicalHyperbolicTokenizer(MorphologyTerm, HyperbolicTokenizer):
    """Hyperbolic tokenizer whose merges run in three phases: characters, subwords (morphemes), words."""

    #: iterations of the three phases (the reference's ``range(2000)``, ``range(5000)``, ``range(10000)``)
    PHASE_STEPS = (2000, 5000, 10000)
    _logger = logger

    def __init__(
        self,
        vocab: List[str],
        embeddings: torch.nn.Parameter,
        corpus_path: Optional[str] = None,
        curvature: float = 1.0,
        merge_threshold: float = 0.05,
        lr: float = 1e-3,
        device: Optional[torch.device] = None,
        max_vocab_size: int = 100000,
        use_approximate_search: bool = True,
        language: str = "english",
        *,
        sign_convention: str = "reference",
        engine=None,
        shard=None,
        incremental: bool = False,
        prefilter: str = "auto",
    ):
        if shard is not None:
            raise ValueError("HierarchicalHyperbolicTokenizer: shard= is not supported")
        if incremental:
            raise ValueError("HierarchicalHyperbolicTokenizer: incremental=True is not supported (the class minima are "
                             "maintained incrementally already)")
        super().__init__(vocab=vocab, embeddings=embeddings, curvature=curvature, merge_threshold=merge_threshold, lr=lr,
                         device=device, max_vocab_size=max_vocab_size, use_approximate_search=use_approximate_search,
                         sign_convention=sign_convention, engine=engine, prefilter=prefilter)
        self.language = language
        self.token_frequencies: Dict[str, int] = {}
        self.common_morphemes: Set[str] = set()
        self.common_words: Set[str] = set()
        self._cm = None                # (key, ClassMinima)
        self._cm_backend = None        # (engine, backend)
        if corpus_path:
            self._compute_corpus_statistics(corpus_path)

    # ------------------------------------------------------------------------------------------
    # string sets (the corpus statistics :110-156 and the predicates :158-204, NLTK absent: MorphologyTerm)
    # ------------------------------------------------------------------------------------------
    def _string_sets(self):
        """(key, frequent substrings, split index A, split index B): the split indexes list the exception partners
        of each new row (class_minima.py)."""
        sets = super()._string_sets()
        if len(sets) == 2:                 # rebuilt for other sets: the split indexes join the cached tuple
            sets = self._sets = sets + (SplitIndex(set(self.common_morphemes) | sets[1]), SplitIndex(self.common_words))
        return sets

    # ------------------------------------------------------------------------------------------
    # filters (reference :206-277)
    # ------------------------------------------------------------------------------------------
    def _filter_morphologically_valid(self, candidates: List[Tuple[int, int, float]]) -> List[Tuple[int, int, float]]:
        out = []
        for i, j, dist in candidates:
            if self._is_potential_morpheme(self.vocab[i] + self.vocab[j]):
                out.append((i, j, dist * 0.8))
            else:
                out.append((i, j, dist))
        return out

    def _filter_word_valid(self, candidates: List[Tuple[int, int, float]]) -> List[Tuple[int, int, float]]:
        out = []
        for i, j, dist in candidates:
            if self._is_valid_word(self.vocab[i] + self.vocab[j]):
                out.append((i, j, dist * 0.7))
            else:
                out.append((i, j, dist))
        return out

    def _find_merge_candidates(self) -> List[Tuple[int, int, float]]:
        eng = self._get_engine()
        i, j, d, total = eng.candidates(self.curvature, self._search_threshold())
        if total > len(i):
            raise RuntimeError(f"HierarchicalHyperbolicTokenizer: {total} merge candidates, more than the engine lists "
                               f"({len(i)}); lower merge_threshold")
        return [(int(a), int(b), float(x)) for a, b, x in zip(i.tolist(), j.tolist(), d.tolist())]

    # ------------------------------------------------------------------------------------------
    # step selection
    # ------------------------------------------------------------------------------------------
    def _class_min_ok(self) -> bool:
        cls = type(self)
        return all(getattr(cls, m) is getattr(HierarchicalHyperbolicTokenizer, m) and m not in self.__dict__
                   for m in _LIST_METHODS)

    def refresh_engine(self) -> None:
        super().refresh_engine()
        self._cm = None

    def _class_minima(self) -> ClassMinima:
        eng = self._get_engine()
        if self._cm_backend is None or self._cm_backend[0] is not eng:
            self._cm_backend = (eng, make_backend(eng))
            self._cm = None
        sets = self._string_sets()
        n = self.current_vocab_size
        key = (self.embeddings.data_ptr(), self.embeddings._version, float(self.curvature), id(self.vocab), sets[0])
        st = self._cm
        if st is None or st[0] != key or st[1].rows > n:
            st = (key, ClassMinima(self._cm_backend[1], float(self.curvature), self.vocab, n, sets[2], sets[3]))
            self._cm = st
        else:
            st[1].advance(self.vocab, n)
        return st[1]

    def _phase_pick(self, phase: int, count: int):
        """(any candidate at all, the (i, j, key) the phase merges or None)."""
        if not self._class_min_ok():
            return self._phase_pick_list(phase, count)
        st = self._class_minima()
        thr = self._search_threshold()

        def cand(b):
            return b if b is not None and b[0] < thr else None

        first = cand(st.union(range(N_CLASSES)))
        if first is None:
            return False, None
        if phase == 1:
            best = cand(st.union(P1_LE2))
            if best is None and count < 500:
                best = cand(st.union(P1_LE3))
            return True, None if best is None else (best[1], best[2], best[0])
        if phase == 2:
            e = cand(st.exc[0])
            best = lexmin(first, None if e is None else (e[0] * 0.8, e[1], e[2]))
        else:
            b = cand(lexmin(st.union(P3_BOOSTED), st.exc[1]))
            best = lexmin(None if b is None else (b[0] * 0.7, b[1], b[2]), cand(st.union(P3_OTHER)))
        return True, (best[1], best[2], best[0])

    def _phase_pick_list(self, phase: int, count: int):
        """The reference's list code (:295-400) over ``_find_merge_candidates()``."""
        candidates = self._find_merge_candidates()
        if not candidates:
            return False, None
        if phase == 1:
            pool = [c for c in candidates if len(self.vocab[c[0]]) <= 2 and len(self.vocab[c[1]]) <= 2]
            if not pool and count < 500:
                pool = [c for c in candidates if len(self.vocab[c[0]]) <= 3 and len(self.vocab[c[1]]) <= 3]
        elif phase == 2:
            pool = self._filter_morphologically_valid(candidates)
        else:
            pool = self._filter_word_valid(candidates) or candidates
        return True, (min(pool, key=lambda x: x[2]) if pool else None)

    # ------------------------------------------------------------------------------------------
    # the three phases (reference :279-428)
    # ------------------------------------------------------------------------------------------
    def _hierarchical_merge_strategy(self, target_vocab_size: Optional[int] = None) -> None:
        logger.info(f"Starting hierarchical merge with vocabulary size: {self.current_vocab_size}")
        phases = (
            (1, 0.05, "Phase 1: Character-level merges (building basic subwords)", "Phase 1: Character merges", 500),
            (2, 0.1, "Phase 2: Subword-level merges (building morphemes)", "Phase 2: Subword merges", 2000),
            (3, 0.2, "Phase 3: Word-level merges (building words and compounds)", "Phase 3: Word merges", 5000),
        )
        for (phase, thr0, title, desc, floor), steps in zip(phases, self.PHASE_STEPS):
            self.merge_threshold = thr0
            logger.info(title)
            bar = tqdm(range(steps), desc=desc, disable=TQDM_OFF)
            count = 0
            for step in bar:
                any_cand, best = self._phase_pick(phase, count)
                if not any_cand:
                    if count < floor and (phase != 3 or self.merge_threshold < 1.0):
                        self.merge_threshold *= 1.2
                        logger.info(f"Increasing threshold to {self.merge_threshold:.4f}")
                        continue
                    break
                if best is None:
                    break
                i, j = best[0], best[1]
                self._merge_tokens(i, j)
                count += 1
                if step % 100 == 0:
                    logger.info(f"Merged '{self.vocab[i]}' + '{self.vocab[j]}' → '{self.vocab[-1]}'")
                if target_vocab_size and self.current_vocab_size >= target_vocab_size:
                    logger.info(f"Reached target vocabulary size {target_vocab_size}")
                    return
                if not bar.disable:
                    bar.set_postfix({"vocab_size": self.current_vocab_size, f"phase{phase}_merges": count})
            logger.info(f"Completed Phase {phase} with {count} merges. Vocabulary size: {self.current_vocab_size}")
        logger.info(f"Final vocabulary size: {self.current_vocab_size}")

    @_loop_without_cyclic_gc
    def optimize_merges(self, steps: int = 10000, log_every: int = 1000, hierarchical: bool = True,
                        target_vocab_size: Optional[int] = None) -> None:
        """The three phases, or ``HyperbolicTokenizer.optimize_merges(steps, log_every)`` when ``hierarchical`` is False."""
        if hierarchical:
            self._hierarchical_merge_strategy(target_vocab_size)
        else:
            super().optimize_merges(steps, log_every)

    # ------------------------------------------------------------------------------------------
    # persistence (reference :430-498)
    # ------------------------------------------------------------------------------------------
    def save(self, path: str) -> None:
        super().save(path)
        data = {
            "language": self.language,
            "common_morphemes": sorted(self.common_morphemes),
            "common_words": sorted(self.common_words),
        }
        with open(os.path.join(path, "hierarchical_data.json"), "w") as f:
            json.dump(data, f)

    @classmethod
    def load(cls, path: str, device: Optional[torch.device] = None, **kwargs) -> "HierarchicalHyperbolicTokenizer":
        """The four files of ``HyperbolicTokenizer.load`` plus ``hierarchical_data.json`` (optional, with the reference's
        warning).  ``kwargs`` are the keyword-only extras."""
        tok = super().load(path, device, **kwargs)
        try:
            with open(os.path.join(path, "hierarchical_data.json"), "r") as f:
                data = json.load(f)
            tok.language = data.get("language", "english")
            tok.common_morphemes = set(data.get("common_morphemes", []))
            tok.common_words = set(data.get("common_words", []))
        except FileNotFoundError:
            logger.warning("Hierarchical data file not found")
        return tok
