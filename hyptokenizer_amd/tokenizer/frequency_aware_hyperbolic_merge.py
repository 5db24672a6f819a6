"""FrequencyAwareHyperbolicTokenizer on the MI355X merge engine.

Same class surface as the reference's ``tokenizer/frequency_aware_hyperbolic_merge.py`` (constructor kwargs and
defaults, ``pair_frequencies``, method names, log lines, ``frequencies.json`` / ``freq_hyperparams.json``).  A step of
the reference:

* candidates = the parent's row-major list of pairs ``i < j`` with ``d(i, j) < merge_threshold`` (``:210-211``);
* when ``beta > 0`` and no pair frequencies are known, that list unscored: the first row-major candidate is merged
  (``:213-215``); otherwise every candidate that passes ``_is_valid_merge`` scores
  ``alpha / (1 + d) + beta * log1p(freq) / log1p(max freq) + gamma * coherence`` (``:168-199``), the coherence
  drawing one ``torch.randperm(n)[:50]`` per scored candidate, ``gamma == 0`` included (``:114-166``);
* Python's stable sort by ``-score`` (``:232``) picks the first of the list.

What runs where
* **GPU** -- the candidate search (``MergeEngine``); the coherence distances of all scored candidates in one
  ``hm_coherence_batch`` launch (``coherence_batch``, shared with the enhanced class); the corpus pass of
  ``_compute_pair_frequencies``: ``hm_tokenize_batch`` + the adjacent-pair histogram ``hm_pairfreq_add``
  (``pair_counter.py``).
* **host** -- the permutations (torch's CPU generator, in candidate order), the frequency lookups, the scores in
  float64 in the reference's order of operations, and the sort (Python's ``list.sort``: with NaN scores, which the
  reference sign convention produces once merged rows are NaN, its order is the one the reference gets).

Additive keyword-only arguments: ``sign_convention``, ``engine`` and ``prefilter`` as in ``HyperbolicTokenizer``;
``shard=`` and ``incremental=True`` are refused (ValueError).  More candidates than the engine's listing holds raise
(RuntimeError) instead of scoring a truncated list.

Deviation, documented: ``load`` returns a working tokenizer (the reference's own ``load`` builds the class from the
whole pre-allocated table with ``max_vocab_size=100000`` and raises on its own files).
"""
from __future__ import annotations

import json
import logging
import os
import time
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch
from tqdm import tqdm

from .hyperbolic_merge import TQDM_OFF, HyperbolicTokenizer, _loop_without_cyclic_gc
from .scoring import FrequencyTerm, now_ms, read_frequencies, select_row_major, write_frequencies

logger = logging.getLogger(__name__)


class FrequencyAwareHyperbolicTokenizer(FrequencyTerm, HyperbolicTokenizer):
    """Merges chosen by a mix of hyperbolic distance, corpus pair frequency and semantic coherence."""

    _logger = logger

    def __init__(
        self,
        vocab: List[str],
        embeddings: torch.nn.Parameter,
        corpus_path: Optional[str] = None,
        alpha: float = 0.4,
        beta: float = 0.4,
        gamma: float = 0.2,
        curvature: float = 1.0,
        merge_threshold: float = 1.0,
        lr: float = 1e-3,
        device: Optional[torch.device] = None,
        max_vocab_size: int = 100000,
        use_approximate_search: bool = True,
        *,
        sign_convention: str = "reference",
        engine=None,
        shard=None,
        incremental: bool = False,
        prefilter: str = "auto",
    ):
        if shard is not None:
            raise ValueError("FrequencyAwareHyperbolicTokenizer: shard= is not supported (the scoring needs the whole "
                             "candidate list)")
        if incremental:
            raise ValueError("FrequencyAwareHyperbolicTokenizer: incremental=True is not supported")
        super().__init__(vocab=vocab, embeddings=embeddings, curvature=curvature, merge_threshold=merge_threshold, lr=lr,
                         device=device, max_vocab_size=max_vocab_size, use_approximate_search=use_approximate_search,
                         sign_convention=sign_convention, engine=engine, prefilter=prefilter)
        self.alpha = alpha
        self.beta = beta
        self.gamma = gamma
        self.pair_frequencies: Dict[Tuple[str, str], int] = {}
        self.last_timing = {}          # ms of the last scoring: list / rng / coherence / score_sort
        if corpus_path:
            self._compute_pair_frequencies(corpus_path)

    # ------------------------------------------------------------------------------------------
    # scoring (reference :168-199; the corpus pass :92-112, the frequency and coherence terms :114-191: FrequencyTerm)
    # ------------------------------------------------------------------------------------------
    def _scores(self, ii: np.ndarray, jj: np.ndarray, dd: np.ndarray) -> np.ndarray:
        """``alpha * (1 / (1 + d)) + beta * freq + gamma * coherence`` in float64, left to right (reference ``:197``)."""
        freq = self._frequency_scores(ii, jj)
        t0 = now_ms()
        coh = self._semantic_coherence_batch(ii, jj)
        self.last_timing["coherence_ms"] = self.last_timing.get("coherence_ms", 0.0) + (now_ms() - t0)
        dist_score = 1.0 / (1.0 + np.asarray(dd, np.float64))
        with np.errstate(invalid="ignore", over="ignore"):
            return self.alpha * dist_score + self.beta * freq + self.gamma * coh

    def _score_merge_candidate(self, i: int, j: int, dist: float) -> float:
        return float(self._scores(np.array([i], np.int32), np.array([j], np.int32), np.array([dist]))[0])

    # ------------------------------------------------------------------------------------------
    # candidates (reference :201-234)
    # ------------------------------------------------------------------------------------------
    def _distance_candidates(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """The parent's candidate list as arrays (row-major); raises when the listing cannot hold all of them."""
        eng = self._get_engine()
        i, j, d, total = eng.candidates(self.curvature, self._search_threshold())
        if total > len(i):
            raise RuntimeError(f"FrequencyAwareHyperbolicTokenizer: {total} merge candidates, more than the engine lists "
                               f"({len(i)}); every candidate is scored, so a truncated list cannot be used -- lower "
                               f"merge_threshold")
        return i, j, d

    def _valid_mask(self, ii: np.ndarray, jj: np.ndarray) -> Optional[np.ndarray]:
        """``_is_valid_merge`` of every candidate when a subclass or an instance overrides it; None: all valid."""
        if type(self)._is_valid_merge is HyperbolicTokenizer._is_valid_merge and "_is_valid_merge" not in self.__dict__:
            return None
        vocab = self.vocab
        return np.fromiter((bool(self._is_valid_merge(vocab[a], vocab[b])) for a, b in zip(ii.tolist(), jj.tolist())),
                           bool, len(ii))

    def _find_merge_candidates(self) -> List[Tuple[int, int, float]]:
        """Unscored ``(i, j, d)`` (no frequencies, ``beta > 0``) or scored ``(i, j, -score)`` sorted ascending."""
        self.last_timing = {}
        t0 = now_ms()
        i, j, d = self._distance_candidates()
        self.last_timing["list_ms"] = now_ms() - t0
        if len(i) == 0:
            return []
        if self.beta > 0 and not self.pair_frequencies:
            return [(a, b, float(x)) for a, b, x in zip(i.tolist(), j.tolist(), d.tolist())]
        keep = self._valid_mask(i, j)
        if keep is not None:
            i, j, d = i[keep], j[keep], d[keep]
        dd = [float(x) for x in d.tolist()]
        scores = self._scores(i, j, np.asarray(dd, np.float64))
        t1 = now_ms()
        scored = [(a, b, -s) for a, b, s in zip(i.tolist(), j.tolist(), scores.tolist())]
        scored.sort(key=lambda x: x[2])
        self.last_timing["score_sort_ms"] = now_ms() - t1
        return scored

    def _step_pick(self) -> Tuple[int, Optional[Tuple[int, int, float]]]:
        """(``len(_find_merge_candidates())``, its first entry or None); the unscored case lists one candidate only."""
        if self.beta > 0 and not self.pair_frequencies:
            eng = self._get_engine()
            thr = self._search_threshold()
            total = eng.topk(self.curvature, thr, 0, 0, -1, count=True)[3]
            if total == 0:
                return 0, None
            first, _ = select_row_major(eng, self.curvature, thr, 1)
            return total, first[0]
        candidates = self._find_merge_candidates()
        return len(candidates), (candidates[0] if candidates else None)

    def _scored_loop_ok(self) -> bool:
        cls = type(self)
        return (cls._find_merge_candidates is FrequencyAwareHyperbolicTokenizer._find_merge_candidates
                and "_find_merge_candidates" not in self.__dict__)

    # ------------------------------------------------------------------------------------------
    # merge loop (reference :236-313)
    # ------------------------------------------------------------------------------------------
    @_loop_without_cyclic_gc
    def optimize_merges(self, steps: int = 10000, log_every: int = 1000, parallel_eval: bool = True,
                        sample_ratio: float = 1.0, corpus_path: Optional[str] = None) -> None:
        """Greedy merge loop with frequency-aware scoring (reference ``:236-313``).  ``parallel_eval`` and
        ``sample_ratio`` are accepted and unused, as there."""
        if corpus_path:
            self._compute_pair_frequencies(corpus_path)
        self._freq_top = None            # counts may have been edited since the last call
        bar = tqdm(range(steps), desc="Optimizing merges", disable=TQDM_OFF)
        no_candidate_count = 0
        for step in bar:
            start_time = time.time()
            if self._scored_loop_ok():
                count, best = self._step_pick()
            else:
                candidates = self._find_merge_candidates()
                count, best = len(candidates), (candidates[0] if candidates else None)
            if step % log_every == 0:
                logger.info(f"Step {step}: vocab_size={self.current_vocab_size}")
                logger.info(f"  Merge candidates: {count}")
                logger.info(f"  Merge threshold: {self.merge_threshold:.6f}")
            if best is None:
                no_candidate_count += 1
                if no_candidate_count > 5:
                    self.merge_threshold *= 1.5
                    logger.info(f"No candidates found. Increasing threshold to {self.merge_threshold:.6f}")
                    no_candidate_count = 0
                # (the reference's "> 10" branch sits behind "> 5" and never runs)
                continue
            no_candidate_count = 0
            i, j, score = best
            t0 = now_ms()
            self._merge_tokens(i, j)
            self.last_timing["merge_ms"] = now_ms() - t0
            if not bar.disable:
                bar.set_postfix({"vocab_size": self.current_vocab_size, "score": f"{-score:.4f}",
                                 "threshold": f"{self.merge_threshold:.4f}",
                                 "time": f"{time.time() - start_time:.2f}s"})
            if (step + 1) % log_every == 0:
                logger.info(f"Step {step+1}: merged '{self.vocab[i]}' + '{self.vocab[j]}' -> '{self.vocab[-1]}' "
                            f"(score: {-score:.4f})")
            if step > 0 and step % 1000 == 0:
                self.merge_threshold *= 1.1

    # ------------------------------------------------------------------------------------------
    # persistence (reference :315-396)
    # ------------------------------------------------------------------------------------------
    def save(self, path: str) -> None:
        super().save(path)
        write_frequencies(path, self.pair_frequencies)
        with open(os.path.join(path, "freq_hyperparams.json"), "w") as f:
            json.dump({"alpha": self.alpha, "beta": self.beta, "gamma": self.gamma}, f)

    @classmethod
    def load(cls, path: str, device: Optional[torch.device] = None, **kwargs) -> "FrequencyAwareHyperbolicTokenizer":
        """The four files of ``HyperbolicTokenizer.load`` plus ``freq_hyperparams.json`` and ``frequencies.json``
        (each optional, with the reference's warnings).  Keys are read back as ``tuple(k.split("|"))``, as the
        reference does: a token that contains ``|`` gives a key that is not a pair.  Unlike the reference's ``load``
        (which raises on its own files), this returns a working tokenizer.  ``kwargs`` are the keyword-only extras."""
        tok = super().load(path, device, **kwargs)
        try:
            with open(os.path.join(path, "freq_hyperparams.json"), "r") as f:
                hyperparams = json.load(f)
            tok.alpha = hyperparams.get("alpha", 0.4)
            tok.beta = hyperparams.get("beta", 0.4)
            tok.gamma = hyperparams.get("gamma", 0.2)
        except FileNotFoundError:
            logger.warning("Hyperparameters file not found, using defaults")
        try:
            tok.pair_frequencies = read_frequencies(path)
        except FileNotFoundError:
            logger.warning("Frequencies file not found")
        return tok
