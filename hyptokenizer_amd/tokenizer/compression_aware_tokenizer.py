"""CompressionAwareTokenizer on the MI355X merge engine.

Same class surface as the reference's ``tokenizer/compression_aware_tokenizer.py`` (constructor kwargs and
defaults, ``tokenize_cache`` keys, method names, log lines, ``compression_config.json``).  A step of the reference:

* candidates = the parent's row-major list of pairs ``i < j`` with ``d(i, j) < merge_threshold`` (``:174-176``),
* the first ``sample_size`` of them (row-major, not the nearest) score
  ``compression_weight * original / merged + distance_weight * 1 / (1 + d)`` (``:122-190``): ``merged`` is the
  greedy longest-match token count of the corpus sample under "vocabulary + vocab[i] + vocab[j]", ``original`` the
  count of ``tokenize`` at the first scoring; every other candidate scores ``1 / (1 + d)``,
* the stable sort by ``-score`` picks the first maximum, evaluated candidates before the rest (``:182-188``).

What runs where
* **GPU** -- the candidate search (``MergeEngine``), and the greedy counts of all evaluated candidates over the
  corpus sample in one ``hm_greedy_count`` call (``GreedyMatcher``, hm_greedy.hip); the reference re-tokenises the
  whole sample once per candidate with a scan of the sorted vocabulary at every position.
* **host** -- the scores, as Python floats in the reference's order of operations, and the cache keys.

``optimize_merges`` takes each step's pick from ``_best_scored``, which never builds the full candidate list: the
first ``sample_size`` candidates in row-major order and the best of the rest come from row-range counts and one
``argmin`` (``select_row_major``).  A subclass or an instance that overrides ``_find_merge_candidates`` is honoured:
the loop then calls it, as the reference does.

Additive keyword-only arguments: ``sign_convention``, ``engine`` and ``prefilter`` as in ``HyperbolicTokenizer``;
``shard=`` and ``incremental=True`` are refused (ValueError).

Deviations, documented: an empty-string vocabulary entry never matches (the reference's greedy loop does not
terminate on one); ``load`` returns a working tokenizer (the reference's own ``load`` copies the whole
pre-allocated table into a constructor that expects ``len(vocab)`` rows and raises on its own files).
"""
from __future__ import annotations

import json
import logging
import os
from typing import Dict, List, Optional, Tuple

import torch
from tqdm import tqdm

from .hyperbolic_merge import TQDM_OFF, HyperbolicTokenizer, _loop_without_cyclic_gc
from .scoring import CompressionTerm, now_ms, select_row_major  # noqa: F401  (select_row_major: imported from here by callers)

logger = logging.getLogger(__name__)


class CompressionAwareTokenizer(CompressionTerm, HyperbolicTokenizer):
    """Merges chosen by a mix of compression ratio on a corpus sample and hyperbolic distance."""

    def __init__(
        self,
        vocab: List[str],
        embeddings: torch.nn.Parameter,
        corpus_sample: Optional[List[str]] = None,
        compression_weight: float = 0.7,
        distance_weight: float = 0.3,
        sample_size: int = 100,
        curvature: float = 1.0,
        merge_threshold: float = 0.1,
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
            raise ValueError("CompressionAwareTokenizer: shard= is not supported (the scoring needs the whole candidate list)")
        if incremental:
            raise ValueError("CompressionAwareTokenizer: incremental=True is not supported")
        super().__init__(vocab=vocab, embeddings=embeddings, curvature=curvature, merge_threshold=merge_threshold, lr=lr,
                         device=device, max_vocab_size=max_vocab_size, use_approximate_search=use_approximate_search,
                         sign_convention=sign_convention, engine=engine, prefilter=prefilter)
        self.compression_weight = compression_weight
        self.distance_weight = distance_weight
        self.sample_size = sample_size
        self.corpus_sample = corpus_sample or []
        self.tokenize_cache: Dict[str, int] = {}
        self.last_timing = {}          # ms of the last _best_scored: select / matcher_device / matcher_call / score

    # ------------------------------------------------------------------------------------------
    # compression-aware scoring (reference :122-190; the greedy longest match :91-120 and its counts: CompressionTerm)
    # ------------------------------------------------------------------------------------------
    def _original_tokens(self) -> int:
        """``tokenize_cache["original"]``: computed at the first scoring that has candidates, never refreshed."""
        cache = self.tokenize_cache
        if "original" not in cache:
            if self.device.type == "cuda":
                cache["original"] = sum(len(t) for t in self.tokenize_batch(list(self.corpus_sample)))
            else:
                cache["original"] = sum(len(self.tokenize(text)) for text in self.corpus_sample)
        return cache["original"]

    def _merged_totals(self, pairs: List[Tuple[int, int]], materialise: bool) -> List[int]:
        """``merged_tokens`` of every pair (reference :152-161), cache entries honoured.  ``materialise``: leave every
        ``merge_{i}_{j}_{text[:20]}`` entry in ``tokenize_cache`` as the reference does."""
        if not pairs:
            return []
        if not materialise and not any(key.startswith("merge_") for key in self.tokenize_cache):
            totals, _ = self._greedy_counts(pairs, per_line=False)
            return [int(t) for t in totals.tolist()]
        return self._cached_merge_counts(pairs)

    def _scores(self, evaluated: List[Tuple[int, int, float]], materialise: bool) -> List[float]:
        original = self._original_tokens()
        merged = self._merged_totals([(i, j) for i, j, _ in evaluated], materialise)
        cw, dw = self.compression_weight, self.distance_weight
        out = []
        for (_, _, dist), m in zip(evaluated, merged):
            ratio = 1.0 if m == 0 else original / m
            out.append(cw * ratio + dw * (1.0 / (1.0 + dist)))
        return out

    def _compression_aware_scoring(self, candidates: List[Tuple[int, int, float]]) -> List[float]:
        """Scores of ``candidates`` (higher is better), reference ``:122-190``."""
        if not self.corpus_sample:
            return [1.0 / (1.0 + dist) for _, _, dist in candidates]
        sample_size = min(self.sample_size, len(candidates))
        scores = self._scores(candidates[:sample_size], materialise=True)
        if sample_size < len(candidates):
            scores.extend([1.0 / (1.0 + dist) for _, _, dist in candidates[sample_size:]])
        return scores

    def _find_merge_candidates(self) -> List[Tuple[int, int, float]]:
        """Every candidate as ``(i, j, -score)``, sorted ascending (best first), reference ``:192-218``."""
        candidates = super()._find_merge_candidates()
        if not candidates:
            return []
        scores = self._compression_aware_scoring(candidates)
        scored = [(i, j, -score) for (i, j, _), score in zip(candidates, scores)]
        scored.sort(key=lambda x: x[2])
        return scored

    def _best_scored(self) -> Optional[Tuple[int, int, float]]:
        """``(i, j, score)`` of ``_find_merge_candidates()[0]`` without building the list, or None."""
        eng = self._get_engine()
        thr = self._search_threshold()
        timing = {}
        if not self.corpus_sample:
            hit = eng.argmin(self.curvature, thr)
            self.last_timing = timing
            if hit is None:
                return None
            d, i, j = hit
            return i, j, 1.0 / (1.0 + d)
        t0 = now_ms()
        first, rest = select_row_major(eng, self.curvature, thr, self.sample_size)
        timing["select_ms"] = now_ms() - t0
        if not first and rest is None:
            self.last_timing = timing
            return None
        best = None
        if first:
            t1 = now_ms()
            scores = self._scores(first, materialise=False)
            timing["matcher_call_ms"] = now_ms() - t1
            timing["matcher_device_ms"] = float(getattr(self._matcher, "last_device_ms", 0.0))
            t = max(range(len(scores)), key=scores.__getitem__)       # first maximum: the stable sort's pick
            best = (first[t][0], first[t][1], scores[t])
        if rest is not None:
            score = 1.0 / (1.0 + rest[2])
            if best is None or score > best[2]:
                best = (rest[0], rest[1], score)
        self.last_timing = timing
        return best

    # ------------------------------------------------------------------------------------------
    # merge loop (reference :220-278)
    # ------------------------------------------------------------------------------------------
    def _scored_loop_ok(self) -> bool:
        """``_best_scored`` may stand in for ``_find_merge_candidates()[0]`` unless that method is customised."""
        cls = type(self)
        return (cls._find_merge_candidates is CompressionAwareTokenizer._find_merge_candidates
                and "_find_merge_candidates" not in self.__dict__)

    @_loop_without_cyclic_gc
    def optimize_merges(self, steps: int = 10000, log_every: int = 1000,
                        corpus_sample: Optional[List[str]] = None) -> None:
        """Greedy merge loop with compression-aware scoring (reference ``:220-278``)."""
        if corpus_sample:
            self.corpus_sample = corpus_sample
            self.tokenize_cache = {}
        bar = tqdm(range(steps), desc="Optimizing merges", disable=TQDM_OFF)
        for step in bar:
            if self._scored_loop_ok():
                best = self._best_scored()
            else:
                candidates = self._find_merge_candidates()
                best = (candidates[0][0], candidates[0][1], -candidates[0][2]) if candidates else None
            if best is None:
                logger.info(f"No more merge candidates found after {step} steps")
                break
            i, j, score = best
            self._merge_tokens(i, j)
            for key in [k for k in self.tokenize_cache if k.startswith("merge_")]:
                self.tokenize_cache.pop(key)
            if not bar.disable:
                bar.set_postfix({"vocab_size": self.current_vocab_size, "score": f"{score:.4f}",
                                 "threshold": f"{self.merge_threshold:.4f}"})
            if (step + 1) % log_every == 0:
                logger.info(f"Step {step+1}: merged '{self.vocab[i]}' + '{self.vocab[j]}' -> '{self.vocab[-1]}' "
                            f"(score: {score:.4f})")
            if step > 0 and step % 1000 == 0:
                self.merge_threshold *= 1.1

    # ------------------------------------------------------------------------------------------
    # persistence (reference :280-340)
    # ------------------------------------------------------------------------------------------
    def save(self, path: str) -> None:
        super().save(path)
        config = {"compression_weight": self.compression_weight, "distance_weight": self.distance_weight,
                  "sample_size": self.sample_size}
        with open(os.path.join(path, "compression_config.json"), "w") as f:
            json.dump(config, f)

    @classmethod
    def load(cls, path: str, device: Optional[torch.device] = None, **kwargs) -> "CompressionAwareTokenizer":
        """The four files of ``HyperbolicTokenizer.load`` plus ``compression_config.json`` (defaults, with a warning,
        when it is missing).  ``kwargs`` are the keyword-only extras (``sign_convention``, ``engine``, ...)."""
        compression_config = {}
        try:
            with open(os.path.join(path, "compression_config.json"), "r") as f:
                compression_config = json.load(f)
        except FileNotFoundError:
            logger.warning("Compression config file not found, using defaults")
        tok = super().load(path, device, **kwargs)
        tok.compression_weight = compression_config.get("compression_weight", 0.7)
        tok.distance_weight = compression_config.get("distance_weight", 0.3)
        tok.sample_size = compression_config.get("sample_size", 100)
        return tok

