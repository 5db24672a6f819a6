#!/usr/bin/env python
"""Corpus metrics of trained hyperbolic tokenizers: speed, linguistic quality, compression.

Function surface of the hyperbolic side of the reference's ``scripts/compare_tokenizers.py``: ``load_corpus``,
``load_hyperbolic_tokenizer``, ``benchmark_hyperbolic_tokenizer``, ``evaluate_linguistic_quality``,
``evaluate_compression_efficiency`` and a typer ``main`` -- same names, arguments, defaults, result keys and key order,
and the same ``tokenizer_comparison.json`` layout (``{"baseline": {}, "hyperbolic": {type: {...}}}``).

Every metric is a ratio of integer counts of the token stream.  For a hyperbolic tokenizer (``is_hyperbolic=True``, and
always in ``benchmark_hyperbolic_tokenizer``) the counts come from ``tokenizer.corpus_statistics`` -- the batch encoder and
one statistics kernel on the HIP device, no token on the host (tokenizer/corpus_stats.py) -- and the ratios are Python
``int / int`` of them, so they carry the same bits as the reference's.  With ``is_hyperbolic=False`` the reference's loop
over ``tokenizer.encode(text).tokens`` runs on the host, restated once in ``corpus_stats.corpus_statistics_host``.

Pinned as shipped by the reference:

* ``tokenizer_type`` follows its ``isinstance`` order (:163-170), which tests ``HyperbolicTokenizer`` first and therefore
  reports ``"standard"`` for every subclass; the ``"enhanced"`` extras (:198-211) are kept behind it;
* ``benchmark_hyperbolic_tokenizer`` sums tokens over all ``num_runs`` passes and divides by ``len(corpus)`` once
  (:177-190), so ``avg_tokens_per_text`` is ``num_runs`` times the per-text average;
* ``compression_ratio`` is ``chars / (tokens * 2)`` (:324); a corpus without tokens raises ``ZeroDivisionError``.

``avg_tokenization_time`` and ``tokens_per_second`` are wall-clock seconds around the batch call, device synchronised.

Out of scope: the Hugging Face side of the comparison (``load_huggingface_tokenizer``, ``benchmark_huggingface_tokenizer``,
the baseline directory scan), the plots (``generate_visualizations``) and pandas.
"""
from __future__ import annotations

import json
import logging
import os
import time
from typing import Any, Dict, List, Optional

import torch
import typer

from hyptokenizer_amd.tokenizer.corpus_stats import CorpusStatistics, corpus_statistics, corpus_statistics_host
from hyptokenizer_amd.tokenizer.enhanced_fast_hyperbolic_merge import EnhancedFastHyperbolicTokenizer
from hyptokenizer_amd.tokenizer.fast_hyperbolic_merge import FastHyperbolicTokenizer
from hyptokenizer_amd.tokenizer.hyperbolic_merge import HyperbolicTokenizer

logging.basicConfig(level=logging.INFO, format="%(asctime)s - %(name)s - %(levelname)s - %(message)s")
logger = logging.getLogger(__name__)


def load_corpus(corpus_path: str, sample_size: Optional[int] = None) -> List[str]:
    """The stripped non-empty lines of ``corpus_path``, the first ``sample_size`` of them (None: all)."""
    with open(corpus_path, "r", encoding="utf-8") as f:
        lines = [line.strip() for line in f if line.strip()]
    if sample_size is not None:
        lines = lines[:sample_size]
    return lines


def load_hyperbolic_tokenizer(model_path: str, tokenizer_type: str = "fast", device: Optional[torch.device] = None) -> Any:
    """``tokenizer_type``: "standard", "fast" or "enhanced"."""
    if tokenizer_type == "standard":
        return HyperbolicTokenizer.load(model_path, device=device)
    elif tokenizer_type == "fast":
        return FastHyperbolicTokenizer.load(model_path, device=device)
    elif tokenizer_type == "enhanced":
        return EnhancedFastHyperbolicTokenizer.load(model_path, device=device)
    else:
        raise ValueError(f"Unknown tokenizer type: {tokenizer_type}")


def _statistics(tokenizer: Any, corpus: List[str], is_hyperbolic: bool) -> CorpusStatistics:
    if is_hyperbolic:
        return corpus_statistics(tokenizer, corpus)
    return corpus_statistics_host(lambda text: tokenizer.encode(text).tokens, corpus)


def _synchronize(tokenizer: Any) -> None:
    device = getattr(tokenizer, "device", None)
    if isinstance(device, torch.device) and device.type == "cuda":
        torch.cuda.synchronize(device)


def benchmark_hyperbolic_tokenizer(tokenizer: Any, corpus: List[str], num_runs: int = 3) -> Dict[str, Any]:
    if isinstance(tokenizer, HyperbolicTokenizer):
        tokenizer_type = "standard"
    elif isinstance(tokenizer, FastHyperbolicTokenizer):
        tokenizer_type = "fast"
    elif isinstance(tokenizer, EnhancedFastHyperbolicTokenizer):
        tokenizer_type = "enhanced"
    else:
        tokenizer_type = "unknown"

    total_time = 0
    total_tokens = 0
    avg_token_length = 0
    for _ in range(num_runs):
        _synchronize(tokenizer)
        start_time = time.time()
        stats = corpus_statistics(tokenizer, corpus)
        _synchronize(tokenizer)
        total_time += (time.time() - start_time)
        total_tokens += stats.tokens
        avg_token_length += stats.token_chars

    avg_time = total_time / num_runs
    tokens_per_second = total_tokens / avg_time
    avg_tokens_per_text = total_tokens / len(corpus)
    avg_token_length = avg_token_length / total_tokens
    vocab_size = len(tokenizer.vocab)

    additional_metrics = {}
    if tokenizer_type == "enhanced":
        if hasattr(tokenizer, "compression_stats"):
            additional_metrics["compression_ratio"] = tokenizer.compression_stats.get("avg_compression_ratio", None)
        if hasattr(tokenizer, "hierarchy_stats"):
            additional_metrics["hierarchy_preservation"] = tokenizer.hierarchy_stats.get("avg_preservation_score", None)
        if hasattr(tokenizer, "frequency_stats"):
            additional_metrics["frequency_correlation"] = tokenizer.frequency_stats.get("correlation_score", None)
        if hasattr(tokenizer, "curvature_history"):
            additional_metrics["final_curvature"] = tokenizer.curvature
            additional_metrics["curvature_changes"] = len(tokenizer.curvature_history)

    return {
        "tokenizer_type": tokenizer_type,
        "vocab_size": vocab_size,
        "avg_tokenization_time": avg_time,
        "tokens_per_second": tokens_per_second,
        "avg_tokens_per_text": avg_tokens_per_text,
        "avg_token_length": avg_token_length,
        **additional_metrics
    }


def evaluate_linguistic_quality(tokenizer: Any, corpus: List[str], is_hyperbolic: bool = False) -> Dict[str, float]:
    stats = _statistics(tokenizer, corpus, is_hyperbolic)
    return {
        "word_boundary_ratio": stats.word_boundary / stats.tokens,
        "morpheme_ratio": stats.morpheme / stats.tokens,
        "subword_ratio": stats.subword / stats.tokens,
    }


def evaluate_compression_efficiency(tokenizer: Any, corpus: List[str], is_hyperbolic: bool = False) -> Dict[str, float]:
    stats = _statistics(tokenizer, corpus, is_hyperbolic)
    return {
        "chars_per_token": stats.chars / stats.tokens,
        "compression_ratio": stats.chars / (stats.tokens * 2),  # the reference assumes 2 bytes per token id
    }


def compare_tokenizers(corpus_path: str, hyperbolic_dirs: Dict[str, str], output_dir: str, sample_size: int = 1000,
                       num_runs: int = 3, device: Optional[torch.device] = None) -> Dict[str, Any]:
    """The three dictionaries of every tokenizer directory, merged per type, written to
    ``output_dir/tokenizer_comparison.json``.  A tokenizer that fails is logged and left out, as in the reference."""
    logger.info(f"Loading corpus from {corpus_path} (sample size: {sample_size})")
    corpus = load_corpus(corpus_path, sample_size)
    os.makedirs(output_dir, exist_ok=True)
    all_results: Dict[str, Any] = {"baseline": {}, "hyperbolic": {}}
    for tokenizer_type, tokenizer_dir in hyperbolic_dirs.items():
        try:
            tokenizer = load_hyperbolic_tokenizer(tokenizer_dir, tokenizer_type, device=device)
            logger.info(f"Benchmarking {tokenizer_type} hyperbolic tokenizer")
            all_results["hyperbolic"][tokenizer_type] = {
                **benchmark_hyperbolic_tokenizer(tokenizer, corpus, num_runs),
                **evaluate_linguistic_quality(tokenizer, corpus, is_hyperbolic=True),
                **evaluate_compression_efficiency(tokenizer, corpus, is_hyperbolic=True),
            }
        except Exception as e:
            logger.error(f"Error benchmarking {tokenizer_type} hyperbolic tokenizer: {e}")
    results_file = os.path.join(output_dir, "tokenizer_comparison.json")
    with open(results_file, "w") as f:
        json.dump(all_results, f, indent=2)
    logger.info(f"Saved comparison results to {results_file}")
    return all_results


def main(
    corpus_path: str = "data/processed/wiki/wiki.txt",
    standard_hyperbolic_dir: str = "results/hyperbolic/v50000",
    fast_hyperbolic_dir: str = "results/hyperbolic/fast_tokenizer",
    enhanced_hyperbolic_dir: str = "results/hyperbolic/enhanced_tokenizer",
    output_dir: str = "results/tokenizer_comparison",
    sample_size: int = 1000,
    num_runs: int = 3,
    device: Optional[str] = None,
) -> None:
    """Compare the saved hyperbolic tokenizers on a corpus and write their metrics as JSON."""
    compare_tokenizers(
        corpus_path=corpus_path,
        hyperbolic_dirs={"standard": standard_hyperbolic_dir, "fast": fast_hyperbolic_dir, "enhanced": enhanced_hyperbolic_dir},
        output_dir=output_dir,
        sample_size=sample_size,
        num_runs=num_runs,
        device=torch.device(device) if device else None,
    )


if __name__ == "__main__":
    typer.run(main)
