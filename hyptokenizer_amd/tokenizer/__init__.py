"""Tokenizer classes on the merge engine (lazy: importing the package loads no native code)."""

_CLASSES = {
    "HyperbolicTokenizer": "hyperbolic_merge",
    "FastHyperbolicTokenizer": "fast_hyperbolic_merge",
    "EnhancedFastHyperbolicTokenizer": "enhanced_fast_hyperbolic_merge",
    "CompressionAwareTokenizer": "compression_aware_tokenizer",
    "FrequencyAwareHyperbolicTokenizer": "frequency_aware_hyperbolic_merge",
    "HierarchicalHyperbolicTokenizer": "hierarchical_hyperbolic_merge",
}

__all__ = sorted(_CLASSES)


def __getattr__(name):
    mod = _CLASSES.get(name)
    if mod is None:
        raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
    import importlib
    return getattr(importlib.import_module(f"{__name__}.{mod}"), name)
