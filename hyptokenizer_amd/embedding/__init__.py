"""The reference's ``embedding`` package: ``lorentz_model`` and ``poincare_ball``, served by the gfx950 kernels."""
from . import lorentz_model, poincare_ball  # noqa: F401

__all__ = ["lorentz_model", "poincare_ball"]
