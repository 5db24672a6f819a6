"""Riemannian optimisers for Lorentz embedding tables (fused HIP steps, csrc/hm_riemann.hip)."""
from .riemannian import RiemannianAdam, RiemannianSGD  # noqa: F401

__all__ = ["RiemannianSGD", "RiemannianAdam"]
