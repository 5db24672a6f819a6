"""Poincare-ball primitives with the reference's function surface, served by the gfx950 kernels.

Mirrors ``embedding/poincare_ball.py`` of the reference: the same eight names, positional arguments, defaults and result
shapes (``norm`` and ``distance`` keep a trailing dimension of 1).  ``mobius_addition``, ``mobius_scalar_mul``,
``exp_map_zero``, ``log_map_zero``, ``distance``, ``lorentz_to_poincare`` and ``poincare_to_lorentz`` run as one fused HIP
kernel each through the C ABI (``hm_rows_*`` of csrc/hm_poincare.hip: a row is read once and written once) and need
tensors on a HIP device; on a CPU tensor they raise ``HypMergeUnavailable`` (there is no CPU fallback).  The last dimension
is at most 128 (129 on the Lorentz side of the conversions).  ``norm`` is the one torch call the reference has.

Curvature: ``c`` is a Python float or a one-element tensor whose value is taken without gradient; ``c <= 0`` or a
non-finite ``c`` raises ``ValueError``.  A float works in all eight functions.  That is a superset of the reference:
its ``mobius_scalar_mul``, ``exp_map_zero`` and ``log_map_zero`` call ``torch.sqrt(c)`` and raise ``TypeError`` for a
Python float -- the default ``c=1.0`` included -- so they only run there when ``c`` is a tensor.

Conversions: the reference's ``poincare_to_lorentz`` does not land on the hyperboloid -- its image has
``x0^2 - |x_s|^2 = 1/(4c)`` and ``lorentz_to_poincare`` does not invert it.  ``conversion="reference"`` (the default)
reproduces it as shipped; ``conversion="standard"`` is ``x0 = (1 + c|p|^2) / (sqrt(c) (1 - c|p|^2))``,
``x_s = 2p / (1 - c|p|^2)``, which satisfies ``x0^2 - |x_s|^2 = 1/c`` and at ``c = 1`` is the exact inverse of
``lorentz_to_poincare``.  For ``c != 1`` the reference's conversions, ``project_to_hyperboloid`` and Lorentz ``distance``
follow mutually inconsistent conventions; nothing here tries to reconcile them.

Autograd: when gradients are being recorded and an operand requires grad, the functions run as the
``torch.autograd.Function`` of ``_poincare_autograd.py`` (same forward kernels, HIP backward kernels that recompute the row
scalars from the inputs).  The derivative is that of the reference's torch expression: the ``clamp(min=1e-8)`` masks, the
``(norm == 0)`` mask arithmetic of the two zero-maps, torch's zero subgradient of the norm at the zero vector, ``atanh`` at
and beyond 1.  ``r`` of ``mobius_scalar_mul`` is a tensor operand and gets a gradient; ``c`` gets none; second derivatives
raise ``RuntimeError``.  Non-fp32 operands are computed in fp32 and receive their gradient in their own dtype.
"""
from __future__ import annotations

import math

import torch

from . import _poincare_autograd as _pa
from ._autograd import wants_grad

_CONVERSIONS = {"reference": 0, "standard": 1}


def _curv(c) -> float:
    if isinstance(c, torch.Tensor):
        if c.numel() != 1:
            raise ValueError(f"c must be a Python float or a one-element tensor, got a tensor of shape {tuple(c.shape)}")
        c = c.detach().item()
    c = float(c)
    if not (math.isfinite(c) and c > 0.0):
        raise ValueError(f"curvature c must be finite and > 0, got {c!r}")
    return c


def _run(op: str, a: torch.Tensor, b, c, standard: int = 0) -> torch.Tensor:
    c = _curv(c)
    if wants_grad(a, b):
        return _pa.apply(op, a, b, c, standard)
    return _pa.forward(op, a, b, c, standard)


def norm(x: torch.Tensor) -> torch.Tensor:
    """Reference ``poincare_ball.py:14-24``: the Euclidean norm, trailing dimension kept."""
    return torch.norm(x, dim=-1, keepdim=True)


def mobius_addition(x: torch.Tensor, y: torch.Tensor, c: float = 1.0) -> torch.Tensor:
    """Reference ``:27-46``: ``((1 + 2c<x,y> + c|y|^2) x + (1 - c|x|^2) y) / (1 + 2c<x,y> + c^2 |x|^2 |y|^2)``."""
    return _run("mobius_add", x, y, c)


def mobius_scalar_mul(r: torch.Tensor, x: torch.Tensor, c: float = 1.0) -> torch.Tensor:
    """Reference ``:49-65``: ``tanh(r atanh(sqrt(c) n)) / (sqrt(c) n) x`` with ``n = clamp(|x|, 1e-8)``; ``r`` is ``(..., 1)``."""
    return _run("mobius_scalar_mul", r, x, c)


def exp_map_zero(v: torch.Tensor, c: float = 1.0) -> torch.Tensor:
    """Reference ``:68-84``: ``tanh(sqrt(c) n) / (sqrt(c) n) v``, the zero vector mapped to itself."""
    return _run("exp_map_zero", v, None, c)


def log_map_zero(x: torch.Tensor, c: float = 1.0) -> torch.Tensor:
    """Reference ``:87-103``: ``atanh(sqrt(c) n) / (sqrt(c) n) x``, the zero vector mapped to itself."""
    return _run("log_map_zero", x, None, c)


def distance(x: torch.Tensor, y: torch.Tensor, c: float = 1.0) -> torch.Tensor:
    """Reference ``:106-126``: ``2 / sqrt(c) atanh(sqrt(c) |(-x) (+) y|)``, shape ``(..., 1)``."""
    return _run("distance", x, y, c)


def lorentz_to_poincare(x: torch.Tensor, c: float = 1.0) -> torch.Tensor:
    """Reference ``:129-140``: ``x[..., 1:] / (x[..., 0:1] + 1 / sqrt(c))``."""
    return _run("lorentz_to_poincare", x, None, c)


def poincare_to_lorentz(x: torch.Tensor, c: float = 1.0, *, conversion: str = "reference") -> torch.Tensor:
    """Reference ``:143-163`` as shipped (``conversion="reference"``) or the standard map (``"standard"``, module docstring)."""
    try:
        standard = _CONVERSIONS[conversion]
    except KeyError:
        raise ValueError(f"conversion must be 'reference' or 'standard', got {conversion!r}") from None
    return _run("poincare_to_lorentz", x, None, c, standard)
