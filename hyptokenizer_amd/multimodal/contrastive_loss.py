"""Hyperbolic InfoNCE and triplet loss with the reference's names and arguments
(``multimodal/contrastive_loss.py``), as fused HIP kernels with HIP backward passes.

``hyperbolic_contrastive_loss`` never builds the B x B similarity matrix: the forward pass keeps the two
log-sum-exp vectors (rows and columns of ``-distance / temp``), the backward pass recomputes the tiles from them.
Saved for backward: the two inputs and those two vectors, O(B * d1 + B) memory.  ``c = 1`` as in the reference.
The ``sign_convention=`` keyword and its default are those of ``embedding.lorentz_model``: under ``"reference"`` every
distance is 0, the loss is ``log B`` and every gradient is exactly 0; ``"lorentz"`` is the
sign-corrected geometry.  ``MultimodalHyperbolicModel`` (a two-tower wrapper around external encoders) is not rebuilt.
There is no CPU fallback: tensors must live on a HIP device.
"""
from __future__ import annotations

from typing import Optional

import torch
from torch.autograd.function import once_differentiable

from .. import _lib
from ..embedding import lorentz_model as _lm
from ..engine import _f, _ptr, _require_cuda, _stream_of

MAX_BATCH = 65536
MAX_D1 = 129
_REDUCTIONS = ("mean", "sum", "none")


def _rows(t: torch.Tensor) -> torch.Tensor:
    return t.detach().reshape(-1, t.shape[-1]).contiguous().float()


class _InfoNCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z_text, z_img, temp: float, reduction: str, sign_mode: int):
        _require_cuda(z_text, z_img)
        L = _lib.load()
        zt, zi = _rows(z_text), _rows(z_img)
        n, d1 = zt.shape
        buf = torch.empty((4, n), dtype=torch.float32, device=zt.device)        # lse_row, lse_col, diag, losses
        total = torch.empty((), dtype=torch.float32, device=zt.device)
        with torch.cuda.device(zt.device):
            _lib.check(L.hm_infonce_fwd(_ptr(zt), _ptr(zi), n, d1, d1, d1, _f(temp), int(sign_mode), _ptr(buf[0]), _ptr(buf[1]),
                                        _ptr(buf[2]), _ptr(buf[3]), _ptr(total), _stream_of(zt)))
        ctx.temp, ctx.reduction, ctx.sign_mode = float(temp), reduction, int(sign_mode)
        ctx.save_for_backward(z_text, z_img, buf[0].clone(), buf[1].clone())
        if reduction == "none":
            return buf[3].clone()
        return total / n if reduction == "mean" else total

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        z_text, z_img, lse_row, lse_col = ctx.saved_tensors
        L = _lib.load()
        zt, zi = _rows(z_text), _rows(z_img)
        n, d1 = zt.shape
        g = g.detach().float()
        if ctx.reduction == "none":
            w = g.reshape(n).contiguous()
        else:
            w = (g / n if ctx.reduction == "mean" else g).reshape(1).expand(n).contiguous()
        gt = torch.empty_like(zt) if ctx.needs_input_grad[0] else None
        gi = torch.empty_like(zi) if ctx.needs_input_grad[1] else None
        with torch.cuda.device(zt.device):
            _lib.check(L.hm_infonce_bwd(_ptr(zt), _ptr(zi), n, d1, d1, d1, _f(ctx.temp), ctx.sign_mode, _ptr(lse_row), _ptr(lse_col),
                                        _ptr(w), _ptr(gt) if gt is not None else None, _ptr(gi) if gi is not None else None, d1,
                                        _stream_of(zt)))
        return (gt.reshape(z_text.shape).to(z_text.dtype) if gt is not None else None,
                gi.reshape(z_img.shape).to(z_img.dtype) if gi is not None else None, None, None, None)


class _Triplet(torch.autograd.Function):
    """Per-sample losses; the reduction is a plain torch op on top."""

    @staticmethod
    def forward(ctx, anchor, positive, negative, margin: float, sign_mode: int):
        _require_cuda(anchor, positive, negative)
        L = _lib.load()
        a, p, n = _rows(anchor), _rows(positive), _rows(negative)
        b, d1 = a.shape
        losses = torch.empty(b, dtype=torch.float32, device=a.device)
        with torch.cuda.device(a.device):
            _lib.check(L.hm_triplet_fwd_bwd(_ptr(a), _ptr(p), _ptr(n), b, d1, d1, _f(margin), int(sign_mode), None, _ptr(losses),
                                            None, None, None, d1, _stream_of(a)))
        ctx.margin, ctx.sign_mode = float(margin), int(sign_mode)
        ctx.save_for_backward(anchor, positive, negative)
        return losses.reshape(anchor.shape[:-1])

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        anchor, positive, negative = ctx.saved_tensors
        L = _lib.load()
        a, p, n = _rows(anchor), _rows(positive), _rows(negative)
        b, d1 = a.shape
        w = g.detach().float().expand(anchor.shape[:-1]).reshape(b).contiguous()
        ga, gp, gn = torch.empty_like(a), torch.empty_like(p), torch.empty_like(n)
        with torch.cuda.device(a.device):
            _lib.check(L.hm_triplet_fwd_bwd(_ptr(a), _ptr(p), _ptr(n), b, d1, d1, _f(ctx.margin), ctx.sign_mode, _ptr(w), None,
                                            _ptr(ga), _ptr(gp), _ptr(gn), d1, _stream_of(a)))
        outs = [t.reshape(src.shape).to(src.dtype) if need else None
                for t, src, need in zip((ga, gp, gn), (anchor, positive, negative), ctx.needs_input_grad[:3])]
        return outs[0], outs[1], outs[2], None, None


def _check_pair(a: torch.Tensor, b: torch.Tensor, what: str) -> None:
    if a.dim() != 2 or a.shape != b.shape:
        raise ValueError(f"{what}: expected two tensors of the same shape (batch_size, d+1), got {tuple(a.shape)} and {tuple(b.shape)}")
    if not 2 <= a.shape[1] <= MAX_D1:
        raise ValueError(f"{what}: d+1 must lie in [2, {MAX_D1}], got {a.shape[1]}")


def hyperbolic_contrastive_loss(z_text: torch.Tensor, z_img: torch.Tensor, temp: float = 0.07, reduction: str = "mean", *,
                                sign_convention: Optional[str] = None) -> torch.Tensor:
    """Reference ``contrastive_loss.py:17-61``: symmetric cross-entropy over ``-distance(z_text[i], z_img[j]) / temp``."""
    if reduction not in _REDUCTIONS:
        raise ValueError(f"reduction must be one of {_REDUCTIONS}, got {reduction!r}")
    _check_pair(z_text, z_img, "hyperbolic_contrastive_loss")
    if not 1 <= z_text.shape[0] <= MAX_BATCH:
        raise ValueError(f"hyperbolic_contrastive_loss: batch size must lie in [1, {MAX_BATCH}], got {z_text.shape[0]}")
    if not temp > 0:
        raise ValueError("hyperbolic_contrastive_loss: temp must be positive")
    return _InfoNCE.apply(z_text, z_img, float(temp), reduction, _lm._sign(sign_convention))


def hyperbolic_triplet_loss(anchor: torch.Tensor, positive: torch.Tensor, negative: torch.Tensor, margin: float = 1.0,
                            reduction: str = "mean", *, sign_convention: Optional[str] = None) -> torch.Tensor:
    """Reference ``contrastive_loss.py:64-97``: ``relu(d(anchor, positive) - d(anchor, negative) + margin)``."""
    if reduction not in _REDUCTIONS:
        raise ValueError(f"reduction must be one of {_REDUCTIONS}, got {reduction!r}")
    _check_pair(anchor, positive, "hyperbolic_triplet_loss")
    _check_pair(anchor, negative, "hyperbolic_triplet_loss")
    losses = _Triplet.apply(anchor, positive, negative, float(margin), _lm._sign(sign_convention))
    if reduction == "mean":
        return losses.mean()
    if reduction == "sum":
        return losses.sum()
    return losses


class HyperbolicInfoNCE(torch.nn.Module):
    """Reference ``contrastive_loss.py:100-131``."""

    def __init__(self, temperature: float = 0.07, *, sign_convention: Optional[str] = None):
        super().__init__()
        self.temperature = temperature
        self.sign_convention = sign_convention

    def forward(self, z1: torch.Tensor, z2: torch.Tensor) -> torch.Tensor:
        return hyperbolic_contrastive_loss(z1, z2, temp=self.temperature, sign_convention=self.sign_convention)
