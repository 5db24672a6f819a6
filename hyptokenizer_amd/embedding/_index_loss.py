"""A loss on a Lorentz table and an index ``[B, 2 + K]`` (anchor, positive, K negatives), the Python side of
csrc/hm_index_loss.h: the check of the index, the one autograd function over a forward / backward pair of C entry points,
and the reductions.  ``graph_embedding.edge_softmax_loss`` and ``entailment_cones.entailment_cone_loss`` are bindings of it.

A loss names its two entry points, the scalars the C ABI takes between ``k`` and the output pointers, and the trailing
shape of a slot's record in ``weights [B, 1 + K, ...]``, the only workspace the backward kernel reads."""
from __future__ import annotations

from typing import Tuple

import torch
from torch.autograd.function import once_differentiable

from .. import _lib
from ..engine import _ptr, _require_cuda, _stream_of
from ._table import ld


def check_index(who: str, index: torch.Tensor) -> None:
    if index.dtype != torch.int64:
        raise ValueError(f"{who}: index must be int64, got {index.dtype}")
    if index.dim() != 2 or index.shape[1] < 2:
        raise ValueError(f"{who}: index must be [B, 2 + K] (anchor, positive, K negatives), got shape {tuple(index.shape)}")


def forward(fwd: str, x: torch.Tensor, index: torch.Tensor, scalars: tuple, slot: Tuple[int, ...]):
    """(loss [B], weights [B, 1 + K, *slot]) of the detached table ``x``: the forward kernel alone."""
    b, k = index.shape[0], index.shape[1] - 2
    loss = torch.empty(b, dtype=torch.float32, device=x.device)
    weights = torch.empty((b, 1 + k) + tuple(slot), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(getattr(_lib.load(), fwd)(_ptr(x), ld(x), x.shape[0], x.shape[1], _ptr(index), b, k, *scalars, _ptr(loss),
                                             _ptr(weights), _stream_of(x)))
    return loss, weights


class _IndexLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, table, index, fwd: str, bwd: str, scalars: tuple, slot: tuple, sparse_grad: bool):
        loss, weights = forward(fwd, table.detach(), index, scalars, slot)
        ctx.bwd, ctx.scalars, ctx.sparse_grad = bwd, scalars, bool(sparse_grad)
        ctx.save_for_backward(table, index, weights)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        table, index, weights = ctx.saved_tensors
        x = table.detach()
        v, d1 = x.shape
        b, k = index.shape[0], index.shape[1] - 2
        g = g.detach().float().contiguous()
        values = torch.empty((b * (2 + k), d1), dtype=torch.float32, device=x.device)
        coo = torch.empty(b * (2 + k), dtype=torch.int64, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(getattr(_lib.load(), ctx.bwd)(_ptr(x), ld(x), v, d1, _ptr(index), b, k, *ctx.scalars, _ptr(weights), _ptr(g),
                                                     _ptr(values), _ptr(coo), _stream_of(x)))
        grad = torch.sparse_coo_tensor(coo.unsqueeze(0), values, (v, d1), check_invariants=False)
        if not ctx.sparse_grad:
            grad = grad.to_dense()
        return grad, None, None, None, None, None, None


def index_loss(who: str, table: torch.Tensor, index: torch.Tensor, fwd: str, bwd: str, scalars: tuple, slot: tuple, reduction: str,
               sparse_grad: bool, validate: bool) -> torch.Tensor:
    """``[B]`` losses for ``reduction="none"``, their sum, or their sum divided by the number of live samples (``"mean"``;
    0 when there is none); the arguments have passed the caller's checks."""
    _require_cuda(table, index)
    index = index.contiguous()
    v = table.shape[0]
    live = None
    if validate or reduction == "mean":                      # otherwise nothing but the two kernels and a sum is launched
        live = ((index[:, :2] >= 0) & (index[:, :2] < v)).all(dim=1)
    if validate and index.shape[0] > 0 and not bool(live.all()):
        raise ValueError(f"{who}: an anchor or positive lies outside [0, {v})")
    loss = _IndexLoss.apply(table, index, fwd, bwd, scalars, slot, bool(sparse_grad))
    if reduction == "none":
        return loss
    total = loss.sum()
    if reduction == "sum":
        return total
    return total / live.sum().clamp(min=1).to(total.dtype)
