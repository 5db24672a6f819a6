"""``torch.autograd.Function`` wrappers of the Lorentz primitives: forward through the existing C entry points
(``engine.device_rows_op`` / ``device_batch_distance``, unchanged), backward through the ``hm_*_bwd`` kernels.

``lorentz_model`` dispatches here only when autograd is recording and an operand requires grad; every other call
takes the code path it always took.  Conventions: the derivative is that of the reference's torch
expression (clamp masks, ``acosh'`` infinite at 1, the mask arithmetic of ``log_map`` / ``exp_map``); operands are
broadcast like ``engine._broadcast_rows`` and the backward sums over the broadcast dimensions; non-fp32 operands are
computed in fp32 and receive their gradient in their own dtype; ``c`` is a Python float without gradient; second
derivatives are not implemented.
"""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from .. import _lib
from ..engine import _f, _ptr, _require_cuda, _stream_of, device_batch_distance, device_rows_op


def wants_grad(*tensors) -> bool:
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


def _rows(t: torch.Tensor, shape) -> torch.Tensor:
    """``t`` broadcast to ``shape`` as contiguous fp32 rows [b, shape[-1]].  No copy when it already is that; a broadcast,
    strided or non-fp32 operand is materialised as a full [b, shape[-1]] fp32 copy (in the forward and again in the backward)."""
    return t.detach().expand(shape).reshape(-1, shape[-1]).contiguous().float()


def _reduce(g: torch.Tensor, like: torch.Tensor, shape) -> torch.Tensor:
    """Gradient of the broadcast operand back to ``like``'s shape and dtype."""
    return g.reshape(shape).sum_to_size(like.shape).to(like.dtype)


class _PairOp(torch.autograd.Function):
    """minkowski_dot / distance / log_map / exp_map on two broadcast operands."""

    @staticmethod
    def forward(ctx, x, y, op: str, c: float, sign_mode: int):
        _require_cuda(x, y)
        ctx.op, ctx.c, ctx.sign_mode = op, float(c), int(sign_mode)
        ctx.save_for_backward(x, y)
        return device_rows_op(op, x, y, float(c), int(sign_mode))

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, y = ctx.saved_tensors
        L = _lib.load()
        shape = torch.broadcast_shapes(x.shape, y.shape)
        xb, yb = _rows(x, shape), _rows(y, shape)
        b, d1 = xb.shape
        gx, gy = torch.empty_like(xb), torch.empty_like(yb)
        s = _stream_of(xb)
        with torch.cuda.device(xb.device):
            if ctx.op in ("minkowski", "distance"):
                gb = g.detach().expand(shape[:-1]).reshape(-1).contiguous().float()
                if ctx.op == "minkowski":
                    _lib.check(L.hm_rows_minkowski_bwd(_ptr(xb), _ptr(yb), _ptr(gb), b, d1, d1, ctx.sign_mode, _ptr(gx), _ptr(gy), d1, s))
                else:
                    _lib.check(L.hm_rows_distance_bwd(_ptr(xb), _ptr(yb), _ptr(gb), b, d1, d1, _f(ctx.c), ctx.sign_mode,
                                                      _ptr(gx), _ptr(gy), d1, s))
            else:
                gb = _rows(g, shape)
                if ctx.op == "log_map":
                    _lib.check(L.hm_rows_log_map_bwd(_ptr(xb), _ptr(yb), _ptr(gb), d1, b, d1, d1, ctx.sign_mode, _ptr(gx), _ptr(gy), d1, s))
                elif ctx.op == "exp_map":
                    _lib.check(L.hm_rows_exp_map_bwd(_ptr(xb), _ptr(yb), _ptr(gb), d1, b, d1, d1, _ptr(gx), _ptr(gy), d1, s))
                else:
                    raise ValueError(ctx.op)
        return (_reduce(gx, x, shape) if ctx.needs_input_grad[0] else None,
                _reduce(gy, y, shape) if ctx.needs_input_grad[1] else None, None, None, None)


class _Project(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, c: float):
        _require_cuda(x)
        ctx.c = float(c)
        ctx.save_for_backward(x)
        return device_rows_op("project", x, None, float(c), 0)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        L = _lib.load()
        xb, gb = _rows(x, x.shape), _rows(g, x.shape)
        b, d1 = xb.shape
        gx = torch.empty_like(xb)
        with torch.cuda.device(xb.device):
            _lib.check(L.hm_rows_project_bwd(_ptr(xb), _ptr(gb), d1, b, d1, d1, _f(ctx.c), _ptr(gx), d1, _stream_of(xb)))
        return gx.reshape(x.shape).to(x.dtype), None


class _BatchDistance(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, c: float, sign_mode: int):
        _require_cuda(x, y)
        ctx.c, ctx.sign_mode = float(c), int(sign_mode)
        ctx.save_for_backward(x, y)
        return device_batch_distance(x, y, float(c), int(sign_mode))

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, y = ctx.saved_tensors
        L = _lib.load()
        xb, yb = _rows(x, x.shape), _rows(y, y.shape)
        (n1, d1), n2 = xb.shape, yb.shape[0]
        gb = g.detach().expand(n1, n2).contiguous().float()
        gx = torch.zeros_like(xb) if ctx.needs_input_grad[0] else None
        gy = torch.zeros_like(yb) if ctx.needs_input_grad[1] else None
        with torch.cuda.device(xb.device):
            _lib.check(L.hm_batch_distance_bwd(_ptr(xb), n1, _ptr(yb), n2, d1, d1, d1, _f(ctx.c), ctx.sign_mode, _ptr(gb), n2,
                                               _ptr(gx) if gx is not None else None, _ptr(gy) if gy is not None else None, d1,
                                               _stream_of(xb)))
        return (gx.reshape(x.shape).to(x.dtype) if gx is not None else None,
                gy.reshape(y.shape).to(y.dtype) if gy is not None else None, None, None)


def pair_op(op: str, x: torch.Tensor, y: torch.Tensor, c: float, sign_mode: int) -> torch.Tensor:
    return _PairOp.apply(x, y, op, c, sign_mode)


def project(x: torch.Tensor, c: float) -> torch.Tensor:
    return _Project.apply(x, c)


def batch_distance(x: torch.Tensor, y: torch.Tensor, c: float, sign_mode: int) -> torch.Tensor:
    return _BatchDistance.apply(x, y, c, sign_mode)
