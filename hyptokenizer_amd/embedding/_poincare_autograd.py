"""Device calls and ``torch.autograd.Function`` wrappers of the Poincare-ball primitives (``hm_rows_*`` /
``hm_rows_*_bwd`` of csrc/hm_poincare.hip).

``poincare_ball`` calls ``forward`` directly when no gradient is recorded and ``apply`` otherwise; both run the same
forward entry point.  Conventions, shared with ``_autograd.py``: the derivative is that of the
reference's torch expression; operands are broadcast like ``engine._broadcast_rows`` and the backward sums over the
broadcast dimensions; non-fp32 operands are computed in fp32 and receive their gradient in their own dtype; ``c`` carries
no gradient; only the inputs are saved; second derivatives are not implemented.
"""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from .. import _lib
from ..engine import _ptr, _require_cuda, _stream_of
from ._autograd import _reduce, _rows

MAX_D = 128

_PAIR = ("mobius_add", "distance")                           # two row operands broadcast against each other


def _shapes(op: str, a: torch.Tensor, b):
    """(shape of the first operand after broadcasting, shape of the second, ball width d)."""
    if op == "mobius_scalar_mul":                             # a = r [..., 1], b = x [..., d]
        if a.dim() == 0:
            a = a.reshape(1)
        if a.shape[-1] != 1:
            raise ValueError(f"mobius_scalar_mul: r must have a trailing dimension of 1 (one factor per row), got {tuple(a.shape)}")
        batch = torch.broadcast_shapes(a.shape[:-1], b.shape[:-1])
        return batch + (1,), batch + (b.shape[-1],), b.shape[-1]
    if op in _PAIR:
        shape = torch.broadcast_shapes(a.shape, b.shape)
        return shape, shape, shape[-1]
    return a.shape, None, a.shape[-1] - (1 if op == "lorentz_to_poincare" else 0)


def _check_width(op: str, d: int) -> None:
    if d < 1 or d > MAX_D:
        raise ValueError(f"poincare_ball.{op}: ball width {d} is outside 1..{MAX_D}")


def forward(op: str, a: torch.Tensor, b, c: float, standard: int = 0) -> torch.Tensor:
    """Result of ``op`` as a fresh fp32 tensor shaped like the reference's (no graph)."""
    L = _lib.load()
    _require_cuda(*((a,) if b is None else (a, b)))
    sa, sb, d = _shapes(op, a, b)
    _check_width(op, d)
    if a.dim() == 0:
        a = a.reshape(1)
    ar = _rows(a, sa)
    br = _rows(b, sb) if b is not None else None
    n = ar.shape[0]
    dev = ar.device
    width = 1 if op == "distance" else d + 1 if op == "poincare_to_lorentz" else d
    lead = sb[:-1] if op == "mobius_scalar_mul" else sa[:-1]
    out = torch.empty((n, width), dtype=torch.float32, device=dev)
    if n > 0:
        s = _stream_of(ar)
        with torch.cuda.device(dev):
            if op == "mobius_add":
                st = L.hm_rows_mobius_add(_ptr(ar), _ptr(br), n, d, d, c, _ptr(out), d, s)
            elif op == "distance":
                st = L.hm_rows_poincare_distance(_ptr(ar), _ptr(br), n, d, d, c, _ptr(out), s)
            elif op == "mobius_scalar_mul":
                st = L.hm_rows_mobius_scalar_mul(_ptr(ar), _ptr(br), n, d, d, c, _ptr(out), d, s)
            elif op == "exp_map_zero":
                st = L.hm_rows_exp_map_zero(_ptr(ar), n, d, d, c, _ptr(out), d, s)
            elif op == "log_map_zero":
                st = L.hm_rows_log_map_zero(_ptr(ar), n, d, d, c, _ptr(out), d, s)
            elif op == "lorentz_to_poincare":
                st = L.hm_rows_lorentz_to_poincare(_ptr(ar), n, d + 1, d, c, _ptr(out), d, s)
            elif op == "poincare_to_lorentz":
                st = L.hm_rows_poincare_to_lorentz(_ptr(ar), n, d, d, c, standard, _ptr(out), d + 1, s)
            else:
                raise ValueError(op)
            _lib.check(st)
    return out.reshape(tuple(lead) + (width,))


class _PoincareOp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, op: str, c: float, standard: int):
        ctx.op, ctx.c, ctx.standard = op, float(c), int(standard)
        ctx.save_for_backward(*((a,) if b is None else (a, b)))
        return forward(op, a, b, float(c), int(standard))

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        op, c = ctx.op, ctx.c
        a = ctx.saved_tensors[0]
        b = ctx.saved_tensors[1] if len(ctx.saved_tensors) > 1 else None
        L = _lib.load()
        sa, sb, d = _shapes(op, a, b)
        ar = _rows(a.reshape(1) if a.dim() == 0 else a, sa)
        br = _rows(b, sb) if b is not None else None
        n = ar.shape[0]
        gr = _rows(g, g.shape)
        ga = torch.empty_like(ar)
        gb = torch.empty_like(br) if br is not None else None
        if n > 0:
            s = _stream_of(ar)
            with torch.cuda.device(ar.device):
                if op == "mobius_add":
                    st = L.hm_rows_mobius_add_bwd(_ptr(ar), _ptr(br), _ptr(gr), d, n, d, d, c, _ptr(ga), _ptr(gb), d, s)
                elif op == "distance":
                    st = L.hm_rows_poincare_distance_bwd(_ptr(ar), _ptr(br), _ptr(gr), n, d, d, c, _ptr(ga), _ptr(gb), d, s)
                elif op == "mobius_scalar_mul":
                    st = L.hm_rows_mobius_scalar_mul_bwd(_ptr(ar), _ptr(br), _ptr(gr), d, n, d, d, c, _ptr(ga), _ptr(gb), d, s)
                elif op == "exp_map_zero":
                    st = L.hm_rows_exp_map_zero_bwd(_ptr(ar), _ptr(gr), d, n, d, d, c, _ptr(ga), d, s)
                elif op == "log_map_zero":
                    st = L.hm_rows_log_map_zero_bwd(_ptr(ar), _ptr(gr), d, n, d, d, c, _ptr(ga), d, s)
                elif op == "lorentz_to_poincare":
                    st = L.hm_rows_lorentz_to_poincare_bwd(_ptr(ar), _ptr(gr), d, n, d + 1, d, c, _ptr(ga), d + 1, s)
                elif op == "poincare_to_lorentz":
                    st = L.hm_rows_poincare_to_lorentz_bwd(_ptr(ar), _ptr(gr), d + 1, n, d, d, c, ctx.standard, _ptr(ga), d, s)
                else:
                    raise ValueError(op)
                _lib.check(st)
        return (_reduce(ga, a, sa) if ctx.needs_input_grad[0] else None,
                _reduce(gb, b, sb) if b is not None and ctx.needs_input_grad[1] else None, None, None, None)


def apply(op: str, a: torch.Tensor, b, c: float, standard: int = 0) -> torch.Tensor:
    return _PoincareOp.apply(a, b, op, c, standard)
