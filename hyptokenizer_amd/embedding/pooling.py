"""Lorentz-centroid pooling: one point of the hyperboloid per bag of token rows, as one fused HIP kernel pair with a sparse
backward (Law, Liao, Snell, Zemel: "Lorentzian distance learning for hyperbolic representations", ICML 2019).

``lorentz_centroid(table, ids, offsets, lengths=None, weights=None)`` -- ``table`` is fp32 ``[V, d + 1]`` on a HIP device, rows
on the unit hyperboloid of ``sign_convention="lorentz"`` (``x0^2 - |x_s|^2 = 1``; curvature does not enter); ``ids`` int64
``[T]``; ``offsets`` int64 ``[n + 1]``, non-decreasing inside ``[0, T]``; ``lengths`` int32 ``[n]`` with
``0 <= lengths[i] <= offsets[i + 1] - offsets[i]``; ``weights`` fp32 ``[T]``, non-negative by contract.  Segment ``i`` is
``ids[offsets[i] : offsets[i] + len_i]`` with ``len_i = lengths[i]``, or the whole span without ``lengths``: the slab
``BatchEncoder.run`` produces (tokens at the front of a line's span, slack behind) is consumed as it is.  A token is live when
it lies inside its segment's length and its id lies in ``[0, V)``; every other position (slack, ``-1`` padding) is skipped and
never dereferenced.  With ``s_i = sum_t w_t x_{ids[t]}`` over the live tokens and ``q_i = s_i0^2 - |s_is|^2``

    ``mu_i = s_i / sqrt(q_i)``

Where a segment has no live token, or ``q_i`` is not positive and finite (zero weights, NaN rows), the result is the origin
``(1, 0, .., 0)`` and the segment's gradient is exactly zero.

The gradient on ``table`` is the Euclidean one ``optim.RiemannianSGD`` / ``RiemannianAdam`` consume, by default an uncoalesced
sparse COO tensor ``[V, d + 1]`` with exactly ``T`` entries: entry ``t`` has index ``ids[t]`` and value ``w_t h_i``,
``h_i = (g_i + (g_i . mu_i) J mu_i) / sqrt(q_i)``, ``J = diag(-1, 1, .., 1)``; a skipped position has index 0 and a zero row.
``weights`` receive ``h_i . x_{ids[t]}`` when they require grad.  No atomics: two calls on the same inputs return the same
bits.  There is no CPU fallback: off a HIP device the functions raise ``HypMergeUnavailable``.
"""
from __future__ import annotations

from typing import Optional

import torch
from torch.autograd.function import once_differentiable

from .. import _lib
from ..engine import _ptr, _require_cuda, _stream_of
from ._table import MAX_WIDTH, MIN_WIDTH, check_table, ld as _ld
from .graph_embedding import init_table


def _check_args(table, ids, offsets, lengths, weights, sign_convention: str) -> None:
    if sign_convention != "lorentz":
        raise ValueError(f"lorentz_centroid: sign_convention must be 'lorentz', got {sign_convention!r} (the centroid is "
                         "defined on the hyperboloid x0^2 - |x_s|^2 = 1 only)")
    check_table("lorentz_centroid", table)
    if ids.dtype != torch.int64 or ids.dim() != 1:
        raise ValueError(f"lorentz_centroid: ids must be int64 [T], got {ids.dtype} {tuple(ids.shape)}")
    if offsets.dtype != torch.int64 or offsets.dim() != 1 or offsets.numel() < 1:
        raise ValueError(f"lorentz_centroid: offsets must be int64 [n + 1], got {offsets.dtype} {tuple(offsets.shape)}")
    n = offsets.numel() - 1
    if lengths is not None and (lengths.dtype != torch.int32 or lengths.shape != (n,)):
        raise ValueError(f"lorentz_centroid: lengths must be int32 [{n}], got {lengths.dtype} {tuple(lengths.shape)}")
    if weights is not None and (weights.dtype != torch.float32 or weights.shape != ids.shape):
        raise ValueError(f"lorentz_centroid: weights must be float32 {tuple(ids.shape)}, got {weights.dtype} {tuple(weights.shape)}")


def _validate_segments(offsets: torch.Tensor, lengths: Optional[torch.Tensor], t: int) -> None:
    """The one synchronising read of ``validate=True``."""
    n = offsets.numel() - 1
    span = offsets[1:] - offsets[:-1]
    bad_o = (span < 0).any() | (offsets[0] < 0) | (offsets[n] > t)
    bad_l = ((lengths < 0) | (lengths > span)).any() if lengths is not None else torch.zeros_like(bad_o)
    bad = torch.stack([bad_o, bad_l])
    bad_offsets, bad_lengths = bad.tolist()
    if bad_offsets:
        raise ValueError(f"lorentz_centroid: offsets must be non-decreasing with offsets[0] >= 0 and offsets[n] <= {t}")
    if bad_lengths:
        raise ValueError("lorentz_centroid: lengths must satisfy 0 <= lengths[i] <= offsets[i + 1] - offsets[i]")


class _Centroid(torch.autograd.Function):
    @staticmethod
    def forward(ctx, table, ids, offsets, lengths, weights, sparse_grad: bool):
        L = _lib.load()
        x = table.detach()
        w = None if weights is None else weights.detach()
        n, d1 = offsets.numel() - 1, x.shape[1]
        mu = torch.empty((n, d1), dtype=torch.float32, device=x.device)
        inv_nu = torch.empty(n, dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(L.hm_centroid_fwd(_ptr(x), _ld(x), x.shape[0], d1, _ptr(ids), ids.numel(), _ptr(offsets), _ptr(lengths), _ptr(w), n,
                                         _ptr(mu), _ptr(inv_nu), _stream_of(x)))
        ctx.sparse_grad, ctx.has_lengths, ctx.has_weights = bool(sparse_grad), lengths is not None, weights is not None
        ctx.save_for_backward(table, ids, offsets, mu, inv_nu, *(t for t in (lengths, weights) if t is not None))
        return mu

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        table, ids, offsets, mu, inv_nu, *rest = ctx.saved_tensors
        lengths = rest.pop(0) if ctx.has_lengths else None
        weights = rest.pop(0) if ctx.has_weights else None
        L = _lib.load()
        x = table.detach()
        v, d1 = x.shape
        n, t = offsets.numel() - 1, ids.numel()
        g = g.detach().float().contiguous()
        want_w = ctx.has_weights and ctx.needs_input_grad[4]
        grad_table = grad_w = None
        if ctx.needs_input_grad[0] or want_w:
            values = torch.empty((t, d1), dtype=torch.float32, device=x.device)
            coo = torch.empty(t, dtype=torch.int64, device=x.device)
            grad_w = torch.empty(t, dtype=torch.float32, device=x.device) if want_w else None
            with torch.cuda.device(x.device):
                _lib.check(L.hm_centroid_bwd(_ptr(x), _ld(x), v, d1, _ptr(ids), t, _ptr(offsets), _ptr(lengths),
                                             _ptr(None if weights is None else weights.detach()), n, _ptr(mu), _ptr(inv_nu), _ptr(g),
                                             _ptr(values), _ptr(coo), _ptr(grad_w), _stream_of(x)))
            if ctx.needs_input_grad[0]:
                grad_table = torch.sparse_coo_tensor(coo.unsqueeze(0), values, (v, d1), check_invariants=False)
                if not ctx.sparse_grad:                     # coalesce first: a sort and a segmented sum, the same bits every call
                    grad_table = grad_table.coalesce().to_dense()
        return grad_table, None, None, None, grad_w, None


def lorentz_centroid(table: torch.Tensor, ids: torch.Tensor, offsets: torch.Tensor, lengths: Optional[torch.Tensor] = None,
                     weights: Optional[torch.Tensor] = None, *, sparse_grad: bool = True, validate: bool = True,
                     sign_convention: str = "lorentz") -> torch.Tensor:
    """The centroids ``[n, d + 1]`` described in the module docstring, differentiable in ``table`` and, when they require
    grad, in ``weights``.

    ``sparse_grad=True`` leaves an uncoalesced sparse COO gradient ``[V, d + 1]`` with ``T`` entries on ``table``;
    ``sparse_grad=False`` lets torch densify it.  ``validate=True`` checks ``offsets`` and ``lengths`` with one synchronising
    read and raises ``ValueError``; ``validate=False`` reads nothing back: the kernels clamp ``offsets`` into ``[0, T]`` and
    ``lengths`` into the span, so nothing outside the arrays is touched either way."""
    _check_args(table, ids, offsets, lengths, weights, sign_convention)
    if validate:
        _validate_segments(offsets, lengths, ids.numel())
    _require_cuda(table, ids, offsets, *(t for t in (lengths, weights) if t is not None))
    ids, offsets = ids.contiguous(), offsets.contiguous()
    lengths = None if lengths is None else lengths.contiguous()
    weights = None if weights is None else weights.contiguous()
    return _Centroid.apply(table, ids, offsets, lengths, weights, bool(sparse_grad))


class HyperbolicEmbeddingBag(torch.nn.Module):
    """``nn.EmbeddingBag`` on the hyperboloid: ``weight`` is a Lorentz table ``[num_embeddings, dim + 1]`` initialised like
    ``graph_embedding.init_table`` and ``forward`` returns the Lorentz centroid of every bag.  The gradient on ``weight`` is
    the sparse one of ``lorentz_centroid``; ``optim.RiemannianSGD`` / ``RiemannianAdam`` step it as it is."""

    def __init__(self, num_embeddings: int, dim: int, init_scale: float = 1e-3, seed: int = 0, device=None):
        super().__init__()
        if num_embeddings < 1 or not (MIN_WIDTH <= dim + 1 <= MAX_WIDTH):
            raise ValueError(f"HyperbolicEmbeddingBag: num_embeddings must be >= 1 and dim in {MIN_WIDTH - 1}..{MAX_WIDTH - 1}, got "
                             f"{num_embeddings}, {dim}")
        if device is None:
            device = "cuda" if torch.cuda.is_available() else "cpu"
        self.num_embeddings, self.dim = int(num_embeddings), int(dim)
        self.weight = torch.nn.Parameter(init_table(num_embeddings, dim, init_scale, seed, device))

    def forward(self, ids: torch.Tensor, offsets: torch.Tensor, lengths: Optional[torch.Tensor] = None,
                per_sample_weights: Optional[torch.Tensor] = None) -> torch.Tensor:
        return lorentz_centroid(self.weight, ids, offsets, lengths, per_sample_weights)

    def extra_repr(self) -> str:
        return f"{self.num_embeddings}, {self.dim}"
