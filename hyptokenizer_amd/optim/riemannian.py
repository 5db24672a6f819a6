"""Riemannian SGD and Riemannian Adam for parameters whose rows are points of the unit hyperboloid.

A parameter is an fp32 tensor ``[..., d + 1]`` on a HIP device whose rows satisfy ``<x, x> = -1`` under
``<a, b> = -a0 b0 + sum_k ak bk`` -- the package's ``sign_convention="lorentz"``.  ``step()`` turns the Euclidean gradient
autograd left in ``.grad`` into the Riemannian one, moves every row along the geodesic (exponential map, time coordinate
recomputed from the spatial part) and carries the first moment to the new point by parallel transport, all in one kernel
launch per parameter and in place (``hm_rsgd_step`` / ``hm_radam_step``).  The formulas are those of
DESIGN.md 5.16 (Bonnabel 2013; Nickel & Kiela 2018; Becigneul & Ganea 2019), not ``lorentz_model.exp_map`` /
``parallel_transport`` / ``riemannian_gradient``, which reproduce the reference's expressions.

Curvature is not an argument: ``c`` only scales distances (``acosh(u) / sqrt(c)``), so it is folded into ``lr``.  Under
``sign_convention="reference"`` every distance of the package is 0 and its gradient vanishes: these optimisers are of use
with ``"lorentz"`` only.  Not implemented: weight decay, AMSGrad, Poincare-ball parameters.

Gradients.  A dense ``.grad`` updates every row.  A sparse COO ``.grad`` of a 2-D parameter (``nn.Embedding(sparse=True)``,
``sparse_grad=True``) is coalesced and only the rows it lists are updated; the moments are then lazy (rows not listed keep
their moments untouched) and the step counter of the bias correction counts the parameter's steps, as in
``torch.optim.SparseAdam``.  ``step()`` runs under ``torch.no_grad()`` on the current stream and reads nothing back from
the device (what ``Tensor.coalesce`` does for an uncoalesced sparse gradient is torch's business).

Hyper-parameters reach the kernel as fp32 values; the bias corrections ``1 - beta^t`` are computed on the host in double
from those fp32 betas.  State: ``momentum_buffer`` (RSGD with momentum) or ``exp_avg``, ``exp_avg_sq`` (one value per row)
and ``step`` (a Python int); a run resumed through ``state_dict`` / ``load_state_dict`` continues bit for bit.  Unlike
``torch.optim.SGD`` the first momentum step applies the dampening too (``m+ = mu m + (1 - dampening) u`` from ``m = 0``).
"""
from __future__ import annotations

import ctypes as C
import math

import torch

from .. import _lib
from ..embedding._table import MAX_WIDTH, MIN_WIDTH
from ..engine import _ptr, _require_cuda, _stream_of


def _f32(x: float) -> float:
    """The fp32 value the kernel receives for ``x``, as a Python float."""
    return C.c_float(float(x)).value


def _collapsible(shape, stride) -> bool:
    """Whether the leading dimensions of a tensor with unit last stride flatten into one row index with one row stride."""
    if stride[-1] != 1 and shape[-1] > 1:
        return False
    lead = [(n, s) for n, s in zip(shape[:-1], stride[:-1]) if n != 1]
    for (_, s_outer), (n_inner, s_inner) in zip(lead[:-1], lead[1:]):
        if s_outer != s_inner * n_inner:
            return False
    return not lead or lead[-1][1] >= shape[-1]


def _rows_of(t: torch.Tensor):
    """(rows, leading dimension) of ``t`` [..., d1] seen as a table of rows; ``t`` must pass ``_collapsible``."""
    d1 = t.shape[-1]
    rows = t.numel() // d1
    lead = [(n, s) for n, s in zip(t.shape[:-1], t.stride()[:-1]) if n != 1]
    return rows, (lead[-1][1] if lead else d1)


def _check_param(name: str, p: torch.Tensor) -> None:
    if p.dtype != torch.float32:
        raise ValueError(f"{name}: parameters must be float32, got {p.dtype}")
    if p.dim() < 1 or not (MIN_WIDTH <= p.shape[-1] <= MAX_WIDTH):
        raise ValueError(f"{name}: the last dimension (d + 1) must lie in {MIN_WIDTH}..{MAX_WIDTH}, got shape {tuple(p.shape)}")
    if not _collapsible(p.shape, p.stride()):
        raise ValueError(f"{name}: a parameter needs unit stride in its last dimension and leading dimensions that flatten "
                         f"into one row stride (shape {tuple(p.shape)}, strides {p.stride()})")


def _dense_grad(p: torch.Tensor) -> torch.Tensor:
    g = p.grad
    if g.dtype != torch.float32:
        g = g.float()
    if not _collapsible(g.shape, g.stride()):
        g = g.contiguous()
    return g


def _sparse_grad(name: str, p: torch.Tensor):
    """(row indices int64 [n], values fp32 [n, d1]) of the coalesced sparse gradient: distinct rows."""
    if p.dim() != 2:
        raise ValueError(f"{name}: a sparse gradient needs a 2-D parameter, got shape {tuple(p.shape)}")
    g = p.grad.coalesce()
    if g.sparse_dim() != 1:
        raise ValueError(f"{name}: a sparse gradient must index rows only (sparse_dim 1), got {g.sparse_dim()}")
    idx = g.indices()[0].contiguous()
    val = g.values()
    if val.dtype != torch.float32:
        val = val.float()
    return idx, val.contiguous()


class _RiemannianOptimizer(torch.optim.Optimizer):
    def add_param_group(self, param_group):                  # also reached from __init__, once per group
        super().add_param_group(param_group)
        for p in self.param_groups[-1]["params"]:
            _check_param(type(self).__name__, p)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        L = _lib.load()
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is None:
                    continue
                _require_cuda(p, p.grad)
                _check_param(type(self).__name__, p)          # p.data may have been replaced since construction
                rows, ld = _rows_of(p)
                if p.grad.is_sparse:
                    idx, g = _sparse_grad(type(self).__name__, p)
                    n, ld_g = idx.shape[0], p.shape[-1]
                else:
                    g = _dense_grad(p)
                    idx, n, ld_g = None, rows, _rows_of(g)[1]
                with torch.cuda.device(p.device):
                    self._step_param(L, group, p, rows, ld, g, ld_g, idx, n, _stream_of(p))
        return loss

    def _step_param(self, L, group, p, rows, ld, g, ld_g, idx, n, stream):
        raise NotImplementedError


class RiemannianSGD(_RiemannianOptimizer):
    """Riemannian SGD on the unit hyperboloid: ``m+ = momentum m + (1 - dampening) u``, a geodesic step of ``-lr m+``
    (Nesterov: ``-lr (u + momentum m+)``), ``m+`` transported to the new point.  With ``momentum = 0`` there is no state
    and the step is ``-lr u``.  See the module docstring for what a parameter and its gradient may be."""

    def __init__(self, params, lr, momentum=0.0, dampening=0.0, nesterov=False):
        if not (math.isfinite(lr) and lr >= 0.0):
            raise ValueError(f"RiemannianSGD: invalid learning rate {lr}")
        if not 0.0 <= momentum < 1.0:
            raise ValueError(f"RiemannianSGD: momentum {momentum} is outside [0, 1)")
        if not 0.0 <= dampening < 1.0:
            raise ValueError(f"RiemannianSGD: dampening {dampening} is outside [0, 1)")
        if nesterov and momentum == 0.0:
            raise ValueError("RiemannianSGD: Nesterov momentum needs momentum > 0")
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, nesterov=bool(nesterov)))

    def _step_param(self, L, group, p, rows, ld, g, ld_g, idx, n, stream):
        mu = _f32(group["momentum"])
        buf = None
        if mu != 0.0:
            state = self.state[p]
            if "momentum_buffer" not in state:
                state["momentum_buffer"] = torch.zeros(p.shape, dtype=torch.float32, device=p.device)
            buf = state["momentum_buffer"]
        _lib.check(L.hm_rsgd_step(_ptr(p), ld, _ptr(g), ld_g, _ptr(buf), p.shape[-1], _ptr(idx), n, rows, p.shape[-1],
                                  group["lr"], mu, group["dampening"], int(group["nesterov"]), stream))


class RiemannianAdam(_RiemannianOptimizer):
    """Riemannian Adam on the unit hyperboloid (Becigneul & Ganea 2019): ``m+ = b1 m + (1 - b1) u``, one second moment per
    row ``v+ = b2 v + (1 - b2) <u, u>``, a geodesic step of ``-lr (m+ / bc1) / (sqrt(v+ / bc2) + eps)``, ``m+`` transported
    to the new point.  See the module docstring for what a parameter and its gradient may be."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
        if not (math.isfinite(lr) and lr >= 0.0):
            raise ValueError(f"RiemannianAdam: invalid learning rate {lr}")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"RiemannianAdam: betas {betas} are outside [0, 1)")
        if not (math.isfinite(eps) and eps >= 0.0):
            raise ValueError(f"RiemannianAdam: invalid eps {eps}")
        super().__init__(params, dict(lr=lr, betas=(float(betas[0]), float(betas[1])), eps=eps))

    def _step_param(self, L, group, p, rows, ld, g, ld_g, idx, n, stream):
        state = self.state[p]
        if "step" not in state:
            state["step"] = 0
            state["exp_avg"] = torch.zeros(p.shape, dtype=torch.float32, device=p.device)
            state["exp_avg_sq"] = torch.zeros(rows, dtype=torch.float32, device=p.device)
        state["step"] = t = int(state["step"]) + 1
        b1, b2 = _f32(group["betas"][0]), _f32(group["betas"][1])
        bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t                # in double, from the fp32 betas the kernel uses
        _lib.check(L.hm_radam_step(_ptr(p), ld, _ptr(g), ld_g, _ptr(state["exp_avg"]), p.shape[-1], _ptr(state["exp_avg_sq"]),
                                   _ptr(idx), n, rows, p.shape[-1], group["lr"], b1, b2, group["eps"], bc1, bc2, stream))
