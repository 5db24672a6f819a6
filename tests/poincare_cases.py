"""Float64 "truth" expressions of the Poincare-ball ops and the error measure shared by test_poincare_golden.py (no GPU)
and test_gpu_poincare.py.

The truth of a case is the reference's expression (embedding/poincare_ball.py), written out here from its formulas and
evaluated by torch on the CPU in float64 from the golden's fp32 inputs, then differentiated by torch's autograd.  The
curvature is the fp32 value the reference and the kernels see (``float(np.float32(c))``).  The measure, ``FACTOR`` and
``FLOOR`` are those of tests/autograd_cases.py: an entry is compared where the reference's recorded fp32 value is finite,
as ``|value - truth|`` relative to the largest finite ``|truth|`` of the array; elsewhere the value must be non-finite of
the same kind in the same position.
"""
from __future__ import annotations

import numpy as np
import torch

from autograd_cases import FACTOR, FLOOR, grad_error  # noqa: F401  (re-exported)

CLAMP = 1e-8
DIMS = (1, 2, 5, 32, 100, 128)
ODD_DIMS = (50, 101)                                           # extra widths that are no multiple of 4 (at c = 0.7 only)
CURVATURES = (1.0, 0.7, 2.0)


def _c(c, like):
    return torch.tensor(float(np.float32(c)), dtype=like.dtype)


def norm(x):
    return torch.sqrt((x * x).sum(-1, keepdim=True))


def mobius_addition(x, y, c):
    c = _c(c, x)
    x2, y2, xy = (x * x).sum(-1, keepdim=True), (y * y).sum(-1, keepdim=True), (x * y).sum(-1, keepdim=True)
    num = (1 + 2 * c * xy + c * y2) * x + (1 - c * x2) * y
    return num / (1 + 2 * c * xy + c * c * x2 * y2)


def mobius_scalar_mul(r, x, c):
    a = torch.sqrt(_c(c, x)) * torch.clamp(norm(x), min=CLAMP)
    return torch.tanh(r * torch.atanh(a)) / a * x


def _zero_map(f, v, c):
    n = norm(v)
    mask = (n == 0).to(v.dtype)
    a = torch.sqrt(_c(c, v)) * torch.clamp(n, min=CLAMP)
    return f(a) / a * v * (1 - mask) + mask * v


def exp_map_zero(v, c):
    return _zero_map(torch.tanh, v, c)


def log_map_zero(x, c):
    return _zero_map(torch.atanh, x, c)


def distance(x, y, c):
    sc = torch.sqrt(_c(c, x))
    return 2 / sc * torch.atanh(sc * norm(mobius_addition(-x, y, c)))


def lorentz_to_poincare(x, c):
    return x[..., 1:] / (x[..., 0:1] + 1 / torch.sqrt(_c(c, x)))


def poincare_to_lorentz(x, c):
    """As shipped: x0^2 - |x_s|^2 = 1 / (4c)."""
    c = _c(c, x)
    x2 = (x * x).sum(-1, keepdim=True)
    f = 1.0 / (1 - c * x2)
    return torch.cat([f * (1 + c * x2) / (2 * torch.sqrt(c)), f * x], dim=-1)


def poincare_to_lorentz_standard(x, c):
    c = _c(c, x)
    x2 = (x * x).sum(-1, keepdim=True)
    return torch.cat([(1 + c * x2) / (torch.sqrt(c) * (1 - c * x2)), 2 * x / (1 - c * x2)], dim=-1)


#: op -> (names of the differentiable inputs in call order, expression(inputs..., c))
OPS = {
    "norm": (("x",), lambda x, c: norm(x)),
    "mobius_addition": (("x", "y"), mobius_addition),
    "mobius_scalar_mul": (("r", "x"), mobius_scalar_mul),
    "exp_map_zero": (("x",), exp_map_zero),
    "log_map_zero": (("x",), log_map_zero),
    "distance": (("x", "y"), distance),
    "lorentz_to_poincare": (("x",), lorentz_to_poincare),
    "poincare_to_lorentz": (("x",), poincare_to_lorentz),
}


def truth(case: dict, arrays):
    """(forward value, {input name: gradient}) in float64 for one golden case."""
    names, fn = OPS[case["op"]]
    t = {k: torch.from_numpy(np.asarray(arrays[f"{case['name']}__{k}"])).double().requires_grad_() for k in names}
    out = fn(*[t[k] for k in names], case["c"])
    g = torch.from_numpy(np.asarray(arrays[f"{case['name']}__g"])).double()
    out.backward(g.reshape(out.shape))
    return out.detach().numpy(), {k: t[k].grad.numpy() for k in names}


def quantities(case: dict):
    """The compared arrays of a case: the forward value and one gradient per input."""
    return ["out"] + [f"g{k}" for k in OPS[case["op"]][0]]


def errors(case: dict, arrays, values=None):
    """{quantity: (error, pattern_ok)} of ``values`` (default: the recorded reference arrays) against the float64 truth."""
    out64, grads64 = truth(case, arrays)
    true = {"out": out64, **{f"g{k}": v for k, v in grads64.items()}}
    res = {}
    for q in quantities(case):
        rec = arrays[f"{case['name']}__{q}"]
        val = rec if values is None else values[q]
        res[q] = grad_error(np.asarray(val).reshape(rec.shape), rec, true[q])
    return res
