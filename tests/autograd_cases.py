"""Float64 "truth" expressions and the error measure shared by the autograd tests (test_autograd_golden.py without a
GPU, test_gpu_autograd.py with one).

The truth of a case is the same expression as the reference's, evaluated by torch on the CPU in float64 from the
golden's fp32 inputs and differentiated by torch's autograd.  ``sign`` is +1 for the "reference" convention
(``minkowski_dot = x0*y0 - sum``) and -1 for "lorentz".  A gradient is compared entry by entry: where the reference's
recorded fp32 gradient is finite the error is ``|value - truth|`` relative to the largest finite ``|truth|`` of the
case; where it is not finite the value must be non-finite of the same kind (NaN, +inf, -inf) in the same position.
"""
from __future__ import annotations

import numpy as np
import torch

SIGN = {"reference": 1.0, "lorentz": -1.0}
FLOOR = 2.0 ** -20
FACTOR = 4.0


def mdot(x, y, sign):
    return sign * (x[..., 0] * y[..., 0] - (x[..., 1:] * y[..., 1:]).sum(-1))


def dist(x, y, c, sign):
    u = torch.clamp(-mdot(x, y, sign), min=1.0 + 1e-8)
    return torch.acosh(u) / torch.sqrt(torch.tensor(c, dtype=x.dtype))


def log_map(x, y, sign):
    m = mdot(x, y, sign)
    u = torch.clamp(-m, min=1.0 + 1e-8)
    coef = torch.clamp(torch.acosh(u) / torch.sqrt(u * u - 1), max=1e4)
    mask = ((coef != coef) | (coef > 1e4)).to(coef.dtype)
    coef = mask * torch.ones_like(coef) + (1 - mask) * coef
    return coef.unsqueeze(-1) * (y + m.unsqueeze(-1) * x)


def exp_map(x, v):
    n = torch.sqrt(torch.clamp((v[..., 1:] * v[..., 1:]).sum(-1, keepdim=True), min=1e-8))
    mask = (n < 1e-6).to(v.dtype)
    direction = v / (n + mask)
    direction = mask * torch.zeros_like(direction) + (1 - mask) * direction
    return torch.cosh(n) * x + torch.sinh(n) * direction


def project(x, c):
    n = torch.norm(x[..., 1:], dim=-1, keepdim=True)
    return torch.cat([torch.sqrt(1.0 + c * n * n), x[..., 1:]], dim=-1)


def batch_dist(x, y, c, sign):
    return dist(x.unsqueeze(1), y.unsqueeze(0), c, sign)


def reduce(losses, reduction):
    return losses.mean() if reduction == "mean" else losses.sum() if reduction == "sum" else losses


def infonce(zt, zi, temp, reduction, sign):
    s = -batch_dist(zt, zi, 1.0, sign) / temp
    labels = torch.arange(zt.shape[0])
    ce = torch.nn.functional.cross_entropy
    return (ce(s, labels, reduction=reduction) + ce(s.t(), labels, reduction=reduction)) / 2.0


def triplet(a, p, n, margin, reduction, sign):
    return reduce(torch.relu(dist(a, p, 1.0, sign) - dist(a, n, 1.0, sign) + margin), reduction)


#: op -> (names of the differentiable inputs, expression(inputs, params, sign))
OPS = {
    "minkowski": (("x", "y"), lambda t, p, s: mdot(t["x"], t["y"], s)),
    "distance": (("x", "y"), lambda t, p, s: dist(t["x"], t["y"], p["c"], s)),
    "log_map": (("x", "y"), lambda t, p, s: log_map(t["x"], t["y"], s)),
    "exp_map": (("x", "y"), lambda t, p, s: exp_map(t["x"], t["y"])),
    "project": (("x",), lambda t, p, s: project(t["x"], p["c"])),
    "batch_distance": (("x", "y"), lambda t, p, s: batch_dist(t["x"], t["y"], p["c"], s)),
    "batch_distance_optimized": (("x", "y"), lambda t, p, s: batch_dist(t["x"], t["y"], p["c"], s)),
    "infonce": (("x", "y"), lambda t, p, s: infonce(t["x"], t["y"], p["temp"], p["reduction"], s)),
    "triplet": (("x", "y", "z"), lambda t, p, s: triplet(t["x"], t["y"], t["z"], p["margin"], p["reduction"], s)),
}


def truth(case: dict, arrays, mode: str):
    """(forward value, {input name: gradient}) in float64 for one golden case."""
    names, fn = OPS[case["op"]]
    t = {k: torch.from_numpy(np.asarray(arrays[f"{case['name']}__{k}"])).double().requires_grad_() for k in names}
    out = fn(t, case["params"], SIGN[mode])
    g = torch.from_numpy(np.asarray(arrays[f"{case['name']}__g"])).double()
    out.backward(g.reshape(out.shape))
    return out.detach().numpy(), {k: t[k].grad.numpy() for k in names}


def _kind(a):
    a = np.asarray(a, np.float64)
    return np.where(np.isnan(a), 3, np.where(np.isposinf(a), 1, np.where(np.isneginf(a), 2, 0)))


def grad_error(value, ref32, true64):
    """(error relative to max |truth| over the entries where ``ref32`` is finite, pattern_ok)."""
    value, ref32, true64 = (np.asarray(a, np.float64) for a in (value, ref32, true64))
    fin = np.isfinite(ref32)
    pattern_ok = bool(np.array_equal(_kind(value)[~fin], _kind(ref32)[~fin]) and np.isfinite(value[fin]).all())
    tf = true64[np.isfinite(true64)]
    scale = max(float(np.abs(tf).max()) if tf.size else 0.0, 1e-30)
    use = fin & np.isfinite(true64)
    err = float(np.abs(value[use] - true64[use]).max()) / scale if use.any() else 0.0
    return err, pattern_ok
