"""The Riemannian optimiser step of DESIGN.md 5.16 written out in torch, the seeded cases and the error measure shared by
test_riemannian_host.py (no GPU) and test_gpu_riemannian.py.

The truth of a case is the step evaluated by torch on the CPU in float64, straight from the formulas; the place of a
reference is taken by the same code run in float32 on the CPU, whose error against the truth is e_ref.  Both start from the
same fp32 inputs and use the hyper-parameters as the fp32 values the kernel receives (``f32``; the rule of
poincare_cases._c).  The measure, ``FACTOR`` and ``FLOOR`` are those of tests/autograd_cases.py: the largest absolute error
of an array relative to the array's largest magnitude, ``e_hip <= FACTOR * e_ref + FLOOR``, non-finite entries compared by
position and kind.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

from autograd_cases import FACTOR, FLOOR, grad_error  # noqa: F401  (re-exported)

WIDTHS = (2, 3, 5, 17, 65, 66, 101, 129)                       # d1: spatial widths 1..128, both sides of the 16 / 32-lane switch
ROWS = (1, 3, 37, 257)                                         # partly filled group, partly filled wave, several blocks


def f32(x) -> float:
    return float(np.float32(x))


def ldot(a, b):
    return -a[..., 0] * b[..., 0] + (a[..., 1:] * b[..., 1:]).sum(-1)


def lift(s):
    """Spatial part -> point of the hyperboloid."""
    return torch.cat([torch.sqrt(1 + (s * s).sum(-1, keepdim=True)), s], -1)


def rgrad(x, g):
    h = torch.cat([-g[..., :1], g[..., 1:]], -1)
    return h + ldot(x, h).unsqueeze(-1) * x


def retract(x, s):
    n = torch.sqrt(torch.clamp(ldot(s, s), min=0)).unsqueeze(-1)
    one = torch.ones_like(n)
    coef = torch.where(n > 0, torch.sinh(n) / torch.where(n > 0, n, one), one)
    y = torch.cosh(n) * x + coef * s
    return lift(y[..., 1:])


def transport(x, y, w):
    w = w + (ldot(y, w) / (1 - ldot(x, y))).unsqueeze(-1) * (x + y)
    return w + ldot(y, w).unsqueeze(-1) * y


def sgd_step(x, g, m, lr, momentum=0.0, dampening=0.0, nesterov=False):
    """-> (x', m'); m' is None without momentum."""
    lr, mu, damp = f32(lr), f32(momentum), f32(dampening)
    u = rgrad(x, g)
    if mu == 0.0:
        return retract(x, -lr * u), None
    m2 = mu * m + (1 - damp) * u
    d = u + mu * m2 if nesterov else m2
    y = retract(x, -lr * d)
    return y, transport(x, y, m2)


def bias_corrections(beta1, beta2, t):
    """(bc1, bc2) in double from the fp32 betas, then as the fp32 values the kernel receives."""
    return f32(1.0 - f32(beta1) ** t), f32(1.0 - f32(beta2) ** t)


def adam_step(x, g, m, v, t, lr, beta1=0.9, beta2=0.999, eps=1e-8):
    """-> (x', m', v')."""
    lr, b1, b2, eps = f32(lr), f32(beta1), f32(beta2), f32(eps)
    bc1, bc2 = bias_corrections(beta1, beta2, t)
    u = rgrad(x, g)
    m2 = b1 * m + (1 - b1) * u
    v2 = b2 * v + (1 - b2) * ldot(u, u)
    d = (m2 / bc1) / (torch.sqrt(v2 / bc2) + eps).unsqueeze(-1)
    y = retract(x, -lr * d)
    return y, transport(x, y, m2), v2


#: name -> (optimiser, keyword arguments of the step, first step number of RAdam)
SETTINGS = {
    "sgd": ("sgd", dict(lr=0.1), 0),
    "sgd_mom": ("sgd", dict(lr=0.1, momentum=0.9), 0),
    "sgd_damp": ("sgd", dict(lr=0.1, momentum=0.9, dampening=0.1), 0),
    "sgd_nesterov": ("sgd", dict(lr=0.1, momentum=0.9, nesterov=True), 0),
    "adam_t1": ("adam", dict(lr=0.05, beta1=0.9, beta2=0.999, eps=1e-8), 1),
    "adam_t3": ("adam", dict(lr=0.05, beta1=0.9, beta2=0.999, eps=1e-8), 3),
}


@functools.lru_cache(maxsize=None)
def inputs(rows: int, d1: int, scale: float, seed: int, steps: int = 1):
    """Seeded fp32 inputs: x on the hyperboloid with spatial norm about ``scale``, ``steps`` gradients, a tangent m, v > 0.

    Size of the gradients.  The transport divides and multiplies by quantities of size |x'|, so a rounding error of the
    step reaches m' multiplied by about |x'|^2, and |x'| grows like cosh of the geodesic length of the step.  A step several
    units long (|x'| of 50 and more) makes the fp32 error of m' the outcome of a single cancellation in a single row -- one
    ulp of cosh moves it by an order of magnitude either way -- and a rule that compares two fp32 evaluations by a factor
    of 4 then measures luck.  The cases therefore use steps of the length an optimiser is run at, a fraction of a unit: with
    x0 ~ sqrt(1 + scale^2), <u, u> = <h, h> + <x, h>^2 <= about 3 x0^2 |g|^2, so Gaussian gradients of Euclidean norm
    1 / x0 (entries of deviation 1 / sqrt(d1 (1 + scale^2))) give |u| below about 1.7, a momentum built the same way,
    directions u + mu m+ below about 6 and, at the rates of SETTINGS, steps of length up to about 0.6.  RAdam's second
    moment comes in at the size of <u, u>.  The cancellation in the tangent projection far from the origin (scale 6) is
    untouched by this: it comes from |x|, not from the step."""
    gen = torch.Generator().manual_seed(seed)
    d = d1 - 1
    k = 1.0 / np.sqrt(d1 * (1.0 + scale * scale))
    x = lift(torch.randn(rows, d, generator=gen, dtype=torch.float64) * (scale / np.sqrt(d))).float()
    g = [(torch.randn(rows, d1, generator=gen, dtype=torch.float64) * k).float() for _ in range(steps)]
    m = rgrad(x.double(), torch.randn(rows, d1, generator=gen, dtype=torch.float64) * k).float()
    v = ((0.5 + torch.rand(rows, generator=gen, dtype=torch.float64)) * 2.0).float()
    return x, g, m, v


def run(setting: str, x, gs, m, v, dtype):
    """The chained steps of ``setting`` in ``dtype`` on the CPU -> one dict {"x", "m", "v"} (numpy; absent state omitted) per step."""
    opt, kw, t0 = SETTINGS[setting]
    x, m, v = x.to(dtype), m.to(dtype), v.to(dtype)
    out = []
    for k, g in enumerate(gs):
        g = g.to(dtype)
        if opt == "sgd":
            x, m2 = sgd_step(x, g, m, **kw)
            m = m if m2 is None else m2
            out.append({"x": x.numpy()} if m2 is None else {"x": x.numpy(), "m": m.numpy()})
        else:
            x, m, v = adam_step(x, g, m, v, t0 + k, **kw)
            out.append({"x": x.numpy(), "m": m.numpy(), "v": v.numpy()})
    return out


@functools.lru_cache(maxsize=None)
def reference(setting: str, rows: int, d1: int, scale: float, seed: int, steps: int = 1):
    """(float64 truth, fp32 CPU result) of a seeded case, computed once."""
    x, gs, m, v = inputs(rows, d1, scale, seed, steps)
    return run(setting, x, gs, m, v, torch.float64), run(setting, x, gs, m, v, torch.float32)


def compare(name: str, truth, ref32, ours, failures: list) -> None:
    """Prints ``name e_ref e_hip`` for every array of every step and appends what misses the bound to ``failures``."""
    for k, (t, r, o) in enumerate(zip(truth, ref32, ours)):
        for q in t:
            e_ref, _ = grad_error(r[q], r[q], t[q])
            e_hip, pattern_ok = grad_error(np.asarray(o[q]).reshape(r[q].shape), r[q], t[q])
            print(f"{name}:step{k + 1}:{q} e_ref={e_ref:.3e} e_hip={e_hip:.3e}")
            if not pattern_ok:
                failures.append(f"{name}:step{k + 1}:{q}: non-finite pattern differs from the fp32 reference's")
            elif not e_hip <= FACTOR * e_ref + FLOOR:
                failures.append(f"{name}:step{k + 1}:{q}: e_ref={e_ref:.3e} e_hip={e_hip:.3e}")


# ---- end to end: 16 rows of width 5 pulled towards 5 fixed points -------------------------------------------------------
E2E = {"sgd": dict(lr=0.02, momentum=0.9), "adam": dict(lr=0.05)}
E2E_STEPS = 200


def e2e_inputs():
    gen = torch.Generator().manual_seed(2024)
    x = lift(torch.randn(16, 4, generator=gen, dtype=torch.float64)).float()
    p = lift(torch.randn(5, 4, generator=gen, dtype=torch.float64)).float()
    return x, p


def e2e_loss(x, p):
    u = torch.clamp(-ldot(x.unsqueeze(1), p.unsqueeze(0)), min=1.0 + 1e-8)
    return (torch.acosh(u) ** 2).sum()


@functools.lru_cache(maxsize=None)
def e2e_loop(opt: str, dtype):
    """The training loop on the CPU in ``dtype`` -> (initial loss, final loss, final x as numpy)."""
    x, p = (t.to(dtype) for t in e2e_inputs())
    m, v = torch.zeros_like(x), torch.zeros(x.shape[0], dtype=dtype)
    first = None
    for t in range(1, E2E_STEPS + 1):
        xr = x.clone().requires_grad_(True)
        loss = e2e_loss(xr, p)
        loss.backward()
        first = float(loss.detach()) if first is None else first
        if opt == "sgd":
            x, m = sgd_step(x, xr.grad, m, **E2E["sgd"])
        else:
            x, m, v = adam_step(x, xr.grad, m, v, t, **E2E["adam"])
    return first, float(e2e_loss(x, p)), x.numpy()
