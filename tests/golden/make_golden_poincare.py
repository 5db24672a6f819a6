#!/usr/bin/env python
"""Generate tests/golden/g13_poincare.{npz,json} by running the REFERENCE's ``embedding/poincare_ball.py`` under torch
autograd on the CPU.

Like make_golden_autograd.py it runs only where the reference is present (it is imported, never copied).  The curvature
is passed as a 0-d fp32 tensor: with a Python float three of the reference's eight functions raise ``TypeError``
(``torch.sqrt(c)``), with a tensor all eight run.  There is no sign-convention split: this module has no Minkowski form.

The npz holds, for every case ``<name>``: the fp32 inputs ``<name>__x`` (``__y``, or ``__r`` and ``__x`` for
``mobius_scalar_mul``), the upstream gradient ``<name>__g``, the reference's fp32 forward value ``<name>__out`` and its
fp32 gradients ``<name>__gx`` (``__gy``, ``__gr``).  The json lists the cases (op, ``c``, the radius cap of the drawn
points, whether the case is ordinary, whether every recorded array is finite) with ``e_ref``: the largest error of the
reference's fp32 forward value and gradients against the float64 truth of tests/poincare_cases.py.

Ordinary cases: every op at d in {1, 2, 5, 32, 100, 128} and c in {1.0, 0.7, 2.0}, and at d in {50, 101} with c = 0.7; points with sqrt(c)|x| <= cap (0.9
unless OP_CAP lowers it for an op), ``distance`` pairs at least 0.05 / sqrt(c) apart; e_ref <= 1e-4 is asserted.
Special cases are recorded as the reference gives them, non-finite values included: zero vectors in both zero-maps,
norms below the 1e-8 clamp, a point on the boundary and one outside it, x == y in ``distance``, r = 0 and negative r,
broadcast operands (a single row against many, a 3-D batch).

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_poincare.py
"""
from __future__ import annotations

import json
import os
import sys
import warnings

REF = "/root/reference"
if not os.path.isdir(REF):
    sys.exit("make_golden_poincare.py: /root/reference is not present; golden vectors can only be regenerated "
             "in the build container.")

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, REF)
warnings.filterwarnings("ignore")

import numpy as np  # noqa: E402
import torch  # noqa: E402

import embedding.lorentz_model as L  # noqa: E402  (reference)
import embedding.poincare_ball as P  # noqa: E402  (reference)

import poincare_cases as PC  # noqa: E402  (ours: float64 truth and the error measure)

E_REF_MAX = 1e-4
CAP = 0.9
#: radius cap per op where 0.9 cannot meet E_REF_MAX (none needed so far)
OP_CAP = {}
ROWS = {1: 16, 2: 16, 5: 16, 32: 8, 100: 3, 128: 3}
FNS = {"norm": P.norm, "mobius_addition": P.mobius_addition, "mobius_scalar_mul": P.mobius_scalar_mul,
       "exp_map_zero": P.exp_map_zero, "log_map_zero": P.log_map_zero, "distance": P.distance,
       "lorentz_to_poincare": P.lorentz_to_poincare, "poincare_to_lorentz": P.poincare_to_lorentz}


def ball(gen, n, d, c, cap, lo=0.1):
    """n points with sqrt(c) |x| uniform in [lo, cap]."""
    v = torch.randn(n, d, generator=gen)
    v = v / v.norm(dim=-1, keepdim=True)
    r = lo + (cap - lo) * torch.rand(n, 1, generator=gen)
    return (v * r / np.sqrt(c)).float()


def apart(gen, x, c, cap):
    """Points like ``ball`` at least 0.05 / sqrt(c) away from the rows of x."""
    y = ball(gen, x.shape[0], x.shape[1], c, cap)
    for _ in range(200):
        bad = (x - y).norm(dim=-1) * np.sqrt(c) < 0.05
        if not bool(bad.any()):
            return y
        y[bad] = ball(gen, int(bad.sum()), x.shape[1], c, cap)
    raise AssertionError("could not separate the points")


def run_case(op, c, inputs, g=None):
    leaves = [t.clone().float().requires_grad_() for t in inputs]
    ct = torch.tensor(c, dtype=torch.float32)
    out = FNS[op](*leaves) if op == "norm" else FNS[op](*leaves, ct)
    if g is None:
        g = torch.ones_like(out)
    out.backward(g)
    return out.detach(), [t.grad if t.grad is not None else torch.zeros_like(t) for t in leaves], g


def generate() -> None:
    gen = torch.Generator().manual_seed(20240913)
    arrays, cases = {}, []

    def add(name, op, c, inputs, ordinary=False, cap=None):
        names = PC.OPS[op][0]
        shape = run_case(op, c, inputs)[0].shape
        g = torch.randn(shape, generator=gen)
        out, grads, g = run_case(op, c, inputs, g)
        case = {"name": name, "op": op, "c": c, "ordinary": bool(ordinary), "cap": cap}
        for key, t in zip(names, inputs):
            arrays[f"{name}__{key}"] = t.float().numpy()
        arrays[f"{name}__g"] = g.numpy()
        arrays[f"{name}__out"] = out.numpy()
        for key, t in zip(names, grads):
            arrays[f"{name}__g{key}"] = t.numpy()
        errs = PC.errors(case, arrays)
        assert all(ok for _, ok in errs.values()), name
        case["e_ref"] = max(e for e, _ in errs.values())
        case["finite"] = bool(all(np.isfinite(arrays[f"{name}__{q}"]).all() for q in PC.quantities(case)))
        if ordinary:
            assert case["e_ref"] <= E_REF_MAX, (name, case["e_ref"], errs)
            assert case["finite"], name
        cases.append(case)
        return case

    # ---- ordinary cases -----------------------------------------------------------------------------------------
    for op in PC.OPS:
        cap = OP_CAP.get(op, CAP)
        for d in PC.DIMS:
            for c in PC.CURVATURES:
                b = ROWS[d]
                x = ball(gen, b, d, c, cap)
                if op in ("mobius_addition", "distance"):
                    inputs = [x, apart(gen, x, c, cap)]
                elif op == "mobius_scalar_mul":
                    inputs = [(torch.rand(b, 1, generator=gen) * 4 - 2).float(), x]
                elif op == "lorentz_to_poincare":
                    inputs = [L.project_to_hyperboloid(torch.randn(b, d + 1, generator=gen) * 0.5, c).detach()]
                else:
                    inputs = [x]
                add(f"{op}_d{d}_c{c}", op, c, inputs, ordinary=True, cap=cap)

    # ---- special cases ------------------------------------------------------------------------------------------
    d = 5
    z = ball(gen, 6, d, 1.0, CAP)
    z[0] = 0.0
    z[3] = 0.0
    add("expzero_zero_rows", "exp_map_zero", 1.0, [z.clone()])
    add("logzero_zero_rows", "log_map_zero", 0.7, [z.clone()])
    t = ball(gen, 6, d, 2.0, CAP)
    t[0] = 1e-9                                                           # norm 2.2e-9 < 1e-8: clamp active, norm not 0
    t[1] = 0.0
    t[1, 2] = 5e-9
    t[2] = 1e-4                                                           # small but above the clamp
    for op in ("exp_map_zero", "log_map_zero"):
        add(f"{op}_below_clamp", op, 2.0, [t.clone()])
    add("scalarmul_below_clamp", "mobius_scalar_mul", 2.0, [(torch.rand(6, 1, generator=gen) * 2 - 1).float(), t.clone()])
    tz = t.clone()
    tz[3] = 0.0
    add("scalarmul_zero_row", "mobius_scalar_mul", 2.0, [(torch.rand(6, 1, generator=gen) * 2 - 1).float(), tz])
    e = ball(gen, 4, d, 1.0, CAP)
    e[0] = 0.0
    e[0, 1] = 1.0                                                         # on the boundary: sqrt(c) |x| == 1 exactly
    e[1] = 0.0
    e[1, 0] = 1.5                                                         # outside the ball
    e[1, 3] = -0.5
    add("logzero_boundary", "log_map_zero", 1.0, [e.clone()])
    add("expzero_boundary", "exp_map_zero", 1.0, [e.clone()])
    add("scalarmul_boundary", "mobius_scalar_mul", 1.0, [torch.full((4, 1), 0.5), e.clone()])
    add("p2l_boundary", "poincare_to_lorentz", 1.0, [e.clone()])
    other = ball(gen, 4, d, 1.0, CAP)
    other[0] = 0.0                                                        # (-x) (+) 0 = -x: the norm is exactly 1, atanh exactly inf
    add("dist_boundary", "distance", 1.0, [e.clone(), other])
    add("mobadd_boundary", "mobius_addition", 1.0, [e.clone(), ball(gen, 4, d, 1.0, CAP)])
    s = ball(gen, 8, d, 1.0, CAP)
    s[0] = 0.0
    add("dist_identical", "distance", 1.0, [s, s.clone()])
    # x == y leaves rounding noise of a few 1e-8 in (-x) (+) y (or exactly 0), and the gradient of its norm is then a unit vector
    # along that noise times the conformal factor 2 / (1 - c |x|^2): the float64 truth is 0 and e_ref is not a small number.
    # Identical rows are therefore kept in cases of their own, apart from rows whose gradient means something.
    half = torch.cat([ball(gen, 4, d, 0.7, 0.3), ball(gen, 4, d, 0.7, CAP, lo=0.7)])
    other = apart(gen, half, 0.7, CAP)
    add("dist_identical_c0.7", "distance", 0.7, [half[:4], half[:4].clone()])
    add("dist_near_boundary", "distance", 0.7, [half[4:], other[4:]])      # both points at sqrt(c) |x| in [0.7, 0.9]
    r = (torch.rand(8, 1, generator=gen) * 3).float()
    r[0] = 0.0
    r[1] = -1.0
    r[2] = -2.5
    r[3] = 1.0
    add("scalarmul_r_zero_negative", "mobius_scalar_mul", 0.7, [r, ball(gen, 8, d, 0.7, CAP)])
    # broadcast operands
    add("mobadd_bcast_row", "mobius_addition", 1.0, [ball(gen, 1, d, 1.0, CAP), ball(gen, 9, d, 1.0, CAP)])
    add("mobadd_bcast_3d", "mobius_addition", 2.0, [ball(gen, 3, d, 2.0, CAP).reshape(3, 1, d), ball(gen, 4, d, 2.0, CAP)])
    add("dist_bcast_row", "distance", 1.0, [ball(gen, 9, d, 1.0, CAP), ball(gen, 1, d, 1.0, CAP)])
    add("dist_bcast_3d", "distance", 0.7, [ball(gen, 3, d, 0.7, CAP).reshape(3, 1, d), ball(gen, 4, d, 0.7, CAP)])
    add("scalarmul_bcast_r", "mobius_scalar_mul", 1.0, [torch.tensor([[0.75]]), ball(gen, 7, d, 1.0, CAP)])
    add("scalarmul_bcast_3d", "mobius_scalar_mul", 2.0,
        [(torch.rand(3, 1, 1, generator=gen) * 2).float(), ball(gen, 4, d, 2.0, CAP)])
    add("scalarmul_bcast_x", "mobius_scalar_mul", 1.0, [(torch.rand(6, 1, generator=gen) * 2).float(), ball(gen, 1, d, 1.0, CAP)])
    add("logzero_3d", "log_map_zero", 1.0, [ball(gen, 6, 32, 1.0, CAP).reshape(2, 3, 32)])
    add("l2p_3d", "lorentz_to_poincare", 1.0, [L.project_to_hyperboloid(torch.randn(2, 3, d + 1, generator=gen) * 0.5, 1.0).detach()])

    # ---- ordinary cases at widths that are no multiple of 4: the 4-byte access form with all four slots of a lane in use,
    # 16 lanes per row (d = 50) and 32 lanes per row (d = 101); drawn last so that the cases above keep their values
    for op in PC.OPS:
        cap = OP_CAP.get(op, CAP)
        for dd in PC.ODD_DIMS:
            c = 0.7
            x = ball(gen, 3, dd, c, cap)
            if op in ("mobius_addition", "distance"):
                inputs = [x, apart(gen, x, c, cap)]
            elif op == "mobius_scalar_mul":
                inputs = [(torch.rand(3, 1, generator=gen) * 4 - 2).float(), x]
            elif op == "lorentz_to_poincare":
                inputs = [L.project_to_hyperboloid(torch.randn(3, dd + 1, generator=gen) * 0.5, c).detach()]
            else:
                inputs = [x]
            add(f"{op}_d{dd}_c{c}", op, c, inputs, ordinary=True, cap=cap)

    path = os.path.join(HERE, "g13_poincare.npz")
    np.savez_compressed(path, **arrays)
    assert os.path.getsize(path) < 1 << 20, os.path.getsize(path)
    with open(os.path.join(HERE, "g13_poincare.json"), "w") as f:
        json.dump({"e_ref_max": E_REF_MAX, "cap": CAP, "op_cap": OP_CAP, "cases": cases}, f, indent=1)
    worst = {}
    for c in cases:
        if c["ordinary"]:
            worst[c["op"]] = max(worst.get(c["op"], 0.0), c["e_ref"])
    print(f"{len(cases)} cases, {os.path.getsize(path)} bytes; worst ordinary e_ref per op: "
          + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    print("special cases:", ", ".join(f"{c['name']} e_ref={c['e_ref']:.2e}{'' if c['finite'] else ' (non-finite)'}"
                                     for c in cases if not c["ordinary"]))


if __name__ == "__main__":
    generate()
