#!/usr/bin/env python
"""Generate tests/golden/g11_autograd_{reference,lorentz}.{npz,json} by running the REFERENCE's
``embedding/lorentz_model.py`` and ``multimodal/contrastive_loss.py`` under torch autograd on the CPU.

Like make_golden.py it runs only where the reference is present (it is imported, never copied) and applies the same
sign patch:
  reference : the modules exactly as shipped (every distance is 0.0, every distance gradient exactly 0)
  lorentz   : ``minkowski_dot`` negated and ``batch_distance`` invoked as ``orig(x, -y, c)``
``multimodal/contrastive_loss.py`` cannot be imported as shipped (its package-relative import of ``distance`` has no
parent package): its source is read at generation time, that one import is pointed at the already
imported ``embedding.lorentz_model``, and the module is executed from memory.

Per mode the npz holds, for every case ``<name>``: the fp32 inputs ``<name>__x`` (``__y``, ``__z``), the upstream
gradient ``<name>__g``, the reference's fp32 forward value ``<name>__out`` and its fp32 gradients ``<name>__gx``
(``__gy``, ``__gz``).  The json lists the cases (op, parameters, whether it is an ordinary table) with the measured
error ``e_ref`` of the reference's fp32 gradients against the float64 truth of tests/autograd_cases.py and, for the
losses, the recorded loss and the range it was required to lie in.

Ordinary tables: d in {1, 5, 32, 100, 128}, b up to 512, B in {2, 7, 64, 256}, sized so that each npz
stays below 1 MiB, row pairs at least 0.1 (all-pairs tables 0.02) above u = 1; the loss inputs are pairs at spatial
scale 1.0 with noise 0.5 and the temperature is raised from 0.07 until the loss lies strictly between 0.05 and log B
(at scale 0.3 and temp 0.07 it collapses to 1e-6 and tests nothing).  Special cases: clamped pairs, identical points,
masked log_map / exp_map branches, broadcast operands, all three reductions, non-uniform upstream gradients.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_autograd.py [reference|lorentz|all]
"""
from __future__ import annotations

import json
import math
import os
import sys
import types
import warnings

REF = "/root/reference"
if not os.path.isdir(REF):
    sys.exit("make_golden_autograd.py: /root/reference is not present; golden vectors can only be regenerated "
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

import autograd_cases as AC  # noqa: E402  (ours: float64 truth and the error measure)

_ORIG = {"minkowski_dot": L.minkowski_dot, "batch_distance": L.batch_distance}
LOSS_LO = 0.05
TEMPS = (0.07, 0.2, 0.5, 1.0, 2.0, 5.0)
E_REF_MAX = 1e-4


def set_mode(mode: str) -> None:
    """Install / remove the two sign patches (make_golden.py set_mode)."""
    if mode == "reference":
        L.minkowski_dot = _ORIG["minkowski_dot"]
        L.batch_distance = _ORIG["batch_distance"]
    elif mode == "lorentz":
        L.minkowski_dot = lambda a, b: -_ORIG["minkowski_dot"](a, b)
        L.batch_distance = lambda x, y, c=1.0: _ORIG["batch_distance"](x, -y, c)
    else:
        raise ValueError(mode)


def load_losses():
    """The reference's loss module, executed from its source with the broken relative import redirected."""
    path = os.path.join(REF, "multimodal", "contrastive_loss.py")
    src = open(path).read()
    rel = "from ..embedding.lorentz_model import distance"
    assert rel in src
    mod = types.ModuleType("reference_contrastive_loss")
    exec(compile(src.replace(rel, "from embedding.lorentz_model import distance"), path, "exec"), mod.__dict__)
    return mod


def pts(gen, n, d, scale):
    """n points on the unit hyperboloid with spatial part N(0, scale^2)."""
    return L.project_to_hyperboloid(torch.randn(n, d + 1, generator=gen) * scale, 1.0).detach()


def apart(gen, x, n, d, scale, margin):
    """n points like ``pts`` whose Lorentz u against every row of x (row-wise when n == len(x) and margin > 0.05) exceeds
    1 + margin: pairs closer than that make d acosh/du ill-conditioned in fp32, which measures the inputs, not the code."""
    rowwise = margin > 0.05
    y = pts(gen, n, d, scale)
    for _ in range(200):
        if rowwise:
            u = x[:, 0] * y[:, 0] - (x[:, 1:] * y[:, 1:]).sum(-1)
        else:
            u = (x[:, None, 0] * y[None, :, 0] - (x[:, None, 1:] * y[None, :, 1:]).sum(-1)).min(0).values
        bad = u < 1.0 + margin
        if not bool(bad.any()):
            return y
        y[bad] = pts(gen, int(bad.sum()), d, scale)
    raise AssertionError("could not separate the points")


def origin(d):
    o = torch.zeros(1, d + 1)
    o[0, 0] = 1.0
    return o


def run_case(CL, mode, op, params, inputs, g=None):
    """Run the reference on fp32 inputs; returns (out, grads, g)."""
    leaves = [t.clone().float().requires_grad_() for t in inputs]
    c = params.get("c", 1.0)
    if op == "minkowski":
        out = L.minkowski_dot(*leaves)
    elif op == "distance":
        out = L.distance(*leaves, c=c)
    elif op == "log_map":
        out = L.log_map(*leaves)
    elif op == "exp_map":
        out = L.exp_map(*leaves)
    elif op == "project":
        out = L.project_to_hyperboloid(leaves[0], c)
    elif op == "batch_distance":
        out = L.batch_distance(*leaves, c)
    elif op == "batch_distance_optimized":
        # the einsum form has no patched twin: under "lorentz" it is fed -y like batch_distance (make_golden.py)
        out = L.batch_distance_optimized(leaves[0], leaves[1] if mode == "reference" else -leaves[1], c)
    elif op == "infonce":
        out = CL.hyperbolic_contrastive_loss(*leaves, temp=params["temp"], reduction=params["reduction"])
    elif op == "triplet":
        out = CL.hyperbolic_triplet_loss(*leaves, margin=params["margin"], reduction=params["reduction"])
    else:
        raise ValueError(op)
    if g is None:
        g = torch.ones_like(out)
    out.backward(g)
    return out.detach(), [t.grad if t.grad is not None else torch.zeros_like(t) for t in leaves], g


def generate(mode: str) -> None:
    set_mode(mode)
    CL = load_losses()
    gen = torch.Generator().manual_seed(20240611)
    arrays, cases = {}, []

    def add(name, op, params, inputs, g=None, ordinary=False, g_random=True):
        if g is None and g_random:
            shape = run_case(CL, mode, op, params, inputs)[0].shape
            g = torch.randn(shape, generator=gen) if len(shape) else torch.tensor(1.0)
        out, grads, g = run_case(CL, mode, op, params, inputs, g)
        case = {"name": name, "op": op, "params": params, "ordinary": bool(ordinary)}
        for key, t in zip("xyz", inputs):
            arrays[f"{name}__{key}"] = t.float().numpy()
        arrays[f"{name}__g"] = g.numpy()
        arrays[f"{name}__out"] = out.numpy()
        for key, t in zip("xyz", grads):
            arrays[f"{name}__g{key}"] = t.numpy()
        _, true = AC.truth(case, arrays, mode)
        errs = {}
        for key in AC.OPS[op][0]:
            e, ok = AC.grad_error(arrays[f"{name}__g{key}"], arrays[f"{name}__g{key}"], true[key])
            assert ok
            errs[key] = e
        case["e_ref"] = max(errs.values())
        case["finite"] = bool(all(np.isfinite(arrays[f"{name}__g{k}"]).all() for k in AC.OPS[op][0]))
        if ordinary:
            assert case["e_ref"] <= E_REF_MAX, (name, case["e_ref"])
            # the reference stays finite on ordinary tables (log_map under "reference" is NaN by construction: u <= -1)
            assert case["finite"] or (mode == "reference" and op == "log_map"), name
        cases.append(case)
        return case, out

    # ---- ordinary tables: primitives --------------------------------------------------------------------------
    for d, b in ((1, 64), (5, 128), (32, 24), (100, 8), (128, 8)):
        x = pts(gen, b, d, 0.5)
        y = apart(gen, x, b, d, 0.5, 0.1)
        add(f"mink_d{d}", "minkowski", {}, [x, y], ordinary=True)
        if d == 5:
            xl = pts(gen, 512, d, 0.5)
            add(f"dist_d{d}", "distance", {"c": 0.5}, [xl, apart(gen, xl, 512, d, 0.5, 0.1)], ordinary=True)
        else:
            add(f"dist_d{d}", "distance", {"c": 1.0}, [x, y], ordinary=True)
        add(f"logmap_d{d}", "log_map", {}, [x, y], ordinary=True)
        add(f"expmap_d{d}", "exp_map", {}, [x, torch.randn(b, d + 1, generator=gen) * 0.3], ordinary=True)
        add(f"project_d{d}", "project", {"c": 1.0 if d != 32 else 0.7}, [torch.randn(b, d + 1, generator=gen)], ordinary=True)
    for d, n1, n2 in ((1, 7, 5), (5, 40, 70), (32, 30, 64), (128, 10, 66)):
        x = pts(gen, n1, d, 1.0 if d == 1 else 0.5)
        add(f"bdist_d{d}", "batch_distance", {"c": 1.0 if d != 32 else 2.0}, [x, apart(gen, x, n2, d, 1.0 if d == 1 else 0.5, 0.02)],
            ordinary=True)
    x = pts(gen, 9, 32, 0.5)
    add("bdistopt_d32", "batch_distance_optimized", {"c": 1.0}, [x, apart(gen, x, 20, 32, 0.5, 0.02)], ordinary=True)

    # ---- ordinary tables: losses (range asserted) ---------------------------------------------------------------
    for B, d in ((2, 100), (7, 1), (64, 32), (256, 5), (16, 128)):
        a = pts(gen, B, d, 1.0)
        b2 = L.project_to_hyperboloid(a + torch.randn(B, d + 1, generator=gen) * 0.5, 1.0).detach()
        for _ in range(200):                                              # no pair of the B x B table closer than u = 1.02
            bad = (a[:, None, 0] * b2[None, :, 0] - (a[:, None, 1:] * b2[None, :, 1:]).sum(-1)).min(0).values < 1.02
            if not bool(bad.any()):
                break
            b2[bad] = L.project_to_hyperboloid(a[bad] + torch.randn(int(bad.sum()), d + 1, generator=gen) * 0.5, 1.0).detach()
        else:
            raise AssertionError("could not separate the pairs")
        hi = math.log(B)
        for temp in TEMPS:
            with torch.no_grad():
                loss = float(CL.hyperbolic_contrastive_loss(a, b2, temp=temp))
            if mode == "reference" or LOSS_LO < loss < hi:
                break
        else:
            raise AssertionError(f"no temperature puts the loss of B={B}, d={d} into ({LOSS_LO}, log B)")
        for red in ("mean", "sum", "none"):
            if (red == "none" and B not in (7, 64)) or (red == "sum" and B != 7):
                continue
            case, out = add(f"nce_B{B}_d{d}_{red}", "infonce", {"temp": temp, "reduction": red}, [a, b2], ordinary=True)
            if red == "mean":
                case["loss"] = float(out)
                # under "reference" every distance is 0 and the loss is log B itself: the closed range
                case["loss_range"] = [LOSS_LO, hi]
                assert (LOSS_LO < case["loss"] < hi) if mode == "lorentz" else abs(case["loss"] - hi) < 1e-5, (B, d, case["loss"])
        neg = pts(gen, B, d, 1.0)
        for red in ("mean", "sum", "none"):
            if (red == "none" and B not in (7, 64)) or (red == "sum" and B != 7):
                continue
            add(f"trip_B{B}_d{d}_{red}", "triplet", {"margin": 1.0, "reduction": red}, [a, b2, neg], ordinary=True)

    # ---- special cases ----------------------------------------------------------------------------------------------------
    d = 5
    off = torch.randn(16, d + 1, generator=gen) * 0.4                    # rows off the hyperboloid: u < 1 under "lorentz" for most
    on = pts(gen, 16, d, 0.5)
    add("dist_clamped", "distance", {"c": 1.0}, [torch.cat([off, on]), torch.cat([off.flip(0), on.flip(0)])])
    same = torch.cat([origin(d), pts(gen, 7, d, 0.5)])
    add("dist_identical", "distance", {"c": 1.0}, [same, same.clone()])
    add("dist_identical_ones", "distance", {"c": 1.0}, [same, same.clone()], g=torch.ones(8))
    add("logmap_identical", "log_map", {}, [torch.cat([same, on[:4]]), torch.cat([same, on[4:8]])])
    add("bdist_identical", "batch_distance", {"c": 1.0}, [same, same.clone()])
    add("dist_bcast_row", "distance", {"c": 1.0}, [pts(gen, 1, d, 0.5), pts(gen, 9, d, 0.5)])
    add("dist_bcast_3d", "distance", {"c": 0.5}, [pts(gen, 3, d, 0.5).reshape(3, 1, d + 1), pts(gen, 4, d, 0.5)])
    add("logmap_bcast", "log_map", {}, [pts(gen, 1, d, 0.5), pts(gen, 6, d, 0.5)])
    add("expmap_bcast", "exp_map", {}, [pts(gen, 5, d, 0.5), torch.randn(1, d + 1, generator=gen) * 0.3])
    add("mink_bcast", "minkowski", {}, [pts(gen, 2, d, 0.5).reshape(2, 1, d + 1), pts(gen, 3, d, 0.5)])
    v = torch.randn(8, d + 1, generator=gen) * 0.3
    v[0] = 0.0                                                            # zero tangent: clamp(min=1e-8) active
    v[1, 1:] = 2e-5                                                       # squared norm 2e-9 < 1e-8: clamp active
    v[2, 1:] = 1e-3                                                       # small but above the clamp
    add("expmap_small", "exp_map", {}, [pts(gen, 8, d, 0.5), v])
    z = torch.randn(6, d + 1, generator=gen)
    z[0, 1:] = 0.0                                                        # zero spatial part: norm backward gives 0
    add("project_zero_row", "project", {"c": 1.0}, [z])
    a = pts(gen, 7, d, 1.0)
    b2 = L.project_to_hyperboloid(a + torch.randn(7, d + 1, generator=gen) * 0.5, 1.0).detach()
    add("nce_weighted_none", "infonce", {"temp": 0.5, "reduction": "none"}, [a, b2], g=torch.rand(7, generator=gen) + 0.1)
    same4 = pts(gen, 4, 4, 0.3)
    add("nce_identical", "infonce", {"temp": 0.07, "reduction": "mean"}, [same4, same4.clone()], g_random=False)
    withorigin = torch.cat([origin(4), same4])
    add("nce_identical_origin", "infonce", {"temp": 0.07, "reduction": "mean"}, [withorigin, withorigin.clone()], g_random=False)
    add("trip_inactive", "triplet", {"margin": -50.0, "reduction": "sum"}, [a, b2, pts(gen, 7, d, 1.0)])
    add("trip_relu_zero", "triplet", {"margin": 0.0, "reduction": "none"}, [a, b2, b2.clone()])
    add("trip_identical", "triplet", {"margin": 1.0, "reduction": "mean"}, [withorigin, withorigin.clone(), pts(gen, 5, 4, 0.5)],
        g_random=False)

    np.savez_compressed(os.path.join(HERE, f"g11_autograd_{mode}.npz"), **arrays)
    with open(os.path.join(HERE, f"g11_autograd_{mode}.json"), "w") as f:
        json.dump({"mode": mode, "loss_lo": LOSS_LO, "e_ref_max": E_REF_MAX, "cases": cases}, f, indent=1)
    worst = max((c["e_ref"] for c in cases if c["ordinary"]), default=0.0)
    print(f"{mode}: {len(cases)} cases, worst ordinary e_ref {worst:.3g}, "
          f"non-finite cases: {[c['name'] for c in cases if not c['finite']]}")


if __name__ == "__main__":
    which = sys.argv[1] if len(sys.argv) > 1 else "all"
    for m in (("reference", "lorentz") if which == "all" else (which,)):
        generate(m)
