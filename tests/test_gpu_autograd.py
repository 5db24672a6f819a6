"""Differentiable Lorentz primitives and the fused hyperbolic InfoNCE / triplet loss on the GPU, against the goldens
recorded from the reference (g11) and the float64 truth of tests/autograd_cases.py.

Bound of every gradient comparison (set by the feature's specification, not tuned): with e_ref the largest error of
the reference's own fp32 gradient against the float64 truth and e_hip ours, both relative to the largest |truth| of
the case, ``e_hip <= 4 * e_ref + 2**-20``; non-finite entries are compared by position and kind.  Each case prints
``name e_ref e_hip`` before it asserts (run with -s to collect the table of DESIGN.md 5.11).
"""
import json
import math
import os

import numpy as np
import pytest
import torch

import autograd_cases as AC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def LM():
    from hyptokenizer_amd.embedding import lorentz_model
    return lorentz_model


def CL():
    from hyptokenizer_amd.multimodal import contrastive_loss
    return contrastive_loss


def load(golden_dir, mode):
    meta = json.load(open(os.path.join(golden_dir, f"g11_autograd_{mode}.json")))
    return meta, dict(np.load(os.path.join(golden_dir, f"g11_autograd_{mode}.npz")))


def points(n, d, scale, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, d + 1, generator=g) * scale
    x[:, 0] = torch.sqrt(1.0 + (x[:, 1:] ** 2).sum(-1))
    return x


def run_ours(case, arrays, mode, dtype=torch.float32):
    """Forward + backward of one golden case through the public surface; returns (out, {name: grad})."""
    lm, cl = LM(), CL()
    names = AC.OPS[case["op"]][0]
    t = {k: torch.from_numpy(arrays[f"{case['name']}__{k}"]).to(DEV, dtype).requires_grad_() for k in names}
    p, op, kw = case["params"], case["op"], {"sign_convention": mode}
    if op == "minkowski":
        out = lm.minkowski_dot(t["x"], t["y"], **kw)
    elif op == "distance":
        out = lm.distance(t["x"], t["y"], p["c"], **kw)
    elif op == "log_map":
        out = lm.log_map(t["x"], t["y"], **kw)
    elif op == "exp_map":
        out = lm.exp_map(t["x"], t["y"])
    elif op == "project":
        out = lm.project_to_hyperboloid(t["x"], p["c"])
    elif op == "batch_distance":
        out = lm.batch_distance(t["x"], t["y"], p["c"], **kw)
    elif op == "batch_distance_optimized":
        out = lm.batch_distance_optimized(t["x"], t["y"], p["c"], **kw)
    elif op == "infonce":
        out = cl.hyperbolic_contrastive_loss(t["x"], t["y"], temp=p["temp"], reduction=p["reduction"], **kw)
    elif op == "triplet":
        out = cl.hyperbolic_triplet_loss(t["x"], t["y"], t["z"], margin=p["margin"], reduction=p["reduction"], **kw)
    else:
        raise ValueError(op)
    assert out.requires_grad
    g = torch.from_numpy(arrays[f"{case['name']}__g"]).to(DEV)
    out.backward(g.reshape(out.shape).to(out.dtype))
    return out.detach().cpu().numpy(), {k: t[k].grad.float().cpu().numpy() for k in names}


def check_bound(name, value, ref32, true64, e_ref_case=None):
    e_ref, ok_ref = AC.grad_error(ref32, ref32, true64)
    e_hip, ok = AC.grad_error(value, ref32, true64)
    print(f"{name} e_ref={e_ref:.3e} e_hip={e_hip:.3e}")
    assert ok, f"{name}: non-finite pattern differs from the reference's"
    assert e_hip <= AC.FACTOR * e_ref + AC.FLOOR, (name, e_ref, e_hip)
    return e_ref, e_hip


# ---- 1. fails without the feature: results carry a graph and backward fills .grad ---------------------------------
def test_results_require_grad_and_backward_fills_grad():
    lm = LM()
    x = points(16, 8, 0.5, 1).to(DEV)
    y = points(16, 8, 0.5, 2).to(DEV)
    v = (torch.randn(16, 9) * 0.3).to(DEV)
    kw = {"sign_convention": "lorentz"}
    calls = {
        "minkowski_dot": lambda a: lm.minkowski_dot(a, y, **kw),
        "distance": lambda a: lm.distance(a, y, **kw),
        "batch_distance": lambda a: lm.batch_distance(a, y, **kw),
        "batch_distance_optimized": lambda a: lm.batch_distance_optimized(a, y, **kw),
        "log_map": lambda a: lm.log_map(a, y, **kw),
        "exp_map": lambda a: lm.exp_map(a, v),
        "exp_map_v": lambda a: lm.exp_map(y, a),
        "project_to_hyperboloid": lambda a: lm.project_to_hyperboloid(a, 1.0),
        "minkowski_norm": lambda a: lm.minkowski_norm(a, sign_convention="reference"),
        "parallel_transport": lambda a: lm.parallel_transport(v, a, y, **kw),
        "riemannian_gradient": lambda a: lm.riemannian_gradient(v, a, **kw),
        "lorentz_to_klein": lambda a: lm.lorentz_to_klein(a),
    }
    for name, fn in calls.items():
        a = x.clone().requires_grad_()
        out = fn(a)
        assert out.requires_grad, name
        out.sum().backward()
        assert a.grad is not None and a.grad.shape == a.shape and bool(torch.isfinite(a.grad).all()), name
        assert bool((a.grad != 0).any()), name


def test_second_derivative_raises():
    lm = LM()
    x = points(4, 3, 0.5, 1).to(DEV).requires_grad_()
    y = points(4, 3, 0.5, 2).to(DEV)
    (gx,) = torch.autograd.grad(lm.distance(x, y, sign_convention="lorentz").sum(), x, create_graph=True)
    with pytest.raises(RuntimeError):
        gx.sum().backward()


def test_non_fp32_operands_get_gradients_in_their_dtype():
    lm = LM()
    x = points(8, 4, 0.5, 1).to(DEV).double().requires_grad_()
    y = points(8, 4, 0.5, 2).to(DEV).half()
    lm.distance(x, y, sign_convention="lorentz").sum().backward()
    assert x.grad.dtype == torch.float64


# ---- 2. forward unchanged -----------------------------------------------------------------------------------------
def test_forward_bits_and_entry_points_unchanged(monkeypatch):
    import hyptokenizer_amd.embedding.lorentz_model as lm
    from hyptokenizer_amd.embedding import _autograd
    x = points(300, 32, 0.5, 3).to(DEV)
    y = points(300, 32, 0.5, 4).to(DEV)
    v = (torch.randn(300, 33) * 0.3).to(DEV)
    kw = {"sign_convention": "lorentz"}
    fns = [lambda a, b: lm.minkowski_dot(a, b, **kw), lambda a, b: lm.distance(a, b, 0.7, **kw),
           lambda a, b: lm.batch_distance(a, b, **kw), lambda a, b: lm.batch_distance_optimized(a, b, **kw),
           lambda a, b: lm.log_map(a, b, **kw), lambda a, b: lm.exp_map(a, v), lambda a, b: lm.project_to_hyperboloid(a, 0.7)]
    plain = [f(x, y) for f in fns]
    for f, want in zip(fns, plain):
        assert not want.requires_grad
        got = f(x.clone().requires_grad_(), y)
        assert got.requires_grad
        assert torch.equal(got.detach().view(torch.int32), want.view(torch.int32))
    # without requires_grad (or under no_grad) the autograd layer is never entered: the same C entry point as before
    def boom(*a, **k):
        raise AssertionError("autograd path taken for a call that records no gradient")
    for name in ("pair_op", "project", "batch_distance"):
        monkeypatch.setattr(_autograd, name, boom)
    for f, want in zip(fns, plain):
        assert torch.equal(f(x, y).view(torch.int32), want.view(torch.int32))
        with torch.no_grad():
            assert torch.equal(f(x.clone().requires_grad_(), y).view(torch.int32), want.view(torch.int32))


# ---- 3. / 4. gradients against the goldens ----------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["reference", "lorentz"])
def test_gradients_against_goldens(golden_dir, mode):
    meta, arrays = load(golden_dir, mode)
    failures = []
    for case in meta["cases"]:
        _, true = AC.truth(case, arrays, mode)
        out, grads = run_ours(case, arrays, mode)
        ref_out = arrays[f"{case['name']}__out"]
        fin = np.isfinite(ref_out)
        assert np.array_equal(np.isnan(out), np.isnan(ref_out)), case["name"]
        assert np.allclose(out[fin], ref_out[fin], rtol=2e-5, atol=2e-6), case["name"]
        for key in AC.OPS[case["op"]][0]:
            try:
                check_bound(f"{mode}:{case['name']}:g{key}", grads[key], arrays[f"{case['name']}__g{key}"], true[key])
            except AssertionError as exc:
                failures.append(str(exc))
    assert not failures, "\n".join(failures)


def test_exact_cases(golden_dir):
    meta, arrays = load(golden_dir, "reference")
    for case in meta["cases"]:
        if case["op"] not in ("distance", "batch_distance", "batch_distance_optimized", "infonce", "triplet"):
            continue
        out, grads = run_ours(case, arrays, "reference")
        for key, g in grads.items():
            assert not g.any(), (case["name"], key)                        # exactly 0, not NaN
        if case["op"] == "infonce" and case["params"]["reduction"] == "mean":
            B = arrays[f"{case['name']}__x"].shape[0]
            assert abs(float(out) - math.log(B)) < 1e-5
            assert np.allclose(out, arrays[f"{case['name']}__out"], rtol=1e-6, atol=1e-6)
    meta, arrays = load(golden_dir, "lorentz")
    kinds = lambda a: np.where(np.isnan(a), 3, np.where(np.isposinf(a), 1, np.where(np.isneginf(a), 2, 0)))  # noqa: E731
    for case in meta["cases"]:
        if case["finite"]:
            continue
        _, grads = run_ours(case, arrays, "lorentz")
        for key, g in grads.items():
            assert np.array_equal(kinds(g), kinds(arrays[f"{case['name']}__g{key}"])), (case["name"], key)


# ---- 5. fused loss = composition ------------------------------------------------------------------------------------
@pytest.mark.parametrize("d1", [2, 65, 129])
def test_fused_loss_matches_composition(d1):
    lm, cl = LM(), CL()
    B, temp = 1000, 0.5
    if d1 == 2:          # 1000 points on a hyperbola: an even grid in arc length, positives half a step away
        t = torch.linspace(-2.0, 2.0, B, dtype=torch.float64)
        a = torch.stack([torch.cosh(t), torch.sinh(t)], -1).float()
        b = torch.stack([torch.cosh(t + 0.002), torch.sinh(t + 0.002)], -1).float()
    else:
        a = points(B, d1 - 1, 1.0 / math.sqrt(d1 - 1), 10 + d1)
        b = a + torch.randn(B, d1, generator=torch.Generator().manual_seed(d1)) * 0.5 / math.sqrt(d1 - 1)
        b[:, 0] = torch.sqrt(1.0 + (b[:, 1:] ** 2).sum(-1))
    res = {}
    for which in ("fused", "composed"):
        zt, zi = a.to(DEV).requires_grad_(), b.to(DEV).requires_grad_()
        if which == "fused":
            loss = cl.hyperbolic_contrastive_loss(zt, zi, temp=temp, sign_convention="lorentz")
        else:
            s = -lm.batch_distance(zt, zi, 1.0, sign_convention="lorentz") / temp
            labels = torch.arange(B, device=DEV)
            ce = torch.nn.functional.cross_entropy
            loss = (ce(s, labels) + ce(s.t(), labels)) / 2.0
        loss.backward()
        res[which] = (float(loss.detach()), zt.grad.cpu().numpy(), zi.grad.cpu().numpy())
    t64 = {"x": a.double().requires_grad_(), "y": b.double().requires_grad_()}
    true_loss = AC.infonce(t64["x"], t64["y"], temp, "mean", -1.0)
    true_loss.backward()
    tl = float(true_loss.detach())
    assert 0.05 < tl < math.log(B)
    assert abs(res["fused"][0] - tl) <= 4 * abs(res["composed"][0] - tl) + 2.0 ** -20 * tl
    for k, key in ((1, "x"), (2, "y")):
        check_bound(f"fused_vs_composed:d1={d1}:g{key}", res["fused"][k], res["composed"][k], t64[key].grad.numpy())


# ---- 6. determinism ---------------------------------------------------------------------------------------------
def test_backward_is_deterministic():
    lm, cl = LM(), CL()
    a, b = points(700, 64, 0.125, 5).to(DEV), points(700, 64, 0.125, 6).to(DEV)
    runs = []
    for _ in range(2):
        zt, zi = a.clone().requires_grad_(), b.clone().requires_grad_()
        cl.hyperbolic_contrastive_loss(zt, zi, temp=0.5, sign_convention="lorentz").backward()
        x, y = a.clone().requires_grad_(), b.clone().requires_grad_()
        lm.batch_distance(x, y, sign_convention="lorentz").square().sum().backward()
        runs.append([t.grad.view(torch.int32).clone() for t in (zt, zi, x, y)])
    for g0, g1 in zip(*runs):
        assert torch.equal(g0, g1)
        assert bool((g0 != 0).any())


# ---- 7. memory ------------------------------------------------------------------------------------------------------
def test_fused_loss_memory_is_linear_in_batch():
    cl = CL()
    B, d1 = 8192, 65
    zt = points(B, d1 - 1, 0.125, 7).to(DEV).requires_grad_()
    zi = points(B, d1 - 1, 0.125, 8).to(DEV).requires_grad_()
    cl.hyperbolic_contrastive_loss(zt[:64], zi[:64], sign_convention="lorentz").backward()      # warm-up
    zt.grad = zi.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    loss = cl.hyperbolic_contrastive_loss(zt, zi, temp=0.5, sign_convention="lorentz")
    loss.backward()
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base
    print(f"peak extra bytes {extra} (limit {16 * B * d1 * 4}, one B x B fp32 matrix {B * B * 4})")
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(zt.grad).all())
    assert extra < 16 * B * d1 * 4


# ---- 8. training smoke test -------------------------------------------------------------------------------------------
def test_sgd_lowers_the_fused_loss():
    lm, cl = LM(), CL()
    n, d = 256, 16
    g = torch.Generator().manual_seed(11)
    zt = lm.project_to_hyperboloid((torch.randn(n, d + 1, generator=g) * 0.5).to(DEV)).requires_grad_()
    zi = lm.project_to_hyperboloid((torch.randn(n, d + 1, generator=g) * 0.5).to(DEV)).requires_grad_()
    losses = []
    for _ in range(50):
        loss = cl.hyperbolic_contrastive_loss(zt, zi, temp=0.5, sign_convention="lorentz")
        loss.backward()
        with torch.no_grad():
            for z in (zt, zi):
                z.copy_(lm.project_to_hyperboloid(z - 0.5 * z.grad))
                z.grad = None
        losses.append(float(loss.detach()))
    print("losses", losses[:3], "...", losses[-3:])
    assert sum(losses[-10:]) / 10 < sum(losses[:10]) / 10
    assert bool(torch.isfinite(zt).all()) and bool(torch.isfinite(zi).all())
