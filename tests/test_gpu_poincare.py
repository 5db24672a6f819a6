"""Differentiable Poincare-ball primitives on the GPU, against the goldens recorded from the reference (g13) and the
float64 truth of tests/poincare_cases.py.

Bound of every comparison (the rule of test_gpu_autograd.py, set by the feature's specification, not tuned): with e_ref the
error of the reference's own fp32 value against the float64 truth and e_hip ours, both relative to the largest |truth| of
the array, ``e_hip <= 4 * e_ref + 2**-20``; non-finite entries are compared by position and kind.  Each case prints
``name e_ref e_hip`` before it asserts (run with -s to collect the table of DESIGN.md 5.13).  Where no golden exists
(the standard conversion, whole tables) the place of the reference is taken by the same expression evaluated by torch in
fp32 on the same device, measured in the test.
"""
import json
import os

import numpy as np
import pytest
import torch

import autograd_cases as AC
import poincare_cases as PC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def PB():
    from hyptokenizer_amd.embedding import poincare_ball
    return poincare_ball


def load(golden_dir):
    meta = json.load(open(os.path.join(golden_dir, "g13_poincare.json")))
    return meta, dict(np.load(os.path.join(golden_dir, "g13_poincare.npz")))


def ball(n, d, c, seed, cap=0.9, lo=0.05):
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(n, d, generator=g)
    v = v / v.norm(dim=-1, keepdim=True)
    return (v * (lo + (cap - lo) * torch.rand(n, 1, generator=g)) / np.sqrt(c)).float()


def run_ours(case, arrays, c=None, dtype=torch.float32):
    """Forward + backward of one golden case through the public surface; returns {quantity: array}."""
    pb = PB()
    names = PC.OPS[case["op"]][0]
    t = {k: torch.from_numpy(arrays[f"{case['name']}__{k}"]).to(DEV, dtype).requires_grad_() for k in names}
    fn = getattr(pb, case["op"])
    args = [t[k] for k in names]
    out = fn(*args) if case["op"] == "norm" else fn(*args, case["c"] if c is None else c)
    assert out.requires_grad
    g = torch.from_numpy(arrays[f"{case['name']}__g"]).to(DEV)
    out.backward(g.reshape(out.shape).to(out.dtype))
    res = {"out": out.detach().float().cpu().numpy()}
    for k in names:
        assert t[k].grad is not None and t[k].grad.shape == t[k].shape and t[k].grad.dtype == dtype, (case["name"], k)
        res[f"g{k}"] = t[k].grad.float().cpu().numpy()
    return res


def rel_err(value, true64):
    """Largest |value - truth| relative to the largest |truth| (float64 tensors on the device)."""
    return float((value.double() - true64).abs().max() / true64.abs().max())


# ---- 1. every golden case: forward values and every gradient ------------------------------------------------------------
def test_values_and_gradients_against_goldens(golden_dir):
    meta, arrays = load(golden_dir)
    failures = []
    for case in meta["cases"]:
        ours = run_ours(case, arrays)
        assert ours["out"].shape == arrays[f"{case['name']}__out"].shape, case["name"]
        e_ref = PC.errors(case, arrays)
        e_hip = PC.errors(case, arrays, ours)
        for q in PC.quantities(case):
            print(f"{case['name']}:{q} e_ref={e_ref[q][0]:.3e} e_hip={e_hip[q][0]:.3e}")
            if not e_hip[q][1]:
                failures.append(f"{case['name']}:{q}: non-finite pattern differs from the reference's")
            elif not e_hip[q][0] <= PC.FACTOR * e_ref[q][0] + PC.FLOOR:
                failures.append(f"{case['name']}:{q}: e_ref={e_ref[q][0]:.3e} e_hip={e_hip[q][0]:.3e}")
    assert not failures, "\n".join(failures)


# ---- 2. autograd plumbing ---------------------------------------------------------------------------------------------
def test_results_carry_a_graph_and_backward_fills_grad():
    pb = PB()
    x, y = ball(16, 8, 1.0, 1).to(DEV), ball(16, 8, 1.0, 2).to(DEV)
    r = (torch.rand(16, 1) + 0.5).to(DEV)
    z = torch.randn(16, 9).to(DEV)
    z[:, 0] = torch.sqrt(1 + (z[:, 1:] ** 2).sum(-1))
    calls = {
        "norm": (x, lambda a: pb.norm(a)),
        "mobius_addition": (x, lambda a: pb.mobius_addition(a, y)),
        "mobius_addition_y": (x, lambda a: pb.mobius_addition(y, a, 0.7)),
        "mobius_scalar_mul_r": (r, lambda a: pb.mobius_scalar_mul(a, x)),
        "mobius_scalar_mul_x": (x, lambda a: pb.mobius_scalar_mul(r, a, torch.tensor(0.7))),
        "exp_map_zero": (x, lambda a: pb.exp_map_zero(a)),
        "log_map_zero": (x, lambda a: pb.log_map_zero(a)),
        "distance": (x, lambda a: pb.distance(a, y)),
        "lorentz_to_poincare": (z, lambda a: pb.lorentz_to_poincare(a)),
        "poincare_to_lorentz": (x, lambda a: pb.poincare_to_lorentz(a)),
        "poincare_to_lorentz_standard": (x, lambda a: pb.poincare_to_lorentz(a, 0.7, conversion="standard")),
    }
    for name, (src, fn) in calls.items():
        assert not fn(src).requires_grad, name
        a = src.clone().requires_grad_()
        with torch.no_grad():
            assert not fn(a).requires_grad, name
        out = fn(a)
        assert out.requires_grad and out.dtype == torch.float32, name
        out.sum().backward()
        assert a.grad is not None and a.grad.shape == a.shape and bool(torch.isfinite(a.grad).all()), name
        assert bool((a.grad != 0).any()), name
    assert pb.distance(x, y).shape == (16, 1) and pb.norm(x).shape == (16, 1)
    assert pb.poincare_to_lorentz(x).shape == (16, 9) and pb.lorentz_to_poincare(z).shape == (16, 8)


def test_second_derivative_raises():
    pb = PB()
    x = ball(4, 3, 1.0, 1).to(DEV).requires_grad_()
    (gx,) = torch.autograd.grad(pb.log_map_zero(x).sum(), x, create_graph=True)
    with pytest.raises(RuntimeError):
        gx.sum().backward()


def test_non_fp32_operands_get_gradients_in_their_dtype(golden_dir):
    pb = PB()
    x = ball(8, 4, 1.0, 1).to(DEV).double().requires_grad_()
    y = ball(8, 4, 1.0, 2).to(DEV).half()
    pb.distance(x, y).sum().backward()
    assert x.grad.dtype == torch.float64
    r = torch.full((8, 1), 0.5, device=DEV, dtype=torch.bfloat16, requires_grad=True)
    pb.mobius_scalar_mul(r, x).sum().backward()
    assert r.grad.dtype == torch.bfloat16 and r.grad.shape == (8, 1)
    # fp64 operands are computed in fp32: the golden bound holds for them as well
    meta, arrays = load(golden_dir)
    case = next(c for c in meta["cases"] if c["name"] == "log_map_zero_d32_c0.7")
    e_ref, e_hip = PC.errors(case, arrays), PC.errors(case, arrays, run_ours(case, arrays, dtype=torch.float64))
    for q in PC.quantities(case):
        assert e_hip[q][1] and e_hip[q][0] <= PC.FACTOR * e_ref[q][0] + PC.FLOOR, (q, e_ref[q], e_hip[q])


def test_float_and_tensor_curvature_give_identical_bits(golden_dir):
    meta, arrays = load(golden_dir)
    seen = set()
    for case in meta["cases"]:
        if case["op"] == "norm" or (case["op"], case["c"]) in seen or not case["ordinary"]:
            continue
        seen.add((case["op"], case["c"]))
        a = run_ours(case, arrays, c=case["c"])
        for c in (torch.tensor(case["c"]), torch.tensor([case["c"]], device=DEV), torch.tensor(case["c"], requires_grad=True)):
            b = run_ours(case, arrays, c=c)
            for q in a:
                assert np.array_equal(a[q].view(np.uint32), b[q].view(np.uint32)), (case["name"], q)
            assert not isinstance(c, torch.Tensor) or c.grad is None
    assert len(seen) == 7 * 3


def test_broadcast_gradients_have_the_operands_shape():
    pb = PB()
    row, many = ball(1, 5, 1.0, 1).to(DEV).requires_grad_(), ball(9, 5, 1.0, 2).to(DEV).requires_grad_()
    pb.distance(row, many).sum().backward()
    assert row.grad.shape == (1, 5) and many.grad.shape == (9, 5)
    ref = torch.zeros(1, 5, device=DEV)
    for k in range(9):                                                    # the broadcast operand's gradient is the sum over the rows
        a = row.detach().clone().requires_grad_()
        pb.distance(a, many.detach()[k:k + 1]).sum().backward()
        ref += a.grad
    assert torch.allclose(row.grad, ref, rtol=1e-5, atol=1e-6)
    a3, b2 = ball(3, 5, 2.0, 3).reshape(3, 1, 5).to(DEV).requires_grad_(), ball(4, 5, 2.0, 4).to(DEV).requires_grad_()
    out = pb.mobius_addition(a3, b2, 2.0)
    assert out.shape == (3, 4, 5)
    out.sum().backward()
    assert a3.grad.shape == (3, 1, 5) and b2.grad.shape == (4, 5)
    r0 = torch.tensor(0.75, device=DEV, requires_grad=True)               # a 0-d factor against many rows
    r3 = torch.rand(3, 1, 1, device=DEV).requires_grad_()
    x = ball(4, 5, 1.0, 5).to(DEV).requires_grad_()
    assert pb.mobius_scalar_mul(r0, x).shape == (4, 5)
    out = pb.mobius_scalar_mul(r3, x)
    assert out.shape == (3, 4, 5)
    (out.sum() + pb.mobius_scalar_mul(r0, x).sum()).backward()
    assert r0.grad.shape == () and r3.grad.shape == (3, 1, 1) and x.grad.shape == (4, 5)
    empty = torch.zeros(0, 5, device=DEV, requires_grad=True)
    out = pb.log_map_zero(empty)
    out.sum().backward()
    assert out.shape == (0, 5) and empty.grad.shape == (0, 5)
    with pytest.raises(ValueError):
        pb.log_map_zero(torch.zeros(2, 129, device=DEV))


# ---- 3. the two conversions -------------------------------------------------------------------------------------------
def test_reference_conversion_is_reproduced_as_shipped(golden_dir):
    pb = PB()
    meta, arrays = load(golden_dir)
    for case in meta["cases"]:
        if case["op"] != "poincare_to_lorentz" or not case["ordinary"]:
            continue
        x = torch.from_numpy(arrays[f"{case['name']}__x"]).to(DEV)
        assert np.allclose(pb.poincare_to_lorentz(x, case["c"]).cpu().numpy(), arrays[f"{case['name']}__out"], rtol=1e-5, atol=1e-6)
        img = pb.poincare_to_lorentz(x, case["c"], conversion="reference").double()
        form = img[:, 0] ** 2 - (img[:, 1:] ** 2).sum(-1)
        assert torch.allclose(form, torch.full_like(form, 1 / (4 * case["c"])), rtol=1e-3)          # a quarter of 1 / c: as shipped
    p = ball(64, 5, 1.0, 7, lo=0.35, cap=0.45).to(DEV)
    back = pb.lorentz_to_poincare(pb.poincare_to_lorentz(p))
    assert float((back - p).abs().max()) > 0.05                            # and lorentz_to_poincare does not invert it


@pytest.mark.parametrize("c", PC.CURVATURES)
def test_standard_conversion_lands_on_the_hyperboloid(c):
    pb = PB()
    p = ball(4096, 32, c, 11).to(DEV)
    want = 1.0 / float(np.float32(c))

    def form_error(img):
        img = img.double()
        return float(((img[:, 0] ** 2 - (img[:, 1:] ** 2).sum(-1)) - want).abs().max() / want)

    e_torch = form_error(PC.poincare_to_lorentz_standard(p, c))
    e_hip = form_error(pb.poincare_to_lorentz(p, c, conversion="standard"))
    print(f"standard_form c={c} e_torch={e_torch:.3e} e_hip={e_hip:.3e}")
    assert e_hip <= 4 * e_torch + 2.0 ** -20


def test_standard_conversion_is_inverted_and_is_an_isometry_at_c1():
    pb = PB()
    from hyptokenizer_amd.embedding import lorentz_model as lm
    p, q = ball(4096, 32, 1.0, 12).to(DEV), ball(4096, 32, 1.0, 13).to(DEV)
    scale = float(p.abs().max())
    e_torch = float((PC.lorentz_to_poincare(PC.poincare_to_lorentz_standard(p, 1.0), 1.0) - p).abs().max()) / scale
    e_hip = float((pb.lorentz_to_poincare(pb.poincare_to_lorentz(p, conversion="standard")) - p).abs().max()) / scale
    print(f"standard_roundtrip e_torch={e_torch:.3e} e_hip={e_hip:.3e}")
    assert e_hip <= 4 * e_torch + 2.0 ** -20
    # Lorentz distance of the images == Poincare distance of the points
    d_ball64 = PC.distance(p.double(), q.double(), 1.0).squeeze(-1)
    scale = float(d_ball64.abs().max())
    t_l = AC.dist(PC.poincare_to_lorentz_standard(p, 1.0), PC.poincare_to_lorentz_standard(q, 1.0), 1.0, AC.SIGN["lorentz"])
    t_b = PC.distance(p, q, 1.0).squeeze(-1)
    e_torch = float((t_l - t_b).abs().max()) / scale
    h_l = lm.distance(pb.poincare_to_lorentz(p, conversion="standard"), pb.poincare_to_lorentz(q, conversion="standard"),
                      sign_convention="lorentz")
    h_b = pb.distance(p, q).squeeze(-1)
    e_hip = float((h_l - h_b).abs().max()) / scale
    print(f"standard_isometry e_torch={e_torch:.3e} e_hip={e_hip:.3e}")
    assert h_l.shape == h_b.shape == (4096,)
    assert e_hip <= 4 * e_torch + 2.0 ** -20
    assert float((h_b.double() - d_ball64).abs().max()) / scale <= 4 * float((t_b.double() - d_ball64).abs().max()) / scale + 2.0 ** -20


# ---- 4. whole tables ------------------------------------------------------------------------------------------------------
def _peak_of(fn):
    """(result, peak bytes allocated above what was live before the call)."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    return out, torch.cuda.max_memory_allocated() - base


@pytest.mark.parametrize("rows,d1", [(50000, 101), (1 << 20, 65)])
def test_whole_table_to_euclidean_features(rows, d1):
    """``log_map_zero(lorentz_to_poincare(table))`` (what the reference's training script does to the trained table): agrees
    with the torch-composed fp32 expression under the golden bound, and each of the two calls, measured on its own,
    allocates its result -- one allocator block -- and nothing else."""
    pb = PB()
    g = torch.Generator(device=DEV).manual_seed(rows)
    table = torch.randn(rows, d1, device=DEV, generator=g) * (1.0 / np.sqrt(d1 - 1))
    table[:, 0] = torch.sqrt(1.0 + (table[:, 1:] ** 2).sum(-1))
    pb.log_map_zero(pb.lorentz_to_poincare(table[:64]))                   # warm-up
    block = 2 << 20                                                        # torch's caching allocator hands out blocks above 1 MiB in multiples of 2 MiB
    one_result = -(-rows * (d1 - 1) * 4 // block) * block
    ball_table, extra_l2p = _peak_of(lambda: pb.lorentz_to_poincare(table))
    feats, extra_log = _peak_of(lambda: pb.log_map_zero(ball_table))
    composed, extra_torch = _peak_of(lambda: PC.log_map_zero(PC.lorentz_to_poincare(table, 1.0), 1.0))
    true64 = PC.log_map_zero(PC.lorentz_to_poincare(table.double(), 1.0), 1.0)
    e_torch, e_hip = rel_err(composed, true64), rel_err(feats, true64)
    print(f"whole_table {rows}x{d1} e_torch={e_torch:.3e} e_hip={e_hip:.3e} extra_bytes lorentz_to_poincare={extra_l2p} "
          f"log_map_zero={extra_log} (one result {one_result}) composed_extra_bytes={extra_torch}")
    assert feats.shape == ball_table.shape == (rows, d1 - 1) and bool(torch.isfinite(feats).all())
    assert e_hip <= PC.FACTOR * e_torch + PC.FLOOR
    assert extra_l2p <= one_result and extra_log <= one_result


# ---- 5. x == y in distance ------------------------------------------------------------------------------------------------
def test_distance_of_identical_points(golden_dir):
    """The golden bound says nothing for x == y: the float64 truth is 0, the reference's gradient there is rounding noise and
    e_ref is of order 1e9.  What can be asked instead, from the arithmetic: (-x) (+) x = (B - A) x / D with
    A = (1 - 2c|x|^2) + c|x|^2 and B = 1 - c|x|^2 equal in exact arithmetic; they differ by at most four fp32 roundings of
    numbers below 2, |A - B| <= 4 * 2^-24 = 2.4e-7, while sqrt(c)|x| / D <= 0.9 / (1 - 0.81)^2 = 25 inside the cap.  So
    sqrt(c) |(-x) (+) x| <= 6e-6 and the distance, 2 / sqrt(c) times that, stays below 1.2e-5 / sqrt(c); the gradient is finite."""
    pb = PB()
    meta, arrays = load(golden_dir)
    for name in ("dist_identical", "dist_identical_c0.7"):
        case = next(c for c in meta["cases"] if c["name"] == name)
        ours = run_ours(case, arrays)
        worst = float(np.abs(ours["out"]).max())
        print(f"{name} largest distance of identical points {worst:.3e}")
        assert worst <= 1.2e-5 / np.sqrt(case["c"]), name
        assert np.isfinite(ours["gx"]).all() and np.isfinite(ours["gy"]).all(), name
    x = ball(4096, 64, 1.0, 21).to(DEV)
    worst = float(pb.distance(x, x.clone()).abs().max())
    print(f"4096 identical pairs: largest distance {worst:.3e}")
    assert worst <= 1.2e-5


# ---- 6. the C ABI on padded and misaligned rows ---------------------------------------------------------------------------
def test_padded_and_misaligned_rows_through_the_c_abi(golden_dir):
    """Python always passes contiguous rows; the entry points also take a leading dimension above the width and bases that
    are not 16-byte aligned, where the kernels fall back from 16-byte to 4-byte accesses.  Every d = 32 golden case is run
    again through ctypes with ld = d + 3 (d + 1 + 3 on the Lorentz side) from a base one float past an aligned address, and
    must obey the same bound; the padding must stay untouched."""
    from hyptokenizer_amd import _lib
    from hyptokenizer_amd.engine import _ptr
    L = _lib.load()
    meta, arrays = load(golden_dir)
    PAD = 3
    FILL = 777.0

    def padded(a):
        """[n, w] array -> (device buffer, view of its rows with ld = w + PAD starting one float in)."""
        a = torch.from_numpy(np.ascontiguousarray(a)).to(DEV).reshape(-1, a.shape[-1])
        n, w = a.shape
        buf = torch.full((1 + n * (w + PAD),), FILL, device=DEV)
        view = buf[1:].view(n, w + PAD)
        view[:, :w] = a
        assert view.data_ptr() % 16 == 4
        return buf, view

    def blank(n, w):
        return padded(np.zeros((n, w), np.float32))

    def rows_of(view, w):
        assert bool((view[:, w:] == FILL).all())                            # the padding was not written
        return view[:, :w].cpu().numpy()

    seen = set()
    for case in meta["cases"]:
        op, c, name = case["op"], case["c"], case["name"]
        if op == "norm" or not case["ordinary"] or "_d32_" not in name:
            continue
        seen.add(op)
        A = lambda k: arrays[f"{name}__{k}"]                              # noqa: E731
        d, n = 32, A("g" + PC.OPS[op][0][-1]).shape[0]
        s = None                                                          # the default stream
        if op in ("mobius_addition", "distance"):
            (bx, x), (by, y) = padded(A("x")), padded(A("y"))
            if op == "mobius_addition":
                (bo, o), (bg, g), (b1, gx), (b2, gy) = blank(n, d), padded(A("g")), blank(n, d), blank(n, d)
                _lib.check(L.hm_rows_mobius_add(_ptr(x), _ptr(y), n, d + PAD, d, c, _ptr(o), d + PAD, s))
                _lib.check(L.hm_rows_mobius_add_bwd(_ptr(x), _ptr(y), _ptr(g), d + PAD, n, d + PAD, d, c, _ptr(gx), _ptr(gy), d + PAD, s))
                ours = {"out": rows_of(o, d), "gx": rows_of(gx, d), "gy": rows_of(gy, d)}
            else:
                o = torch.zeros(n, device=DEV)
                g = torch.from_numpy(A("g")).to(DEV).reshape(-1).contiguous()
                (b1, gx), (b2, gy) = blank(n, d), blank(n, d)
                _lib.check(L.hm_rows_poincare_distance(_ptr(x), _ptr(y), n, d + PAD, d, c, _ptr(o), s))
                _lib.check(L.hm_rows_poincare_distance_bwd(_ptr(x), _ptr(y), _ptr(g), n, d + PAD, d, c, _ptr(gx), _ptr(gy), d + PAD, s))
                ours = {"out": o.cpu().numpy(), "gx": rows_of(gx, d), "gy": rows_of(gy, d)}
        elif op == "mobius_scalar_mul":
            r = torch.from_numpy(A("r")).to(DEV).reshape(-1).contiguous()
            gr = torch.zeros(n, device=DEV)
            (bx, x), (bo, o), (bg, g), (b1, gx) = padded(A("x")), blank(n, d), padded(A("g")), blank(n, d)
            _lib.check(L.hm_rows_mobius_scalar_mul(_ptr(r), _ptr(x), n, d + PAD, d, c, _ptr(o), d + PAD, s))
            _lib.check(L.hm_rows_mobius_scalar_mul_bwd(_ptr(r), _ptr(x), _ptr(g), d + PAD, n, d + PAD, d, c, _ptr(gr), _ptr(gx), d + PAD, s))
            ours = {"out": rows_of(o, d), "gr": gr.cpu().numpy(), "gx": rows_of(gx, d)}
        elif op in ("exp_map_zero", "log_map_zero"):
            fwd, bwd = (L.hm_rows_exp_map_zero, L.hm_rows_exp_map_zero_bwd) if op == "exp_map_zero" else \
                       (L.hm_rows_log_map_zero, L.hm_rows_log_map_zero_bwd)
            (bx, x), (bo, o), (bg, g), (b1, gx) = padded(A("x")), blank(n, d), padded(A("g")), blank(n, d)
            _lib.check(fwd(_ptr(x), n, d + PAD, d, c, _ptr(o), d + PAD, s))
            _lib.check(bwd(_ptr(x), _ptr(g), d + PAD, n, d + PAD, d, c, _ptr(gx), d + PAD, s))
            ours = {"out": rows_of(o, d), "gx": rows_of(gx, d)}
        elif op == "lorentz_to_poincare":
            (bx, x), (bo, o), (bg, g), (b1, gx) = padded(A("x")), blank(n, d), padded(A("g")), blank(n, d + 1)
            _lib.check(L.hm_rows_lorentz_to_poincare(_ptr(x), n, d + 1 + PAD, d, c, _ptr(o), d + PAD, s))
            _lib.check(L.hm_rows_lorentz_to_poincare_bwd(_ptr(x), _ptr(g), d + PAD, n, d + 1 + PAD, d, c, _ptr(gx), d + 1 + PAD, s))
            ours = {"out": rows_of(o, d), "gx": rows_of(gx, d + 1)}
        else:
            (bx, x), (bo, o), (bg, g), (b1, gx) = padded(A("x")), blank(n, d + 1), padded(A("g")), blank(n, d)
            _lib.check(L.hm_rows_poincare_to_lorentz(_ptr(x), n, d + PAD, d, c, 0, _ptr(o), d + 1 + PAD, s))
            _lib.check(L.hm_rows_poincare_to_lorentz_bwd(_ptr(x), _ptr(g), d + 1 + PAD, n, d + PAD, d, c, 0, _ptr(gx), d + PAD, s))
            ours = {"out": rows_of(o, d + 1), "gx": rows_of(gx, d)}
        torch.cuda.synchronize()
        e_ref, e_hip = PC.errors(case, arrays), PC.errors(case, arrays, ours)
        for q in PC.quantities(case):
            print(f"padded:{name}:{q} e_ref={e_ref[q][0]:.3e} e_hip={e_hip[q][0]:.3e}")
            assert e_hip[q][1] and e_hip[q][0] <= PC.FACTOR * e_ref[q][0] + PC.FLOOR, (name, q, e_ref[q], e_hip[q])
    assert len(seen) == 7
