"""Fused Riemannian SGD / Adam steps on the GPU (csrc/hm_riemann.hip, hyptokenizer_amd.optim) against the float64 truth of
tests/riemannian_cases.py.

Bound of every comparison (the rule of test_gpu_autograd.py, set by the feature's specification, not tuned): with e_ref the
error of the same step run by torch in fp32 on the CPU against the float64 truth and e_hip ours, both the largest absolute
error of an array relative to the array's largest magnitude, ``e_hip <= 4 * e_ref + 2**-20``; non-finite entries are
compared by position and kind.  Each case prints ``name e_ref e_hip`` before it asserts (run with -s to collect the table of
DESIGN.md 5.16).  Every case has at most 300 rows.
"""
import numpy as np
import pytest
import torch

import riemannian_cases as RC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 3
FILL = 777.0


def OPT():
    from hyptokenizer_amd import optim
    return optim


def padded(a: torch.Tensor, pad: int):
    """[n, w] rows -> a device view with leading dimension w + pad whose padding holds FILL."""
    n, w = a.shape
    buf = torch.full((n, w + pad), FILL, device=DEV)
    buf[:, :w] = a.to(DEV)
    return buf


def hip_steps(setting, x, gs, m, v, pads=(0, 0, 0), rows=None, table=None, lr=None):
    """The chained steps of ``setting`` through the C ABI.  ``pads``: extra columns of the x, g and m buffers.  ``rows`` (int64
    device tensor): the indexed form, gs are then compact and ``table`` = (x, m, v) are the full tables.  ``lr`` replaces the
    setting's rate.  Returns one dict per step like riemannian_cases.run, and the final device buffers."""
    from hyptokenizer_amd import _lib
    from hyptokenizer_amd.engine import _ptr
    L = _lib.load()
    opt, kw, t0 = RC.SETTINGS[setting]
    kw = kw if lr is None else dict(kw, lr=lr)
    if table is not None:
        x, m, v = table
    d1 = x.shape[1]
    xb, mb = padded(x, pads[0]), padded(m, pads[2])
    vb = v.to(DEV).clone()
    n = gs[0].shape[0]
    out = []
    for k, g in enumerate(gs):
        gb = padded(g, pads[1])
        if opt == "sgd":
            mu = kw.get("momentum", 0.0)
            _lib.check(L.hm_rsgd_step(_ptr(xb), d1 + pads[0], _ptr(gb), d1 + pads[1], _ptr(mb) if mu else None, d1 + pads[2],
                                      _ptr(rows), n, x.shape[0], d1, kw["lr"], mu, kw.get("dampening", 0.0),
                                      int(kw.get("nesterov", False)), None))
            res = {"x": xb[:, :d1].cpu().numpy()}
            if mu:
                res["m"] = mb[:, :d1].cpu().numpy()
        else:
            bc1, bc2 = RC.bias_corrections(kw["beta1"], kw["beta2"], t0 + k)
            _lib.check(L.hm_radam_step(_ptr(xb), d1 + pads[0], _ptr(gb), d1 + pads[1], _ptr(mb), d1 + pads[2], _ptr(vb), _ptr(rows),
                                       n, x.shape[0], d1, kw["lr"], kw["beta1"], kw["beta2"], kw["eps"], bc1, bc2, None))
            res = {"x": xb[:, :d1].cpu().numpy(), "m": mb[:, :d1].cpu().numpy(), "v": vb.cpu().numpy()}
        out.append(res)
        assert bool((gb[:, d1:] == FILL).all())
    torch.cuda.synchronize()
    assert bool((xb[:, d1:] == FILL).all()) and bool((mb[:, d1:] == FILL).all())       # the padding was not written
    return out, (xb, mb, vb)


def check_case(setting, rows, d1, scale, seed, steps=1, pads=(0, 0, 0), failures=None):
    x, gs, m, v = RC.inputs(rows, d1, scale, seed, steps)
    truth, ref32 = RC.reference(setting, rows, d1, scale, seed, steps)
    ours, _ = hip_steps(setting, x, gs, m, v, pads)
    own = [] if failures is None else failures
    RC.compare(f"{setting}_r{rows}_w{d1}_s{scale}" + ("_padded" if any(pads) else ""), truth, ref32, ours, own)
    if failures is None:
        assert not own, "\n".join(own)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- 1. every width, row count and setting against the truth ------------------------------------------------------------------
@pytest.mark.parametrize("d1", RC.WIDTHS)
def test_single_step_every_setting_and_row_count(d1):
    failures = []
    for k, setting in enumerate(RC.SETTINGS):
        for rows in RC.ROWS:
            check_case(setting, rows, d1, 0.3 if (k + rows) % 2 else 2.0, seed=1000 * d1 + rows, failures=failures)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("d1", RC.WIDTHS)
def test_padded_leading_dimensions(d1):
    """ld = d1 + 3 for x, d1 + 1 for g and d1 + 5 for m: a different one per operand; the padding stays untouched."""
    failures = []
    for setting in ("sgd", "sgd_mom", "adam_t3"):
        check_case(setting, 37, d1, 0.3, seed=77 + d1, pads=(PAD, 1, 5), failures=failures)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("setting", list(RC.SETTINGS))
def test_three_chained_steps(setting):
    failures = []
    for d1, scale in ((5, 0.3), (65, 2.0), (101, 0.3), (129, 2.0)):
        check_case(setting, 37, d1, scale, seed=31 + d1, steps=3, failures=failures)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("setting", list(RC.SETTINGS))
def test_points_far_from_the_origin(setting):
    """Spatial norm about 6: <x, h> x cancels against h in the tangent projection, e_ref grows and the bound with it."""
    failures = []
    for d1 in (17, 101):
        check_case(setting, 37, d1, 6.0, seed=600 + d1, failures=failures)
    assert not failures, "\n".join(failures)


# ---- 2. special rows ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", ["sgd", "sgd_mom", "adam_t3"])
@pytest.mark.parametrize("d1", [5, 101])
def test_zero_gradient_row_keeps_its_point(setting, d1):
    x, gs, m, v = RC.inputs(37, d1, 2.0, seed=5, steps=1)
    g, m = gs[0].clone(), m.clone()
    g[11], m[11] = 0.0, 0.0
    ours, _ = hip_steps(setting, x, [g], m, v)
    got = ours[0]["x"]
    assert np.array_equal(bits(got[11, 1:]), bits(x[11, 1:].numpy()))                  # the spatial part bit for bit
    want0 = np.sqrt(1.0 + (x[11, 1:].double().numpy() ** 2).sum())
    # d <= 128 products summed by a tree of depth <= 9, one add and one square root: below 12 roundings of 2^-24
    assert abs(got[11, 0] - want0) <= 2.0 ** -20 * want0
    if "m" in ours[0]:
        assert not ours[0]["m"][11].any()
    assert not np.array_equal(bits(got[10]), bits(x[10].numpy()))


@pytest.mark.parametrize("setting", ["sgd", "sgd_nesterov", "adam_t1"])
@pytest.mark.parametrize("d1", [17, 129])
def test_nan_gradient_row_stays_in_its_row(setting, d1):
    x, gs, m, v = RC.inputs(37, d1, 0.3, seed=6, steps=1)
    clean, _ = hip_steps(setting, x, gs, m, v)
    g = gs[0].clone()
    g[20, d1 // 2] = float("nan")
    dirty, _ = hip_steps(setting, x, [g], m, v)
    for q in clean[0]:
        a, b = clean[0][q], dirty[0][q]
        assert not np.isfinite(b[20]).any(), q                                          # the whole row goes non-finite
        keep = np.arange(37) != 20
        assert np.array_equal(bits(a[keep]), bits(b[keep])), q


# ---- 3. the indexed form --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", ["sgd", "sgd_mom", "adam_t3"])
@pytest.mark.parametrize("d1", [17, 101])
def test_indexed_form(setting, d1):
    x, gs, m, v = RC.inputs(257, d1, 0.3, seed=8, steps=1)
    idx = torch.randperm(257, generator=torch.Generator().manual_seed(3))[:50]          # distinct, unsorted
    compact = gs[0][idx].contiguous()
    dense, _ = hip_steps(setting, x, gs, m, v)
    got, _ = hip_steps(setting, None, [compact], None, None, rows=idx.to(DEV), table=(x, m, v), pads=(PAD, 0, 1))
    before = {"x": x.numpy(), "m": m.numpy(), "v": v.numpy()}
    untouched = np.ones(257, bool)
    untouched[idx.numpy()] = False
    for q in dense[0]:
        assert np.array_equal(bits(got[0][q][idx.numpy()]), bits(dense[0][q][idx.numpy()])), q     # the dense step on those rows
        assert np.array_equal(bits(got[0][q][untouched]), bits(before[q][untouched])), q            # nothing else moved
    # indices outside the table are skipped and change nothing else
    bad = torch.cat([idx[:20], torch.tensor([257]), idx[20:40], torch.tensor([-1, 1 << 40]), idx[40:]])
    compact_bad = torch.zeros(len(bad), d1)
    ok = (bad >= 0) & (bad < 257)
    compact_bad[ok] = compact
    compact_bad[~ok] = 1.0e3
    got_bad, _ = hip_steps(setting, None, [compact_bad], None, None, rows=bad.to(DEV), table=(x, m, v))
    for q in dense[0]:
        assert np.array_equal(bits(got_bad[0][q]), bits(got[0][q])), q


# ---- 4. the optimiser classes ----------------------------------------------------------------------------------------------------
def make(cls, params, **kw):
    o = OPT()
    return {"sgd": o.RiemannianSGD, "adam": o.RiemannianAdam}[cls](params, **kw)


@pytest.mark.parametrize("cls,kw,setting", [("sgd", dict(lr=0.1), "sgd"), ("sgd", dict(lr=0.1, momentum=0.9, dampening=0.1), "sgd_damp"),
                                            ("adam", dict(lr=0.05), "adam_t1")])
def test_optimiser_takes_the_dense_call_and_matches_the_c_abi(cls, kw, setting):
    """From zero state the classes run exactly the entry point of section 1 -- on a 3-D parameter and on a padded table."""
    x, gs, m, v = RC.inputs(36, 17, 0.3, seed=9, steps=2)
    zero_m, zero_v = torch.zeros_like(m), torch.zeros_like(v)
    want, _ = hip_steps(setting, x, gs, zero_m, zero_v)
    p3 = torch.nn.Parameter(x.reshape(4, 9, 17).to(DEV))
    wide = torch.full((36, 24), FILL, device=DEV)
    wide[:, :17] = x.to(DEV)
    pw = wide[:, :17].requires_grad_()
    for p in (p3, pw):
        opt = make(cls, [p], **kw)
        for k, g in enumerate(gs):
            p.grad = g.reshape(p.shape).to(DEV)
            opt.step()
            assert np.array_equal(bits(p.detach().reshape(36, 17).cpu().numpy()), bits(want[k]["x"])), k
        st = opt.state[p]
        if cls == "adam":
            assert st["step"] == 2 and st["exp_avg"].shape == p.shape and st["exp_avg_sq"].shape == (36,)
            assert np.array_equal(bits(st["exp_avg_sq"].cpu().numpy()), bits(want[1]["v"]))
        elif kw.get("momentum"):
            assert np.array_equal(bits(st["momentum_buffer"].reshape(36, 17).cpu().numpy()), bits(want[1]["m"]))
        else:
            assert len(st) == 0
    assert bool((wide[:, 17:] == FILL).all())


@pytest.mark.parametrize("cls,kw", [("sgd", dict(lr=0.1)), ("sgd", dict(lr=0.1, momentum=0.9)), ("adam", dict(lr=0.05))])
def test_sparse_gradient_with_repeated_indices_equals_the_dense_gradient(cls, kw):
    x = RC.inputs(257, 17, 0.3, seed=10)[0]
    gen = torch.Generator().manual_seed(4)
    idx = torch.randperm(257, generator=gen)[:40]
    idx = torch.cat([idx, idx[:15]])[torch.randperm(55, generator=gen)]                  # 15 rows listed twice, unsorted
    vals = torch.randn(55, 17, generator=gen)
    sparse = torch.sparse_coo_tensor(idx.unsqueeze(0), vals, (257, 17)).to(DEV)
    assert not sparse.is_coalesced()
    dense = sparse.coalesce().to_dense()
    ps, pd = torch.nn.Parameter(x.to(DEV)), torch.nn.Parameter(x.to(DEV))
    os_, od = make(cls, [ps], **kw), make(cls, [pd], **kw)
    ps.grad, pd.grad = sparse, dense
    os_.step()
    od.step()
    touched = np.zeros(257, bool)
    touched[idx.numpy()] = True
    a, b = ps.detach().cpu().numpy(), pd.detach().cpu().numpy()
    assert np.array_equal(bits(a[touched]), bits(b[touched]))
    assert np.array_equal(bits(a[~touched]), bits(x.numpy()[~touched]))                  # lazy: rows not listed do not move
    for key in ("momentum_buffer", "exp_avg", "exp_avg_sq"):
        if key in os_.state[ps]:
            sa, sb = os_.state[ps][key].cpu().numpy(), od.state[pd][key].cpu().numpy()
            assert np.array_equal(bits(sa[touched]), bits(sb[touched])), key
            assert not sa[~touched].any(), key
    if cls == "adam":
        assert os_.state[ps]["step"] == 1
    emb = torch.nn.Embedding(257, 17, sparse=True).to(DEV)                               # what nn.Embedding(sparse=True) produces
    with torch.no_grad():
        emb.weight.copy_(x.to(DEV))
    opt = make(cls, emb.parameters(), **kw)
    emb(idx.to(DEV)).square().sum().backward()
    assert emb.weight.grad.is_sparse
    opt.step()
    w = emb.weight.detach().cpu().numpy()
    assert np.array_equal(bits(w[~touched]), bits(x.numpy()[~touched])) and np.isfinite(w).all()
    assert not np.array_equal(bits(w[touched]), bits(x.numpy()[touched]))
    p3 = torch.nn.Parameter(x[:256].reshape(16, 16, 17).to(DEV))
    p3.grad = torch.sparse_coo_tensor(torch.zeros(1, 1, dtype=torch.long), torch.ones(1, 16, 17), (16, 16, 17)).to(DEV)
    o3 = make(cls, [p3], **kw)
    with pytest.raises(ValueError):                                                      # a sparse gradient needs a 2-D parameter
        o3.step()


@pytest.mark.parametrize("cls,kw", [("sgd", dict(momentum=0.9)), ("adam", dict())])
def test_param_groups_state_dict_round_trip_and_closure(cls, kw):
    x, gs, m, v = RC.inputs(37, 17, 0.3, seed=11, steps=4)
    y = RC.inputs(20, 5, 0.3, seed=12, steps=4)

    def fresh():
        a, b = torch.nn.Parameter(x.to(DEV)), torch.nn.Parameter(y[0].to(DEV))
        return a, b, make(cls, [{"params": [a], "lr": 0.1}, {"params": [b], "lr": 0.01}], lr=0.5, **kw)

    def feed(a, b, k):
        a.grad, b.grad = gs[k].to(DEV), y[1][k].to(DEV)

    a, b, opt = fresh()
    for k in range(4):
        feed(a, b, k)
        opt.step()
    # each group stepped at its own rate: the first step equals the C-ABI step at that rate
    a1, b1, o1 = fresh()
    feed(a1, b1, 0)
    o1.step()
    for p, p0, g0, lr in ((a1, x, gs[0], 0.1), (b1, y[0], y[1][0], 0.01)):
        want, _ = hip_steps("sgd_mom" if cls == "sgd" else "adam_t1", p0, [g0], torch.zeros_like(p0), torch.zeros(p0.shape[0]), lr=lr)
        assert np.array_equal(bits(p.detach().cpu().numpy()), bits(want[0]["x"]))
    # two steps, save, restore into a new optimiser, two more steps: bit-identical to four steps in a row
    a2, b2, o2 = fresh()
    for k in range(2):
        feed(a2, b2, k)
        o2.step()
    saved = o2.state_dict()
    a3, b3 = torch.nn.Parameter(a2.detach().clone()), torch.nn.Parameter(b2.detach().clone())
    o3 = make(cls, [{"params": [a3], "lr": 0.1}, {"params": [b3], "lr": 0.01}], lr=0.5, **kw)
    o3.load_state_dict(saved)
    for k in range(2, 4):
        feed(a3, b3, k)
        o3.step()
    assert np.array_equal(bits(a3.detach().cpu().numpy()), bits(a.detach().cpu().numpy()))
    assert np.array_equal(bits(b3.detach().cpu().numpy()), bits(b.detach().cpu().numpy()))
    for key in o3.state[a3]:
        s3, s = o3.state[a3][key], opt.state[a][key]
        assert (s3 == s) if isinstance(s, int) else np.array_equal(bits(s3.cpu().numpy()), bits(s.cpu().numpy())), key
    # a closure is called, with gradients enabled, and its value returned
    calls = []

    def closure():
        assert torch.is_grad_enabled()
        calls.append(1)
        feed(a3, b3, 0)
        return torch.tensor(3.5)

    assert float(o3.step(closure)) == 3.5 and len(calls) == 1
    o3.zero_grad()
    assert a3.grad is None and b3.grad is None
    o3.step()                                                                            # no gradients: nothing to do


# ---- 5. end to end ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", ["sgd", "adam"])
def test_training_loop_descends_and_follows_the_float64_loop(cls):
    from hyptokenizer_amd.embedding import lorentz_model as lm
    x0, pts = RC.e2e_inputs()
    first64, last64, x64 = RC.e2e_loop(cls, torch.float64)
    first32, last32, x32 = RC.e2e_loop(cls, torch.float32)
    p = torch.nn.Parameter(x0.to(DEV))
    pts = pts.to(DEV)
    opt = make(cls, [p], **RC.E2E[cls])

    def loss_of():
        return (lm.distance(p.unsqueeze(1), pts.unsqueeze(0), sign_convention="lorentz") ** 2).sum()

    first = None
    for _ in range(RC.E2E_STEPS):
        opt.zero_grad()
        loss = loss_of()
        loss.backward()
        first = float(loss.detach()) if first is None else first
        opt.step()
    with torch.no_grad():
        last = float(loss_of())
    got = p.detach().cpu().numpy()
    form = lambda a: float(np.abs(-a[:, 0].astype(np.float64) ** 2 + (a[:, 1:].astype(np.float64) ** 2).sum(-1) + 1).max())  # noqa: E731
    scale = float(np.abs(x64).max())
    e_ref, e_hip = float(np.abs(x32 - x64).max()) / scale, float(np.abs(got - x64).max()) / scale
    l_ref, l_hip = abs(last32 - last64) / abs(last64), abs(last - last64) / abs(last64)
    print(f"e2e_{cls}: loss {first:.6f} -> {last:.6f} (float64 {first64:.6f} -> {last64:.6f}) x e_ref={e_ref:.3e} e_hip={e_hip:.3e} "
          f"loss e_ref={l_ref:.3e} e_hip={l_hip:.3e} manifold e_ref={form(x32):.3e} e_hip={form(got):.3e}")
    assert last < first
    assert l_hip <= RC.FACTOR * l_ref + RC.FLOOR
    assert form(got) <= RC.FACTOR * form(x32) + RC.FLOOR
