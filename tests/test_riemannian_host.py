"""Riemannian optimisers, the part that needs no GPU: the float64 truth of tests/riemannian_cases.py has the properties the
step is built for, the two entry points exist and refuse bad arguments before touching a device, and the Python layer
raises what it documents."""
import ctypes as C

import numpy as np
import pytest
import torch

import riemannian_cases as RC


# ---- 1. the truth itself ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d1,scale", [(2, 1.0), (5, 0.3), (101, 0.3), (129, 0.3), (65, 2.0)])
def test_truth_stays_on_the_manifold_and_transports_isometrically(d1, scale):
    """Absolute bounds: they hold for points of moderate norm (|<x', m'>| carries rounding of size 2^-53 |x'| |m'|)."""
    x, gs, m, v = (t[0] if isinstance(t, list) else t for t in RC.inputs(37, d1, scale, seed=d1))
    x, g, m, v = x.double(), gs.double(), m.double(), v.double()
    x = RC.lift(x[:, 1:])                                                  # the fp32 inputs are only near the hyperboloid
    m = m + RC.ldot(x, m).unsqueeze(-1) * x                                # ... and only near its tangent space
    for name, (y, m2) in {
        "sgd_mom": RC.sgd_step(x, g, m, 0.1, 0.9),
        "sgd_nesterov": RC.sgd_step(x, g, m, 0.1, 0.9, 0.1, True),
        "adam": RC.adam_step(x, g, m, v, 3, 0.05)[:2],
    }.items():
        assert float((RC.ldot(y, y) + 1).abs().max()) < 1e-12, name
        assert float(RC.ldot(y, m2).abs().max()) < 1e-12, name
    y, none = RC.sgd_step(x, g, m, 0.1)
    assert none is None and float((RC.ldot(y, y) + 1).abs().max()) < 1e-12
    # the transport is an isometry between the tangent spaces
    u = RC.rgrad(x, g)
    y = RC.retract(x, -0.1 * u)
    a, b = RC.transport(x, y, m), RC.transport(x, y, u)
    for (p, q), (tp, tq) in (((m, m), (a, a)), ((m, u), (a, b)), ((u, u), (b, b))):
        want, got = RC.ldot(p, q), RC.ldot(tp, tq)
        assert float((want - got).abs().max()) <= 1e-12 * float(want.abs().max()) * float(y.abs().max()) ** 2


def test_truth_reaches_the_same_minimum_with_both_optimisers():
    first_s, last_s, xs = RC.e2e_loop("sgd", torch.float64)
    first_a, last_a, xa = RC.e2e_loop("adam", torch.float64)
    assert first_s == first_a and last_s < first_s and last_a < first_a
    assert abs(last_s - last_a) <= 1e-3 * last_s
    assert np.abs(-xs[:, 0] ** 2 + (xs[:, 1:] ** 2).sum(-1) + 1).max() < 1e-12


# ---- 2. the C ABI ------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_listed():
    from hyptokenizer_amd import _lib
    L = _lib.load()
    for name in ("hm_rsgd_step", "hm_radam_step"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(L, name)
    assert L.hm_abi_version() == 3


def test_bad_arguments_are_refused_without_a_device():
    from hyptokenizer_amd import _lib
    L = _lib.load()
    E = _lib.HM_E_ARG
    P = C.c_void_p(4096)                                                    # never dereferenced: every call below fails or has n == 0
    nan, inf = float("nan"), float("inf")

    def sgd(x=P, ld_x=11, g=P, ld_g=11, m=P, ld_m=11, rows=None, n=5, table=5, d1=11, lr=0.1, mu=0.9, damp=0.0, nest=0):
        return L.hm_rsgd_step(x, ld_x, g, ld_g, m, ld_m, rows, n, table, d1, lr, mu, damp, nest, None)

    def adam(x=P, ld_x=11, g=P, ld_g=11, m=P, ld_m=11, v=P, rows=None, n=5, table=5, d1=11, lr=0.1, b1=0.9, b2=0.999, eps=1e-8,
             bc1=0.1, bc2=0.001):
        return L.hm_radam_step(x, ld_x, g, ld_g, m, ld_m, v, rows, n, table, d1, lr, b1, b2, eps, bc1, bc2, None)

    for fn in (sgd, adam):
        assert fn(x=None) == E and fn(g=None) == E and fn(m=None) == E
        assert fn(d1=1) == E and fn(d1=130, ld_x=130, ld_g=130, ld_m=130) == E
        assert fn(ld_x=10) == E and fn(ld_g=10) == E and fn(ld_m=10) == E
        assert fn(n=-1, table=-1) == E and fn(n=-1, rows=P) == E
        assert fn(n=4, table=5) == E                                        # dense: n == table_rows
        assert fn(lr=-0.1) == E and fn(lr=nan) == E and fn(lr=inf) == E
        assert fn(n=0, table=0) == _lib.HM_OK and fn(n=0, table=5, rows=P) == _lib.HM_OK
        assert fn(n=0, table=0, d1=2, ld_x=2, ld_g=2, ld_m=2) == _lib.HM_OK and fn(n=0, table=0, d1=129, ld_x=129, ld_g=200, ld_m=129) == 0
    assert sgd(mu=1.0) == E and sgd(mu=-0.1) == E and sgd(mu=nan) == E
    assert sgd(damp=1.0) == E and sgd(damp=-0.1) == E and sgd(damp=nan) == E
    assert sgd(nest=2) == E
    assert sgd(mu=0.0, m=P) == E                                            # no momentum: no buffer
    assert sgd(mu=0.0, m=None, n=0, table=0) == _lib.HM_OK
    assert adam(v=None) == E
    assert adam(b1=1.0) == E and adam(b1=-0.1) == E and adam(b2=1.0) == E and adam(b2=nan) == E
    assert adam(bc1=0.0) == E and adam(bc2=0.0) == E and adam(bc1=-1.0) == E and adam(bc2=nan) == E
    assert adam(eps=-1e-8) == E and adam(eps=nan) == E
    assert b"hm_radam_step" in L.hm_last_error(None)


# ---- 3. the Python layer ------------------------------------------------------------------------------------------------
def test_python_layer_raises_what_it_documents():
    from hyptokenizer_amd.engine import HypMergeUnavailable
    from hyptokenizer_amd.optim import RiemannianAdam, RiemannianSGD
    for cls in (RiemannianSGD, RiemannianAdam):
        with pytest.raises(ValueError):
            cls([torch.zeros(4, 5, dtype=torch.float64, requires_grad=True)], lr=0.1)
        with pytest.raises(ValueError):
            cls([torch.zeros(4, 1, requires_grad=True)], lr=0.1)
        with pytest.raises(ValueError):
            cls([torch.zeros(4, 130, requires_grad=True)], lr=0.1)
        with pytest.raises(ValueError):
            cls([torch.zeros(5, 4, requires_grad=True).t()], lr=0.1)        # no unit stride in the last dimension
        with pytest.raises(ValueError):
            cls([torch.zeros(4, 5, requires_grad=True)], lr=-1.0)
        p = torch.nn.Parameter(RC.lift(torch.zeros(4, 4)))
        opt = cls([p], lr=0.1)
        opt.step()                                                          # grad is None: skipped
        assert opt.state_dict()["state"] == {}
        p.grad = torch.ones_like(p)
        with pytest.raises(HypMergeUnavailable):
            opt.step()
        opt.zero_grad()
        assert p.grad is None
    with pytest.raises(ValueError):
        RiemannianSGD([torch.zeros(4, 5, requires_grad=True)], lr=0.1, momentum=1.0)
    with pytest.raises(ValueError):
        RiemannianSGD([torch.zeros(4, 5, requires_grad=True)], lr=0.1, nesterov=True)
    with pytest.raises(ValueError):
        RiemannianAdam([torch.zeros(4, 5, requires_grad=True)], betas=(0.9, 1.0))
    with pytest.raises(ValueError):
        RiemannianAdam([torch.zeros(4, 5, requires_grad=True)], eps=-1.0)
    # a padded table (row stride above the width) and flattened leading dimensions are parameters
    wide = torch.zeros(6, 8)
    RiemannianSGD([wide[:, :5].requires_grad_()], lr=0.1)
    RiemannianAdam([torch.zeros(2, 3, 5, requires_grad=True)], lr=0.1)
    from hyptokenizer_amd.optim import riemannian as R
    assert R._rows_of(wide[:, :5]) == (6, 8) and R._rows_of(torch.zeros(2, 3, 5)) == (6, 5) and R._rows_of(torch.zeros(5)) == (1, 5)
