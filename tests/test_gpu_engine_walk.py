"""GPU: the engine walks of tests/engine_walk.py on the HIP engine.

One long-lived ``MergeEngine`` takes every call of a walk -- searches, appends, overwrites, truncations, projections, new
tables, refreshes in two halves, device loops, refused calls -- and after every call its live-row count and every observable
(argmin records, ordered lists, candidate lists, counts, gathered distances, midpoint rows, every table row a call wrote,
loop records) must equal the model's, bit for bit -- a NaN by its position (``engine_walk.same``) -- where the model is the CPU
oracle, which holds no state between calls.  At every
motif's probe the engine is also compared with a NEW engine built by ``set_table`` from the table as it is: state that
survives a call it should not have survived shows there even where engine and oracle share an error.

The shapes are the smallest at which the state can go wrong (max_rows = n0 + 400): (250, 10) starts under one 256-row block
and grows across it; (1015, 37) has an odd width and grows across 1024 and the 512-row block edge; (2040, 100) is the
benchmark width (13 bf16 chunks and a half k-step) and grows across 2048.
"""
import time

import pytest
import torch

import engine_walk as W

pytestmark = pytest.mark.gpu

FORMS = ["f32", "bf16"]
CASES = [(seed, n0, d, mode, form) for (seed, n0, d) in W.SHAPES for mode in ("lorentz", "reference") for form in FORMS]
CASES += [(seed, n0, d, mode, form) for (seed, n0, d) in W.SHAPES[1:2] for mode in ("lorentz", "reference") for form in ("bf16-512", "bf16-k112")]

@pytest.fixture
def prefilter_form(request, monkeypatch):
    """The prefilter forms of tests/test_gpu_engine.py, set the way its fixture sets them: exact fp32 MFMA prefilter, bf16 MFMA
    prefilter, the bf16 prefilter in its large-table shape (512-row blocks, forced here at every size), and the bf16 prefilter
    on image rows padded to whole 16-slot k-steps -- `hm_debug_set_default_knob` applies to every engine created afterwards."""
    from hyptokenizer_amd import _lib
    L = _lib.load()
    monkeypatch.setenv("HM_SCAN_PRECISION", request.param.split("-")[0])
    _lib.check(L.hm_debug_set_default_knob(None, 0.0, 1))
    if request.param.endswith("-512"):
        _lib.check(L.hm_debug_set_default_knob(b"big_rows", 2.0, 0))
    if request.param.endswith("-k112"):
        _lib.check(L.hm_debug_set_default_knob(b"kc_even", 1.0, 0))
    yield request.param
    _lib.check(L.hm_debug_set_default_knob(None, 0.0, 1))


def _gpu_side(max_rows, d1, mode, form, knobs=()):
    from hyptokenizer_amd import _lib
    from hyptokenizer_amd.engine import MergeEngine
    eng = MergeEngine(max_rows, d1, mode)
    for name, value in knobs:
        _lib.check(_lib.load().hm_debug_set_knob(eng._h, name, value))
    table = torch.zeros((max_rows, d1), dtype=torch.float32, device="cuda")
    return W.Side(eng, table, refuses=True, form=form.split("-")[0], close=eng.close)


def _fresh(side):
    """a new engine that has seen nothing but ``set_table`` of the subject's table as it is"""
    from hyptokenizer_amd.engine import MergeEngine
    eng = MergeEngine(side.eng.max_rows, side.eng.d1, side.eng.sign_mode)
    table = side.table.clone()
    eng.set_table(table, side.eng.n)
    return W.Side(eng, table, refuses=True, form=side.form, close=eng.close)


def _walk(seed, n0, d, mode, form, knobs=()):
    trace = W.build_trace(seed, n0, d, mode)
    side = _gpu_side(trace.max_rows, d + 1, mode, form, knobs)
    t0 = time.perf_counter()
    try:
        W.run_trace(trace, side, fresh=_fresh)
    finally:
        side.close()
    grown = [ok for ok, g in side.refreshes if g]
    voided = [ok for ok, g in side.refreshes if not g]
    print(f"engine walk seed={seed} n0={n0} d={d} {mode} {form}: {len(trace.steps)} calls in {time.perf_counter() - t0:.2f} s; "
          f"refreshes accepted: {sum(grown)}/{len(grown)} on a grown table, {sum(voided)}/{len(voided)} after a voiding call; "
          f"{side.host_steps} loop steps through the host path")
    assert len(grown) >= 6
    if mode == "lorentz":
        # a walk in which the engine never took the incremental route on a grown table tests nothing of that route: that
        # would be a defect of motif D's parameters (thresholds, k), not of the engine
        assert sum(grown) >= 1
    # every voiding call of motif E makes the incremental route inapplicable by construction: a refresh accepted after one
    # means a transition forgot to void the cut or the previous list, whether or not a wrong result happens to follow
    assert sum(voided) == 0
    return side


@pytest.mark.parametrize("seed,n0,d,mode,prefilter_form", CASES, indirect=["prefilter_form"])
def test_engine_walk_equals_the_model(oracle, seed, n0, d, mode, prefilter_form):
    _walk(seed, n0, d, mode, prefilter_form)


@pytest.mark.parametrize("prefilter_form", ["bf16"], indirect=True)
def test_engine_walk_through_the_pipelined_loop(oracle, prefilter_form):
    """motif H through the software-pipelined standard loop and its fallbacks (`pipeline_pairs` = 0: pipelined at this small
    size too, where tails longer than scans trip the order guard by themselves)"""
    seed, n0, d = W.SHAPES[2]
    _walk(seed, n0, d, "lorentz", prefilter_form, knobs=((b"pipeline", 1.0), (b"pipeline_pairs", 0.0)))


# Prefixes of the walks above that once failed, kept by name (seed, n0, d, mode, calls):
#   seed 11, call #4: the first uncounted top-k of a 250-row table emitted every candidate and answered their exact number
#       where include/hypmerge.h promises -1 ("at least k, not counted");
#   seed 11 (literal sign mode), call #8 and seed 11 (lorentz), call #340: the first rows merged from NaN operands, whose NaN
#       has other bits on the GPU than on the host CPU (engine_walk.same).
REGRESSIONS = [(11, 250, 10, "lorentz", 5), (11, 250, 10, "reference", 9), (11, 250, 10, "lorentz", 341)]


@pytest.mark.parametrize("prefilter_form", ["f32"], indirect=True)
@pytest.mark.parametrize("seed,n0,d,mode,upto", REGRESSIONS)
def test_engine_walk_regressions(oracle, seed, n0, d, mode, upto, prefilter_form):
    side = W.replay(seed, n0, d, mode, prefilter_form, upto=upto, make_side=_gpu_side, fresh=_fresh)
    side.close()
