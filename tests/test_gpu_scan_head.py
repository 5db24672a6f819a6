"""GPU: the argmin scan's head test (hm_scan.hip, HEAD > 0; knob `head`) changes no result.

A column group whose head k-steps already put every pair above the bound is dropped after 3 of its k-steps; every other
group is recomputed by the complete chain.  Here every search and every 20-step merge loop is compared, bit for bit, with
the oracle AND with the same run under `head = 0` (the kernels without the test), in the regimes where the two kernels
take different paths: a loose bound (every group continues), a bound at distance 0 from the first tile on, nearest pairs
that only the rest slots or only the head slots can tell apart, non-finite rows, the pipelined loop with both counter
sets, a shrunk item queue, a re-projected table (the rest norm in the row's last K-slot must survive) and, on the same
engine, the kernels that multiply that slot by 0 (reference sign is a different engine; top-k is the same one).

The library launches the head kernel only where it expects a tight bound (from the third merge into a table on,
hm_head_live in hm_common.h): the first search of every engine here runs the kernel without the test and the merge loop
switches at its fourth step.  Every comparison is therefore made a third time with `head_force = 1`, which sends every
eligible launch through the head kernel -- the loose-bound first search included, where every group is recomputed.

Widths: d = 100 (13 chunks: the head's time step is the half step), d = 108 (14 chunks: a whole last k-step; `bf16-k112`
turns d = 100 into that layout too) and d = 24 (4 chunks, two k-steps: no head, the knob must be inert)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from hyptokenizer_amd.synthetic import lorentz_table  # noqa: E402

STEPS = 20


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(params=["bf16", "bf16-512", "bf16-k112"], autouse=True)
def prefilter_form(request):
    """the bf16 fixtures of tests/test_gpu_engine.py (the fp32 form has no head test): 256-row blocks, 512-row blocks forced
    at every size (128-row waves: one accumulator set, no head test -- the rest-norm slot must be harmless there), and
    rows padded to whole k-steps"""
    from hyptokenizer_amd import _lib
    L = _lib.load()
    _lib.check(L.hm_debug_set_default_knob(None, 0.0, 1))
    if request.param.endswith("-512"):
        _lib.check(L.hm_debug_set_default_knob(b"big_rows", 2.0, 0))
    if request.param.endswith("-k112"):
        _lib.check(L.hm_debug_set_default_knob(b"kc_even", 1.0, 0))
    yield request.param
    _lib.check(L.hm_debug_set_default_knob(None, 0.0, 1))


def _engine(X, knobs, extra=64, mode="lorentz"):
    from hyptokenizer_amd import _lib
    from hyptokenizer_amd.engine import MergeEngine
    L = _lib.load()
    n, d1 = X.shape
    table = torch.zeros((n + extra, d1), dtype=torch.float32, device="cuda")
    table[:n] = torch.from_numpy(X).cuda()
    eng = MergeEngine(n + extra, d1, mode, prefilter="bf16")
    for k, v in knobs.items():
        _lib.check(L.hm_debug_set_knob(eng._h, k.encode(), float(v)))
    eng.set_table(table, n)
    return eng, table


def _lengths(n):
    return (np.arange(1, n + 1, dtype=np.int32) % 5 + 1).astype(np.int32)


def _oracle_loop(oracle, X, thr, steps, lens):
    """the standard loop on the host: nearest pair below thr, weighted midpoint appended (smoke() of __graft_entry__.py)"""
    n, d1 = X.shape
    Xo = np.zeros((n + steps, d1), np.float32)
    Xo[:n] = X
    lens = list(lens)
    pairs, dist = [], []
    cur = n
    for _ in range(steps):
        od, oi, oj, oc = oracle.pairwise_topk(Xo, cur, 1.0, float(np.float32(thr)), 1, 1)
        if oc == 0:
            break
        i, j = int(oi[0]), int(oj[0])
        w = np.float32(np.float64(lens[j]) / np.float64(lens[i] + lens[j]))
        Xo[cur] = oracle.midpoint_batch(Xo, [i], [j], [w], 1.0, 1)[0]
        lens.append(lens[i] + lens[j])
        pairs.append((i, j))
        dist.append(_bits(od[:1])[0])
        cur += 1
    return pairs, dist, Xo[n:cur]


def _gpu_loop(X, thr, knobs, steps=STEPS):
    n = X.shape[0]
    eng, table = _engine(X, knobs, extra=steps + 8)
    first = eng.argmin(1.0, thr)
    eng.set_token_lengths(_lengths(n))
    recs, done = eng.std_merge_steps(1.0, thr, table, steps)
    rows = table[n:n + done].cpu().numpy()
    return first, [r[2:] for r in recs[:done]], [_bits([r[1]])[0] for r in recs[:done]], rows, done


def _check_table(oracle, X, thr, knobs=None):
    """argmin and a 20-step loop: head test on == head = 0 == oracle, bit for bit"""
    knobs = dict(knobs or {})
    on = _gpu_loop(X, thr, knobs)
    off = _gpu_loop(X, thr, dict(knobs, head=0))
    forced = _gpu_loop(X, thr, dict(knobs, head_force=1))
    for other in (off, forced):
        assert on[0] == other[0] and on[1] == other[1] and on[2] == other[2] and on[4] == other[4]
        assert np.array_equal(on[3].view(np.uint32), other[3].view(np.uint32))
    od, oi, oj, oc = oracle.pairwise_topk(X, X.shape[0], 1.0, float(np.float32(thr)), 1, 1)
    if oc == 0:
        assert on[0] is None
    else:
        assert on[0] is not None and (on[0][1], on[0][2]) == (int(oi[0]), int(oj[0])) and _bits([on[0][0]])[0] == _bits(od[:1])[0]
    pairs, dist, rows = _oracle_loop(oracle, X, thr, STEPS, _lengths(X.shape[0]))
    assert [tuple(p) for p in on[1]] == pairs and on[2] == dist
    assert np.array_equal(on[3].view(np.uint32), rows.view(np.uint32))
    return on


def _rest_dims(d):
    """spatial coordinates no head k-step covers (hm_rest_begin / hm_rest_end of hm_common.h for the default layout:
    K-slots 32 .. 16 * (k-steps - 1)); a width without a head: its upper half"""
    kc = next(v for v in (2, 4, 8, 13, 14, 16) if v >= (d + 4 + 7) // 8)
    ksteps = (kc + 1) // 2
    if ksteps < 4:
        return np.arange(d // 2, d)
    return np.arange(32, min(16 * (ksteps - 1), d))


def _reproject(X):
    X[:, 0] = np.sqrt(np.float32(1.0) + (X[:, 1:].astype(np.float32) ** 2).sum(axis=1, dtype=np.float32)).astype(np.float32)
    return X


WIDTHS = [(1100, 100), (900, 108), (700, 24)]       # >= three 256-row blocks, 6 - 9 column tiles of 128


@pytest.mark.parametrize("n,d", WIDTHS)
def test_fresh_table_loose_bound(oracle, n, d):
    """a. every group continues at the first search; the merged cluster tightens the bound within a few steps"""
    X = lorentz_table(n, d, seed=300 + d, scale=0.05).numpy()
    _check_table(oracle, X, 0.6)


@pytest.mark.parametrize("n,d", WIDTHS)
def test_exact_duplicate_row(oracle, n, d):
    """b. a pair at distance 0: the bound sits at u = 1 from the tile that holds it on, and zero-distance ties follow"""
    X = lorentz_table(n, d, seed=310 + d, scale=0.05).numpy()
    X[n - 5] = X[17]
    X[300] = X[17]
    _check_table(oracle, X, 0.6)


@pytest.mark.parametrize("n,d", WIDTHS)
def test_nearest_pair_differs_in_rest_dims_only(oracle, n, d):
    """c. the head values of the nearest pair and of its duplicates-in-the-head are equal: only the rest slots order them"""
    X = lorentz_table(n, d, seed=320 + d, scale=0.05).numpy()
    rest = _rest_dims(d)
    rs = np.random.RandomState(d)
    for k, (src, dst) in enumerate([(40, 700 % n), (41, 555), (42, 301)]):
        X[dst] = X[src]
        X[dst, 1 + rest] += (rs.randn(len(rest)) * 0.004 * (k + 1)).astype(np.float32)
    _check_table(oracle, _reproject(X), 0.6)


@pytest.mark.parametrize("n,d", WIDTHS)
def test_nearest_pair_with_zero_head_dims(oracle, n, d):
    """d. rows whose head slots are all zero (the head sum is the time product alone), and rows whose rest slots are zero"""
    X = lorentz_table(n, d, seed=330 + d, scale=0.05).numpy()
    rest = _rest_dims(d)
    head = np.setdiff1d(np.arange(d), rest)
    rs = np.random.RandomState(7 * d)
    base = (rs.randn(len(rest)) * 0.05).astype(np.float32)
    for k, row in enumerate((12, 290, 640)):
        X[row, 1 + head] = 0.0
        X[row, 1 + rest] = base + (rs.randn(len(rest)) * 0.002 * (k + 1)).astype(np.float32)
    for row in (13, 513):
        X[row, 1 + rest] = 0.0
    _check_table(oracle, _reproject(X), 0.6)


@pytest.mark.parametrize("n,d", WIDTHS)
def test_nonfinite_rows_present(oracle, n, d):
    """e. NaN and inf entries in head slots, rest slots and time coordinates: such rows are no candidates and hide nobody"""
    X = lorentz_table(n, d, seed=340 + d, scale=0.05).numpy()
    rest = _rest_dims(d)
    X[5, 1 + rest[0]] = np.nan
    X[260, 3] = np.nan
    X[261, 0] = np.nan
    X[262] = np.nan
    X[400, 1 + rest[1]] = np.inf
    X[401, 2] = -np.inf
    X[400:403, 0] = np.inf
    X[600, 1 + rest] = np.float32(3.0e18)
    X[600, 0] = np.inf
    X[n - 1] = X[n - 2]                    # and a zero-distance pair behind them
    _check_table(oracle, X, 0.6)


@pytest.mark.parametrize("knobs", [{"pipeline_pairs": 0}, {"pipeline": 0}, {"pipeline_pairs": 0, "dyn": 1, "dyn_slots": 8},
                                   {"dyn": 1, "dyn_slots": 5}, {"dyn": 0}])
def test_pipelined_loop_and_item_queue(oracle, knobs):
    """f, g. the pipelined loop forced at this size (both counter sets alternate), the sequential chain, and the item queue
    shrunk to a handful of resident blocks"""
    n, d = 1100, 100
    X = lorentz_table(n, d, seed=77, scale=0.05).numpy()
    X[900] = X[3]
    _check_table(oracle, X, 0.6, knobs)


@pytest.mark.parametrize("n,d", WIDTHS[:2])
def test_project_table_keeps_the_rest_norm(oracle, n, d):
    """h. hm_project_table on a live engine rewrites the time slots of every image row: searches afterwards equal those of
    an engine built from the projected table, with the head test and without"""
    X = lorentz_table(n, d, seed=350 + d, scale=0.07).numpy()
    X[n - 7] = X[30]                       # (after the re-projection below: u = 1 / c < 1, acosh gives NaN, no candidate)
    c = 2.3
    want = X.copy()
    oracle.project_table(want, n, c)
    thr = 0.9
    res = []
    for knobs in ({"head_force": 1}, {"head": 0}, {}):
        eng, table = _engine(X, knobs, extra=STEPS + 8)
        assert eng.argmin(1.0, 0.6) is not None
        eng.project_table(table, n, c)
        assert np.array_equal(table[:n].cpu().numpy().view(np.uint32), want.view(np.uint32))
        a = eng.argmin(c, thr)
        eng.set_token_lengths(_lengths(n))
        recs, done = eng.std_merge_steps(c, thr, table, STEPS)
        res.append((a, recs[:done], table[n:n + done].cpu().numpy().view(np.uint32).copy()))
        fresh, _ = _engine(want, knobs)
        assert fresh.argmin(c, thr) == a
    for other in res[1:]:
        assert res[0][0] == other[0] and res[0][1] == other[1] and np.array_equal(res[0][2], other[2])
    od, oi, oj, oc = oracle.pairwise_topk(want, n, c, float(np.float32(thr)), 1, 1)
    a = res[0][0]
    assert oc > 0 and a is not None and (a[1], a[2]) == (int(oi[0]), int(oj[0])) and _bits([a[0]])[0] == _bits(od[:1])[0]


@pytest.mark.parametrize("n,d", WIDTHS[:2])
def test_other_kernels_see_a_zero_in_the_rest_norm_slot(oracle, n, d):
    """i. top-k on the engine whose argmin runs the head test, and the reference sign (every pair at distance 0 or NaN): the
    kernels that keep a stationary 0 in the fourth time slot return what they return with head = 0, and what the oracle does"""
    X = lorentz_table(n, d, seed=360 + d, scale=0.05).numpy()
    X[n - 3] = X[8]
    out = []
    for knobs in ({"head_force": 1}, {"head": 0}):
        eng, _ = _engine(X, knobs)
        a = eng.argmin(1.0, 0.55)
        gd, gi, gj, gc = eng.topk(1.0, 0.55, 400)
        b = eng.argmin(1.0, 0.5)
        ref, _ = _engine(X, knobs, mode="reference")
        rd, ri, rj, rc = ref.topk(1.0, 0.1, 50)
        out.append((a, b, gc, gi.copy(), gj.copy(), _bits(gd).copy(), ref.argmin(1.0, 0.1), rc, ri.copy(), rj.copy(), _bits(rd).copy()))
    for x, y in zip(out[0], out[1]):
        assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y
    od, oi, oj, oc = oracle.pairwise_topk(X, n, 1.0, float(np.float32(0.55)), 1, 400)
    assert out[0][2] == oc and np.array_equal(out[0][3], oi) and np.array_equal(out[0][4], oj) and np.array_equal(out[0][5], _bits(od))
    qd, qi, qj, qc = oracle.pairwise_topk(X, n, 1.0, float(np.float32(0.1)), 0, 50)
    assert out[0][7] == qc and np.array_equal(out[0][8], qi) and np.array_equal(out[0][9], qj) and np.array_equal(out[0][10], _bits(qd))


def test_wide_key_engine(oracle):
    """an engine for more than 131 072 rows keeps a wide running key (the WK instantiations of the head kernels): same
    searches and the same loop as the narrow-key engine of the same table, as head = 0, and as the oracle"""
    n, d = 1100, 100
    X = lorentz_table(n, d, seed=91, scale=0.05).numpy()
    X[1000] = X[44]
    wide = 140000 - n
    runs = []
    for knobs in ({"head_force": 1}, {"head": 0}, {}):
        eng, table = _engine(X, knobs, extra=wide)
        first = eng.argmin(1.0, 0.6)
        eng.set_token_lengths(_lengths(n))
        recs, done = eng.std_merge_steps(1.0, 0.6, table, STEPS)
        runs.append((first, recs[:done], table[n:n + done].cpu().numpy().view(np.uint32).copy()))
    for other in runs[1:]:
        assert runs[0][0] == other[0] and runs[0][1] == other[1] and np.array_equal(runs[0][2], other[2])
    pairs, dist, rows = _oracle_loop(oracle, X, 0.6, STEPS, _lengths(n))
    assert [tuple(r[2:]) for r in runs[0][1]] == pairs and [_bits([r[1]])[0] for r in runs[0][1]] == dist
    assert np.array_equal(runs[0][2], rows.view(np.uint32))


def test_head_knob_values():
    from hyptokenizer_amd import _lib
    from hyptokenizer_amd.engine import MergeEngine
    L = _lib.load()
    eng = MergeEngine(256, 101, "lorentz", prefilter="bf16")
    assert L.hm_debug_set_knob(eng._h, b"head", 0.0) == 0
    assert L.hm_debug_set_knob(eng._h, b"head", 3.0) == 0
    assert L.hm_debug_set_knob(eng._h, b"head", 7.0) != 0
