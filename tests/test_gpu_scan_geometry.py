"""GPU: search results do not depend on the geometry of the pair scan's item list (hm_scan_plan.h).

The knobs that shape the list -- `phases`, `tail`, `tail_div`, `ph_share*`, `chunk` -- and the two ways of handing it out
(one block per item, `dyn = 0`; a resident grid drawing items from the queue, here shrunk to 8 blocks) are set through
hm_debug_set_knob on tables of the smallest sizes at which the default knobs produce a multi-phase list: 16 640 rows in the
bf16 form with 256-row blocks (and once more with 512-row blocks, one phase) and 12 032 rows in the fp32 form.  Every
geometry runs the same searches -- whole-table argmin, argmin over a row range, top-64 with its exact count, and the top-64
after 40 appended rows (the incremental refresh: a scan with col_begin > 0) -- and every returned array must equal, bit for
bit, what the default geometry returns, which in turn must equal the oracle's.  (`emitted` counts may differ between
geometries and are not compared.)"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from hyptokenizer_amd.synthetic import lorentz_table  # noqa: E402

K, APPENDED, RANGE = 64, 40, (3000, 9000)

# form -> (rows, d, sign convention, oracle's sign mode, prefilter, knobs of the form)
FORMS = {
    "bf16-256": (16640, 32, "lorentz", 1, "bf16", {}),
    "bf16-512": (16640, 32, "lorentz", 1, "bf16", {"big_rows": 2}),
    "f32": (12032, 8, "reference", 0, "f32", {}),
}
GEOMETRIES = {
    "default": {},
    "one phase": {"phases": 1},
    "two phases, half the work at chunk / 16": {"phases": 2, "tail": 0.5, "tail_div": 16},
    "six phases": {"phases": 6, "ph_share0": 0.3, "ph_share1": 0.2, "ph_share2": 0.2, "ph_share3": 0.1, "ph_share4": 0.1},
    "chunk 8": {"chunk": 8},
    "chunk 4096": {"chunk": 4096},
}
QUEUES = {"static grid": {"dyn": 0}, "queue of 8": {"dyn": 1, "dyn_slots": 8}}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


_tables, _defaults = {}, {}


def _table(oracle, form):
    """the table of a form (with the rows appended later behind it), the threshold and the oracle's four answers; built once"""
    n, d, _, sign, _, _ = FORMS[form]
    key = (n, d, sign)
    if key in _tables:
        return _tables[key]
    X = lorentz_table(n + APPENDED, d, seed=500 + d, scale=0.05).numpy()
    rs = np.random.RandomState(d)

    def near(dst, src, eps):
        X[dst, 1:] = X[src, 1:] + (rs.randn(d) * eps).astype(np.float32)
        X[dst, 0] = np.sqrt(np.float32(1.0) + (X[dst, 1:] ** 2).sum(dtype=np.float32))

    X[n - 5] = X[17]                                   # a duplicated row: the nearest pair, at distance 0
    near(7001, 3500, 1e-3)                             # a planted near pair inside the row range
    for t in range(APPENDED):                          # the appended rows: each close to a row of the table
        near(n + t, 5000 + 7 * t, 2e-3 * (1 + t % 5))
    if sign:
        # One oracle call about the grown table under a threshold that admits everything: its list without the pairs of an
        # appended row is the list of the table itself.  The threshold is that list's 301st distance -- a few hundred
        # candidates --, so both lists, cut there, hold every answer about the whole table.
        ad, ai, aj, _ = oracle.pairwise_topk(X, n + APPENDED, 1.0, 10.0, sign, 800)
        old = aj < n
        assert int(old.sum()) >= 400
        thr = float(ad[old][300])
        cnt = int((ad[old] < np.float32(thr)).sum())
        assert 200 <= cnt <= 300 and int((ad < np.float32(thr)).sum()) < 800
        whole = (ad[old][:K], ai[old][:K], aj[old][:K], cnt)
        grown = (ad[:K], ai[:K], aj[:K])
    else:
        thr = 0.1                                      # the literal sign mode: every pair is at distance 0
        whole = oracle.pairwise_topk(X, n, 1.0, thr, sign, K)
        grown = oracle.pairwise_topk(X, n + APPENDED, 1.0, thr, sign, K)
    ranged = oracle.pairwise_topk(X, n, 1.0, thr, sign, 1, RANGE[0], RANGE[1])
    _tables[key] = (X, thr, whole, ranged, grown)
    return _tables[key]


def _search(oracle, form, knobs):
    """the four searches on a fresh engine with these knobs -> everything they returned"""
    from hyptokenizer_amd import _lib
    from hyptokenizer_amd.engine import MergeEngine
    L = _lib.load()
    n, d, mode, _, prefilter, form_knobs = FORMS[form]
    X, thr = _table(oracle, form)[:2]
    table = torch.from_numpy(X).cuda()
    eng = MergeEngine(n + APPENDED + 24, d + 1, mode, prefilter=prefilter)
    for name, v in dict(form_knobs, **knobs).items():
        _lib.check(L.hm_debug_set_knob(eng._h, name.encode(), float(v)))
    eng.set_table(table, n)
    whole = eng.argmin(1.0, thr)
    ranged = eng.argmin(1.0, thr, RANGE[0], RANGE[1])
    td, ti, tj, tc = eng.topk(1.0, thr, K)
    eng.update_rows(table, n, n + APPENDED)
    assert eng.n == n + APPENDED
    # the incremental route: its scan starts at col_begin = n.  (The literal sign mode's list is a tie flood cut by rows, which
    # no refresh extends: there the engine answers "not applicable" and the whole table is searched again.)
    incremental = eng.topk_refresh_begin(1.0, thr, K)
    assert incremental == (mode == "lorentz")
    r = eng.topk_refresh_end() if incremental else eng.topk(1.0, thr, K, count=False)[:3]
    assert r is not None
    eng.close()
    return (whole, ranged, tc, ti.copy(), tj.copy(), _bits(td).copy(), r[1].copy(), r[2].copy(), _bits(r[0]).copy())


def _default(oracle, form, queue):
    if (form, queue) not in _defaults:
        _defaults[(form, queue)] = _search(oracle, form, QUEUES[queue])
    return _defaults[(form, queue)]


def _same(a, b):
    return all(np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y for x, y in zip(a, b))


def _rec(od, oi, oj):
    return (_bits(od[:1])[0], int(oi[0]), int(oj[0]))


@pytest.mark.parametrize("queue", list(QUEUES))
@pytest.mark.parametrize("form", list(FORMS))
def test_default_geometry_equals_the_oracle(oracle, form, queue):
    X, thr, whole, ranged, grown = _table(oracle, form)
    got = _default(oracle, form, queue)
    assert got[0] is not None and (_bits([got[0][0]])[0], got[0][1], got[0][2]) == _rec(*whole[:3])
    assert got[1] is not None and (_bits([got[1][0]])[0], got[1][1], got[1][2]) == _rec(*ranged[:3])
    assert got[2] == whole[3] and np.array_equal(got[3], whole[1]) and np.array_equal(got[4], whole[2])
    assert np.array_equal(got[5], _bits(whole[0])) and len(got[3]) == K
    assert np.array_equal(got[6], grown[1]) and np.array_equal(got[7], grown[2]) and np.array_equal(got[8], _bits(grown[0]))
    if FORMS[form][3]:
        n = FORMS[form][0]
        assert (got[0][1], got[0][2]) == (17, n - 5) and (got[1][1], got[1][2]) == (3500, 7001)
        assert int((got[7] >= n).sum()) >= 10          # the appended rows changed the list


@pytest.mark.parametrize("queue", list(QUEUES))
@pytest.mark.parametrize("geometry", [g for g in GEOMETRIES if g != "default"])
@pytest.mark.parametrize("form", list(FORMS))
def test_results_do_not_depend_on_the_list_geometry(oracle, form, geometry, queue):
    want = _default(oracle, form, queue)
    got = _search(oracle, form, dict(GEOMETRIES[geometry], **QUEUES[queue]))
    assert _same(got, want), (form, geometry, queue)


def test_knob_ranges():
    from hyptokenizer_amd import _lib
    from hyptokenizer_amd.engine import MergeEngine
    L = _lib.load()
    eng = MergeEngine(256, 33, "lorentz", prefilter="bf16")
    for name, ok, bad in (("chunk", (4, 4096), (3, 4097)), ("tail", (0.0, 0.9), (-0.1, 0.95)), ("tail_div", (1, 16), (0, 17)),
                          ("phases", (1, 6), (0, 7)), ("ph_share4", (0.0, 1.0), (-0.1, 1.1)), ("ph_div5", (1, 64), (0, 65)),
                          ("shape", (-1, 4), (-2, 5)), ("big_rows", (0, 1 << 20), (-1,))):
        for v in ok:
            assert L.hm_debug_set_knob(eng._h, name.encode(), float(v)) == 0, (name, v)
        for v in bad:
            assert L.hm_debug_set_knob(eng._h, name.encode(), float(v)) != 0, (name, v)
    assert L.hm_debug_set_knob(eng._h, b"ph_share5", 0.1) != 0 and L.hm_debug_set_knob(eng._h, b"ph_div0", 2.0) != 0
