"""The engine walks of tests/engine_walk.py, without a GPU.

The walks exist for the HIP engine (tests/test_gpu_engine_walk.py).  Here the same traces are checked for what does not
need one: the generator never leaves the contract of include/hypmerge.h (``_Gen.do`` asserts it call by call while the
trace is built), a seed gives the same calls twice, a long-lived ``OracleEngine`` answers like the model that is rebuilt
from the table before every probe, the walks reach the transitions they exist for, and the driver notices a subject
that keeps a stale seed.  The conditions below are conditions on the walk, not on the engine under test.
"""
import numpy as np
import pytest

import engine_walk as W
from helpers import OracleEngine

WALKS = [(seed, n0, d, mode) for (seed, n0, d) in W.SHAPES for mode in ("lorentz", "reference")]
# the literal sign mode makes every pair a candidate: its largest walk costs the oracle 14 s per replay, so that one is
# generated and checked for its coverage here, and replayed on the GPU only
REPLAYED = [w for w in WALKS if w[1:] != (2040, 100, "reference")]


@pytest.mark.parametrize("seed,n0,d,mode", WALKS)
def test_walk_reaches_the_transitions_it_exists_for(oracle, seed, n0, d, mode):
    trace = W.build_trace(seed, n0, d, mode)
    cover = trace.cover
    assert all(cover["motifs"][kind] >= 2 for kind in W.MOTIFS), cover["motifs"]
    assert 20 <= sum(cover["motifs"].values()) <= 30
    assert cover["d_probes_grown"] >= 6                       # refreshes of a table that grew since the list
    assert cover["cross64"] >= 3 and cover["cross256"] >= 1   # ... whose appends cross the scan's tile edges
    assert cover["A"] == set(W.A_KINDS)
    assert cover["B"] == set(W.B_KINDS)
    assert cover["C"] == set(W.C_KINDS)
    assert cover["E"] == set(W.E_KINDS)
    assert cover["G"] == set(W.G_KINDS)
    assert cover["K"] == set(W.K_KINDS)
    assert cover["steps_merged"] >= 6                         # the device loops merged something
    # every D probe really sees more rows than its list did, and every appending motif stayed inside the table
    n_at = {}
    for st in trace.steps:
        if st.want is not None:
            assert st.want[0] <= trace.max_rows
        if st.op == "topk" and st.role == "setup" and st.motif.startswith("D"):
            n_at[st.motif] = st.want[0]
        if st.op == "refresh" and st.args["grown"]:
            assert st.want[0] > n_at[st.motif]
            assert len(st.want[1][0]) == st.args["k"]         # the list is full: the refresh is of the incremental kind


@pytest.mark.parametrize("seed,n0,d,mode", REPLAYED)
def test_long_lived_oracle_engine_equals_the_rebuilt_model(oracle, seed, n0, d, mode):
    trace = W.build_trace(seed, n0, d, mode)
    side = W.run_trace(trace, W.oracle_side(trace.max_rows, d + 1, mode))
    assert side.eng.n == [st.want[0] for st in trace.steps if st.want is not None][-1]
    assert len(side.refreshes) == sum(st.op == "refresh" for st in trace.steps)


@pytest.mark.parametrize("mode", ["lorentz", "reference"])
def test_a_seed_gives_the_same_calls_twice(oracle, mode):
    seed, n0, d = W.SHAPES[0]
    a = W._Gen(seed, n0, d, mode).build()
    b = W._Gen(seed, n0, d, mode, rebuild_model=False).build()       # ... whether or not the model is rebuilt
    assert len(a.steps) == len(b.steps)
    for x, y in zip(a.steps, b.steps):
        assert (x.motif, x.role, x.op, sorted(x.args)) == (y.motif, y.role, y.op, sorted(y.args))
        assert all(W.same(x.args[k], y.args[k], nan_by_position=False) for k in x.args), W.fmt_step(x)
        assert (x.want is None) == (y.want is None) and (x.want is None or W.same(x.want, y.want, nan_by_position=False)), W.fmt_step(x)
    other = W._Gen(seed + 1, n0, d, mode).build()
    assert [s.op for s in other.steps] != [s.op for s in a.steps]


class _StaleSeedEngine(OracleEngine):
    """an engine with the defect the walks look for: the nearest pair of the last whole-table search is kept as a bound
    for the next one -- and an overwrite of an existing row forgets to drop it"""
    _seed = None

    def set_table(self, table, n_rows):
        self._seed = None
        super().set_table(table, n_rows)

    def truncate(self, n_rows):
        self._seed = None
        super().truncate(n_rows)

    def project_table(self, table, n_rows, c):
        self._seed = None
        super().project_table(table, n_rows, c)

    def merge_append(self, i, j, w, c, table, new_row):
        if new_row < self._n:
            self._seed = None
        super().merge_append(i, j, w, c, table, new_row)

    def argmin(self, c, thr, row_begin=0, row_end=-1):
        hit = super().argmin(c, thr, row_begin, row_end)
        if row_begin != 0 or row_end != -1:
            return hit
        if self._seed is not None and self._seed[0] == c:
            old = self._seed[1]
            if old[0] < np.float32(thr) and (hit is None or old < hit):
                hit = old                                            # the stale bound wins
        self._seed = (c, hit) if hit is not None else None
        return hit


def test_driver_notices_a_stale_seed(oracle):
    seed, n0, d = W.SHAPES[0]
    trace = W.build_trace(seed, n0, d, "lorentz")
    side = W.Side(_StaleSeedEngine(trace.max_rows, d + 1, "lorentz"), W.oracle_side(trace.max_rows, d + 1, "lorentz").table, refuses=False)
    with pytest.raises(W.WalkMismatch) as err:
        W.run_trace(trace, side)
    msg = str(err.value)
    assert f"seed={seed}" in msg and "(motif " in msg and "replay: engine_walk.replay(" in msg and msg.count("\n    #") == 12
    # the prefix before the failing call replays clean
    upto = int(msg.split("at call #")[1].split()[0])
    W.replay(seed, n0, d, "lorentz", upto=upto)
