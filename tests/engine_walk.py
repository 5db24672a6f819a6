"""Random edit / search walks over the ``MergeEngine`` interface (no GPU import).

``MergeEngine`` carries state between calls: the armed counters and the seed of the last argmin, the cut prediction
and the previous ordered list of the incremental top-k refresh, the per-table route memories, norm bounds that only
rise, the token lengths of the device loops.  Every entry point has to reset exactly the right subset.
A walk is a seeded sequence of *motifs* -- "set up, perturb, probe" -- that steps through those transitions:

    A  armed argmin survives every kind of read          F  margin blown up by a far row, and back
    B  seed kept across appends                          G  NaN row, tie flood and a gap in a live table
    C  seed dropped by an edit                           H  device-resident loops between searches
    D  refresh of a grown table                          K  refused calls change nothing
    E  refresh state voided

``build_trace`` generates the walk on a *model* (``helpers.OracleEngine``, rebuilt from the table before every probe so
that it cannot carry state of its own) and records every call with the model's answer.  All decisions -- thresholds
from quantiles of sampled model distances, operand rows, the nearest pair -- come from the model; the subject is never
read, so a wrong engine cannot steer the walk and every subject executes the same calls.  ``run_trace`` applies a trace
to a subject and compares every observable after every call.  All calls stay inside the contract of include/hypmerge.h
(``check_contract``); the refused calls of motif K are the exception by design.
"""
from __future__ import annotations

import functools
from collections import Counter
from dataclasses import dataclass, field
from typing import Callable, Optional

import numpy as np
import torch

from helpers import OracleEngine, bits

EXTRA_ROWS = 400                 # max_rows = n0 + EXTRA_ROWS
MAX_K = 65536                    # hm_pairwise_topk: largest k
CURVATURES = (1.0, 0.7, 2.5)
MOTIFS = "ABCDEFGHK"
A_KINDS = ("row_argmin", "topk_counted", "topk_ranged", "candidates", "count", "pair_distance", "midpoint", "argmin_into",
           "argmin_other")
B_KINDS = ("merge_append", "batch_chain", "batch_independent", "update_rows")
C_KINDS = ("overwrite_pair_end", "merge_into_existing", "truncate", "project_table", "set_table_other_count", "set_prefilter")
E_KINDS = ("overwrite", "truncate", "project_table", "ranged_topk", "set_prefilter", "other_c", "other_k", "smaller_thr")
G_KINDS = ("nan_row", "tie_flood", "gap")
K_KINDS = ("merge_operand", "truncate_beyond", "update_past_max", "batch_first_row", "refresh_end_idle", "k_too_large")
SCHEDULE = "AA" "BB" "CCC" "DDDD" "EEEE" "FF" "GG" "HHH" "KK"       # 25 motifs, shuffled per seed
MEMO_OPS = {"argmin", "argmin_into", "topk", "count"}       # whole answers the generator may reuse while no row changes
WRITES = {"set_table", "update_rows", "merge_append", "merge_batch", "truncate", "project_table", "std_steps", "incr_steps"}


# ----------------------------------------------------------------------------------------------------------
# one side of the comparison: an object with the MergeEngine interface and the table it writes merges into
# ----------------------------------------------------------------------------------------------------------
class Side:
    def __init__(self, eng, table: torch.Tensor, refuses: bool, form: str = "f32", close: Optional[Callable] = None):
        self.eng, self.table = eng, table
        self.refuses = refuses               # the engine checks its arguments itself (motif K applies to it)
        self.form = form                     # prefilter form in force ("f32" | "bf16"): set_prefilter flips it
        self.refreshes = []                  # per refresh probe: did the engine take the incremental route
        self.host_steps = 0                  # loop steps that went through the host path (record found = 2)
        self._close = close

    def close(self):
        if self._close is not None:
            self._close()


def oracle_side(max_rows: int, d1: int, mode: str, form: str = "f32") -> Side:
    return Side(OracleEngine(max_rows, d1, mode), torch.zeros((max_rows, d1), dtype=torch.float32), refuses=False, form=form)


def _rec(hit):
    return (0, 0, -1, -1) if hit is None else (1, int(bits([hit[0]])[0]), int(hit[1]), int(hit[2]))


def _put(side: Side, r0: int, rows: np.ndarray):
    side.table[r0:r0 + rows.shape[0]] = torch.from_numpy(rows).to(side.table.device)


def _loop(side: Side, kind: str, a: dict):
    """``steps`` iterations of a device-resident loop; a record with found = 2 (emission overflow at that step) goes
    through the host path, as a caller of hm_std_merge_steps has to do it."""
    e, T = side.eng, side.table
    c, thr, left = a["c"], a["thr"], a["steps"]
    lens = list(a["lens"])
    n0 = e.n
    merged, status = [], 1
    best = a.get("best")
    while left > 0:
        if kind == "std":
            recs, done = e.std_merge_steps(c, thr, T, left)
        else:
            recs, done, best = e.incr_merge_steps(c, thr, T, left, best)
        for r in recs[:done]:
            merged.append((int(bits([r[1]])[0]), int(r[2]), int(r[3])))
            lens.append(lens[r[2]] + lens[r[3]])
        left -= done
        if left == 0:
            break
        status = int(recs[done][0])
        if status != 2:
            break
        hit = e.argmin(c, thr)
        if hit is None:
            status = 0
            break
        li, lj = lens[hit[1]], lens[hit[2]]
        e.merge_append(hit[1], hit[2], lj / (li + lj), c, T, e.n)
        lens.append(li + lj)
        e.set_token_lengths(lens)
        merged.append(_rec(hit)[1:])
        side.host_steps += 1
        left -= 1
        status = 1
        if kind == "incr":
            best = e.argmin(c, thr)
            if best is None and left > 0:
                status = 0
                break
    out = (status, merged, T[n0:e.n].cpu().numpy().copy())
    return out + (_rec(best),) if kind == "incr" else out


def _refused(side: Side, a: dict):
    """one call outside the contract: the engine has to raise (HypMergeError, or the wrapper's own ValueError / RuntimeError)"""
    e, T, n = side.eng, side.table, side.eng.n
    kind = a["kind"]
    calls = {
        "merge_operand": lambda: e.merge_append(n, 0, 0.5, 1.0, T, n),
        "truncate_beyond": lambda: e.truncate(n + 1),
        "update_past_max": lambda: e.update_rows(T, e.max_rows - 1, e.max_rows + 1),
        "batch_first_row": lambda: e.merge_append_batch(np.array([0, 1], np.int32), np.array([2, 3], np.int32),
                                                        np.array([0.5, 0.5], np.float32), 1.0, T, n + 1),
        "refresh_end_idle": lambda: e.topk_refresh_end(),
        "k_too_large": lambda: e.topk(1.0, a["thr"], MAX_K + 1),
    }
    call = calls[kind]
    try:
        call()
    except Exception as ex:
        return type(ex).__name__
    raise WalkMismatch(f"refused call {kind!r} was accepted")


def apply(side: Side, op: str, a: dict):
    """Run one call on one side -> (live rows afterwards, observable result)."""
    e, T = side.eng, side.table
    out = ()
    if op == "set_table":
        m = a["rows"].shape[0]
        _put(side, 0, a["rows"])
        T[m:] = 0
        e.set_table(T, m)
    elif op == "update_rows":
        _put(side, a["r0"], a["rows"])
        e.update_rows(T, a["r0"], a["r0"] + a["rows"].shape[0])
    elif op == "argmin":
        out = _rec(e.argmin(a["c"], a["thr"], a["rb"], a["re"]))
    elif op == "argmin_into":
        rec = torch.zeros(4, dtype=torch.int32, device=T.device)
        e.argmin_into(a["c"], a["thr"], a["rb"], a["re"], rec)
        if T.is_cuda:
            torch.cuda.synchronize()
        r = rec.tolist()
        if r[0] == 2:                        # emission overflow: "use argmin"
            out = _rec(e.argmin(a["c"], a["thr"], a["rb"], a["re"]))
        else:
            out = (1, r[1] & 0xFFFFFFFF, r[2], r[3]) if r[0] == 1 else (0, 0, -1, -1)
    elif op == "row_argmin":
        out = _rec(e.row_argmin(a["row"], a["partners"], a["c"], a["thr"]))
    elif op == "topk":
        d, i, j, total = e.topk(a["c"], a["thr"], a["k"], a["rb"], a["re"], count=a["count"])
        out = (int(total), np.array(i), np.array(j), bits(d).copy())
    elif op == "refresh":
        ok = e.topk_refresh_begin(a["c"], a["thr"], a["k"])
        r = e.topk_refresh_end() if ok else None
        side.refreshes.append((bool(ok and r is not None), bool(a["grown"])))
        if r is None:
            r = e.topk(a["c"], a["thr"], a["k"], count=False)[:3]
        out = (np.array(r[1]), np.array(r[2]), bits(r[0]).copy())
    elif op == "candidates":
        i, j, d, total = e.candidates(a["c"], a["thr"], a["rb"], a["re"])
        out = (int(total), np.array(i), np.array(j), bits(d).copy())
    elif op == "count":
        out = int(e.count_candidates(a["c"], a["thr"], a["n_limit"]))
    elif op == "pair_distance":
        out = np.array(e.pair_distance(a["I"], a["J"], a["c"]), np.float32)
    elif op == "midpoint":
        out = e.midpoint(a["I"], a["J"], a["W"], a["c"]).cpu().numpy().copy()
    elif op == "merge_append":
        e.merge_append(a["i"], a["j"], a["w"], a["c"], T, a["new_row"])
        out = T[a["new_row"]].cpu().numpy().copy()
    elif op == "merge_batch":
        e.merge_append_batch(a["I"], a["J"], a["W"], a["c"], T, a["first_row"], independent=a["independent"])
        out = T[a["first_row"]:a["first_row"] + len(a["I"])].cpu().numpy().copy()
    elif op == "truncate":
        e.truncate(a["n_rows"])
        T[a["n_rows"]:] = 0
    elif op == "project_table":
        e.project_table(T, a["n_rows"], a["c"])
        out = T[:a["n_rows"], 0].cpu().numpy().copy()
    elif op == "set_prefilter":
        side.form = "bf16" if side.form == "f32" else "f32"
        e.set_prefilter(side.form)
    elif op == "set_lens":
        e.set_token_lengths(a["lens"])
    elif op == "std_steps":
        out = _loop(side, "std", a)
    elif op == "incr_steps":
        out = _loop(side, "incr", a)
    elif op == "refused":
        if side.refuses:
            _refused(side, a)
    else:
        raise ValueError(op)
    return int(e.n), out


def same(a, b, nan_by_position: bool = True) -> bool:
    """Bit equality of two observables.  Every float that is a number is compared by its bits.  A NaN has to sit in the same
    place on both sides and is not compared further: IEEE 754 leaves the sign and payload of a NaN result to the
    implementation, and x86 and gfx950 choose differently (a negated NaN is 0xffc00000 on one and 0x7fc00000 on the
    other, and the other way round after an invalid operation) -- 149 merged, midpoint and projected rows of the GPU walks
    differed from the oracle's in nothing but that.  No search can observe it: a NaN is never a candidate.
    ``nan_by_position=False`` asks for the NaN's bits as well (two runs on one machine)."""
    if isinstance(a, (tuple, list)):
        return isinstance(b, (tuple, list)) and len(a) == len(b) and all(same(x, y, nan_by_position) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        if not isinstance(b, np.ndarray) or a.shape != b.shape:
            return False
        if a.dtype == np.float32:
            if nan_by_position:
                na, nb = np.isnan(a), np.isnan(b)
                return bool(np.array_equal(na, nb) and np.array_equal(bits(a[~na]), bits(b[~nb])))
            return bool(np.array_equal(bits(a), bits(b)))
        return bool(np.array_equal(a, b))
    return a == b


# ----------------------------------------------------------------------------------------------------------
# the contract of include/hypmerge.h, as far as the walk uses it
# ----------------------------------------------------------------------------------------------------------
def contract_violation(op: str, a: dict, n: int, max_rows: int, have_lens: bool) -> Optional[str]:
    def rows_ok(*idx):
        return all(0 <= int(v) < n for x in idx for v in np.atleast_1d(x))
    if "c" in a and not a["c"] > 0:
        return "curvature must be > 0"
    if op == "set_table":
        return None if a["rows"].shape[0] <= max_rows else "n_rows > max_rows"
    if op == "update_rows":
        return None if 0 <= a["r0"] and a["r0"] + a["rows"].shape[0] <= max_rows else "rows outside [0, max_rows]"
    if op in ("argmin", "argmin_into", "topk", "candidates"):
        if a["rb"] < 0:
            return "row_begin < 0"
        return "k outside [0, 65536]" if op == "topk" and not 0 <= a["k"] <= MAX_K else None
    if op == "refresh":
        return None if 0 < a["k"] <= MAX_K else "k outside [1, 65536]"
    if op == "row_argmin":
        return None if rows_ok(a["row"]) and 0 <= a["partners"] <= n else "row / partners outside the live rows"
    if op in ("pair_distance", "midpoint"):
        return None if rows_ok(a["I"], a["J"]) else "operand outside the live rows"
    if op == "merge_append":
        return None if rows_ok(a["i"], a["j"]) and 0 <= a["new_row"] < max_rows else "operand >= n or new_row outside the table"
    if op == "merge_batch":
        cnt = len(a["I"])
        if not (0 <= a["first_row"] <= n and a["first_row"] + cnt <= max_rows and cnt <= 4096):
            return "first_row beyond the live rows / batch outside the table"
        for t in range(cnt):
            lim = a["first_row"] if a["independent"] else a["first_row"] + t
            if not (0 <= a["I"][t] < lim and 0 <= a["J"][t] < lim):
                return "a merge reads a row that does not exist yet"
        return None
    if op == "truncate":
        return None if 0 <= a["n_rows"] <= n else "n_rows outside [0, live rows]"
    if op == "project_table":
        return None if n <= a["n_rows"] <= max_rows else "n_rows must cover the live rows"
    if op == "set_lens":
        return None if len(a["lens"]) <= max_rows else "more lengths than rows"
    if op in ("std_steps", "incr_steps"):
        if not have_lens or len(a["lens"]) != n:
            return "token lengths not set for the live rows"
        return None if 0 <= a["steps"] <= 256 and n + a["steps"] <= max_rows else "the table cannot take that many rows"
    if op == "refused":
        return {"merge_operand": "operand >= n", "truncate_beyond": "n_rows > live rows", "update_past_max": "row_end > max_rows",
                "batch_first_row": "first_row beyond the live rows", "refresh_end_idle": "no refresh pending",
                "k_too_large": "k > 65536"}[a["kind"]]
    return None


# ----------------------------------------------------------------------------------------------------------
# trace
# ----------------------------------------------------------------------------------------------------------
@dataclass
class Step:
    index: int
    motif: str               # "D3": fourth motif of the walk is a D ...; "-": filler
    role: str                # setup | perturb | check | probe (the motif's probe: compared with a fresh engine) | trio | filler
    op: str
    args: dict
    want: Optional[tuple]    # (n, observable) of the model; None: a trio call, compared with a fresh engine only


@dataclass
class Trace:
    seed: int
    n0: int
    d: int
    mode: str
    steps: list = field(default_factory=list)
    cover: dict = field(default_factory=dict)

    @property
    def max_rows(self):
        return self.n0 + EXTRA_ROWS


def _fmt_val(v):
    if isinstance(v, np.ndarray):
        head = np.array2string(v.ravel()[:4], precision=6, separator=",")
        return f"array{v.shape}{head}"
    if isinstance(v, list) and len(v) > 6:
        return f"list[{len(v)}]{v[:4]}"
    if isinstance(v, float):
        return repr(float(np.float32(v))) if abs(v) < 1e30 else repr(v)
    return repr(v)


def fmt_step(st: Step) -> str:
    return f"#{st.index} [{st.motif}/{st.role}] {st.op}(" + ", ".join(f"{k}={_fmt_val(v)}" for k, v in st.args.items()) + ")"


def _describe(x, limit=6):
    if isinstance(x, tuple):
        return "(" + ", ".join(_describe(v, limit) for v in x) + ")"
    if isinstance(x, np.ndarray):
        flat = x.ravel()
        body = np.array2string(bits(flat[:limit]) if x.dtype == np.float32 else flat[:limit], separator=",")
        return f"{x.dtype}{x.shape}{body}"
    if isinstance(x, list) and len(x) > limit:
        return f"list[{len(x)}]{x[:limit]}"
    return repr(x)


def _diff_summary(want, got) -> str:
    """where two observables differ: for float arrays the number of differing elements, how many of those are NaN on both
    sides (sign / payload only) and the first one that is not"""
    if isinstance(want, (tuple, list)) and isinstance(got, (tuple, list)) and len(want) == len(got):
        return "".join(_diff_summary(w, g) for w, g in zip(want, got))
    if isinstance(want, np.ndarray) and isinstance(got, np.ndarray) and want.shape == got.shape and want.dtype == np.float32 == got.dtype:
        bw, bg = bits(want).ravel(), bits(got).ravel()
        bad = np.nonzero(bw != bg)[0]
        if len(bad) == 0:
            return ""
        both_nan = np.isnan(want.ravel()[bad]) & np.isnan(got.ravel()[bad])
        out = f"\n  {len(bad)} of {bw.size} floats differ, {int(both_nan.sum())} of them NaN on both sides"
        rest = bad[~both_nan]
        if len(rest):
            t = int(rest[0])
            out += f"; first other difference at flat index {t}: want {int(bw[t]):#010x} ({want.ravel()[t]!r}) got {int(bg[t]):#010x} ({got.ravel()[t]!r})"
        return out
    return ""


class WalkMismatch(AssertionError):
    pass


def _message(trace: Trace, st: Step, what: str, want, got) -> str:
    last = "\n    ".join(fmt_step(s) for s in trace.steps[max(0, st.index - 11):st.index + 1])
    return (f"engine walk seed={trace.seed} n0={trace.n0} d={trace.d} mode={trace.mode}: {what} at call #{st.index} "
                       f"(motif {st.motif}, {st.role}, {st.op})\n  want {_describe(want)}\n  got  {_describe(got)}{_diff_summary(want, got)}\n"
                       f"  replay: engine_walk.replay({trace.seed}, {trace.n0}, {trace.d}, {trace.mode!r}, form, upto={st.index + 1})\n"
            f"  last calls:\n    {last}")


def _fail(trace: Trace, st: Step, what: str, want, got):
    raise WalkMismatch(_message(trace, st, what, want, got))


def _first_difference(want, got):
    """the first (i, j) of two top-k / candidate lists that differ: what DESIGN.md 5.7a asks to evaluate in float64"""
    try:
        wi, wj, gi, gj = want[-3], want[-2], got[-3], got[-2]
        m = min(len(wi), len(gi))
        bad = np.nonzero((wi[:m] != gi[:m]) | (wj[:m] != gj[:m]) | (want[-1][:m] != got[-1][:m]))[0]
        if len(bad):
            t = int(bad[0])
            return f" first difference at entry {t}: want ({wi[t]}, {wj[t]}, {want[-1][t]:#x}) got ({gi[t]}, {gj[t]}, {got[-1][t]:#x})"
    except Exception:
        pass
    return ""


def run_trace(trace: Trace, side: Side, fresh: Optional[Callable[[Side], Side]] = None, upto: Optional[int] = None,
              keep_going: int = 0) -> Side:
    """Apply the trace to ``side`` and compare n and every observable with the model's after every call.  ``fresh(side)``
    builds a new engine from the subject's current table (set_table): at every probe the probing search, and the trio of
    argmin / top-k / count that follows a motif's last probe, are compared with it as well.  ``keep_going``: that many
    mismatches are collected before the walk stops (a look at everything a defect touches; the calls themselves do not
    depend on the subject's answers)."""
    f: Optional[Side] = None
    problems = []

    def mismatch(st, what, want, got):
        problems.append(_message(trace, st, what, want, got))
        if len(problems) > keep_going:
            raise WalkMismatch("\n".join(problems))
    try:
        for st in trace.steps[:upto]:
            if st.want is None and fresh is None:
                continue
            try:
                got = apply(side, st.op, st.args)
            except WalkMismatch:
                raise
            except Exception as ex:
                _fail(trace, st, f"{type(ex).__name__}: {ex}", st.want, None)
            if st.want is not None and not same(st.want, got):
                what = "live rows differ" if st.want[0] != got[0] else "result differs from the model" + _first_difference(st.want[1], got[1])
                mismatch(st, what, st.want, got)
            if fresh is None:
                continue
            if st.role == "probe" and st.op in ("argmin", "refresh"):
                if f is not None:
                    f.close()
                f = fresh(side)
                if st.op == "argmin":
                    ref = apply(f, "argmin", st.args)
                else:
                    t = apply(f, "topk", dict(c=st.args["c"], thr=st.args["thr"], k=st.args["k"], rb=0, re=-1, count=False))
                    ref = (t[0], t[1][1:])
                if not same(ref, got):
                    mismatch(st, "result differs from a fresh engine built from the same table" + _first_difference(ref[1], got[1]), ref, got)
            elif st.role == "trio":
                if f is None:
                    f = fresh(side)
                ref = apply(f, st.op, st.args)
                if not same(ref, got):
                    mismatch(st, "result differs from a fresh engine built from the same table" + _first_difference(ref[1], got[1]), ref, got)
            elif f is not None:
                f.close()
                f = None
    finally:
        if f is not None:
            f.close()
    if problems:
        raise WalkMismatch("\n".join(problems))
    return side


# ----------------------------------------------------------------------------------------------------------
# generator
# ----------------------------------------------------------------------------------------------------------
class _Gen:
    def __init__(self, seed: int, n0: int, d: int, mode: str, rebuild_model: bool = True):
        self.rng = np.random.Generator(np.random.PCG64(seed))
        self.n0, self.d, self.d1, self.mode = n0, d, d + 1, mode
        self.trace = Trace(seed, n0, d, mode)
        self.max_rows = self.trace.max_rows
        self.m = oracle_side(self.max_rows, self.d1, mode)
        self.rebuild_model = rebuild_model
        self.motif = "init"
        self.lens = None                     # token lengths of rows [0, n) while they are valid for the device loops
        self._sample = None
        self._memo = {}
        self.cover = dict(motifs=Counter(), A=set(), B=set(), C=set(), E=set(), G=set(), K=set(), d_probes_grown=0, cross64=0, cross256=0,
                          steps_merged=0)
        self.decks = {}

    # -- plumbing ------------------------------------------------------------------------------------------
    @property
    def n(self) -> int:
        return self.m.eng.n

    @property
    def X(self) -> np.ndarray:
        return self.m.eng.X

    def do(self, op: str, role: str = "perturb", **a):
        bad = contract_violation(op, a, self.n, self.max_rows, self.lens is not None)
        assert (bad is not None) == (op == "refused"), (op, bad, self.motif)
        if role == "trio":                   # answered by the subject and a fresh engine alone: the model is not asked
            self.trace.steps.append(Step(len(self.trace.steps), self.motif, role, op, a, None))
            return None
        key = ("argmin" if op == "argmin_into" else op, tuple(sorted(a.items()))) if op in MEMO_OPS else None
        if key is not None and key in self._memo:        # the same search of an unchanged table: the model has no state
            want = self._memo[key]
        else:
            if role in ("probe", "check") and self.rebuild_model:
                self._rebuild()
            want = apply(self.m, op, a)
            if key is not None:
                self._memo[key] = want
        self.trace.steps.append(Step(len(self.trace.steps), self.motif, role, op, a, want))
        if op in WRITES:
            self._sample = None
            self._memo = {}
            if op not in ("std_steps", "incr_steps"):
                self.lens = None
        return want[1]

    def _rebuild(self):
        """a model without a past: a new OracleEngine holding the current table"""
        old = self.m.eng
        new = OracleEngine(self.max_rows, self.d1, self.mode)
        new.set_table(self.m.table, old.n)
        if self.lens is not None:
            new.set_token_lengths(self.lens)
        assert np.array_equal(bits(new.X), bits(old.X))
        self.m.eng = new

    def deck(self, name: str, kinds):
        """the kinds of a motif in a shuffled order, dealt round after round: every kind comes up"""
        if not self.decks.get(name):
            self.decks[name] = [kinds[t] for t in self.rng.permutation(len(kinds))]
        return self.decks[name].pop()

    def rint(self, lo: int, hi: int) -> int:
        """uniform integer in [lo, hi]"""
        return int(self.rng.integers(lo, hi + 1))

    def rows(self, m: int, scale: float = 0.05) -> np.ndarray:
        s = (self.rng.standard_normal((m, self.d)) * scale).astype(np.float32)
        x0 = np.sqrt(np.float32(1.0) + np.sum(s * s, axis=1, dtype=np.float32), dtype=np.float32)
        return np.ascontiguousarray(np.concatenate([x0[:, None], s], axis=1), dtype=np.float32)

    def curvature(self) -> float:
        return float(CURVATURES[self.rint(0, len(CURVATURES) - 1)])

    def thr(self, c: float, target: float) -> float:
        """threshold with about ``target`` candidates in the whole table, from sampled model distances"""
        n = self.n
        if self._sample is None:
            I = self.rng.integers(0, n, 4000)
            J = self.rng.integers(0, n, 4000)
            keep = I != J
            dd = np.asarray(self.m.eng.pair_distance(I[keep], J[keep], 1.0), np.float64)
            self._sample = np.sort(dd[np.isfinite(dd)])
        s = self._sample
        v = 0.0
        if len(s):
            pairs = n * (n - 1) / 2
            v = float(s[min(len(s) - 1, max(3, int(target / pairs * len(s))))]) / float(np.sqrt(c))
        if not v > 0.0:
            v = 0.1                          # (the literal sign mode: every distance is 0)
        return float(np.float32(v))

    def room(self, need: int):
        """make sure ``need`` more rows fit the table"""
        if self.n + need > self.max_rows - 4:
            self.do("truncate", n_rows=min(self.n, self.rint(self.n0 - 30, self.n0 + 30)))

    def goto(self, target: int):
        if self.n > target:
            self.do("truncate", role="setup", n_rows=target)
        elif self.n < target:
            self.do("update_rows", role="setup", r0=self.n, rows=self.rows(target - self.n))

    def row_range(self):
        n = self.n
        rb = self.rint(0, n - 2)
        return rb, self.rint(rb + 1, n)

    # -- building blocks -----------------------------------------------------------------------------------
    def read(self, kind: str, c: float, role: str = "perturb"):
        n = self.n
        if kind == "row_argmin":
            row = self.rint(0, n - 1)
            self.do("row_argmin", role, row=row, partners=row if self.rint(0, 1) and row > 0 else n, c=c, thr=self.thr(c, 4000))
        elif kind == "topk_counted":
            self.do("topk", role, c=c, thr=self.thr(c, 3000), k=(50, 700)[self.rint(0, 1)], rb=0, re=-1, count=True)
        elif kind == "topk_uncounted":
            self.do("topk", role, c=c, thr=self.thr(c, 3000), k=(50, 700)[self.rint(0, 1)], rb=0, re=-1, count=False)
        elif kind == "topk_ranged":
            rb, re = self.row_range()
            self.do("topk", role, c=c, thr=self.thr(c, 6000), k=100, rb=rb, re=re, count=bool(self.rint(0, 1)))
        elif kind == "candidates":
            if self.mode == "lorentz" and self.rint(0, 1):
                self.do("candidates", role, c=c, thr=self.thr(c, 400), rb=0, re=-1)
            else:
                rb = self.rint(0, n - 2)
                self.do("candidates", role, c=c, thr=self.thr(c, 20000), rb=rb, re=min(n, rb + self.rint(1, 3)))
        elif kind == "count":
            self.do("count", role, c=c, thr=self.thr(c, 5000), n_limit=-1 if self.rint(0, 1) else self.rint(max(2, n - n // 4), n))
        elif kind in ("pair_distance", "midpoint"):
            b = self.rint(1, 40)
            I = self.rng.integers(0, n, b).astype(np.int32)
            J = self.rng.integers(0, n, b).astype(np.int32)
            if kind == "pair_distance":
                self.do("pair_distance", role, I=I, J=J, c=c)
            else:
                self.do("midpoint", role, I=I, J=J, W=self.rng.uniform(0.05, 0.95, b).astype(np.float32), c=c)
        elif kind == "argmin_into":
            self.do("argmin_into", role, c=c, thr=self.thr(c, 500), rb=0, re=-1)
        elif kind == "argmin":
            self.do("argmin", role, c=c, thr=self.thr(c, 500), rb=0, re=-1)
        elif kind == "argmin_other":
            if self.rint(0, 1):
                rb, re = self.row_range()
                self.do("argmin", role, c=c, thr=self.thr(c, 500), rb=rb, re=re)
            else:
                c2 = [v for v in CURVATURES if v != c][self.rint(0, 1)]
                self.do("argmin", role, c=c2, thr=self.thr(c2, 500), rb=0, re=-1)
        else:
            raise ValueError(kind)

    def searches(self):
        """every kind of search once"""
        c = self.curvature()
        for kind in ("argmin", "argmin_other", "row_argmin", "topk_counted", "topk_uncounted", "topk_ranged", "candidates", "count",
                     "argmin_into"):
            self.read(kind, c, role="check")

    def trio(self):
        """after a motif's last probe: argmin, one top-k and one count, which a fresh engine answers as well"""
        c = self.curvature()
        self.do("argmin", "trio", c=c, thr=self.thr(c, 500), rb=0, re=-1)
        self.do("topk", "trio", c=c, thr=self.thr(c, 3000), k=50, rb=0, re=-1, count=True)
        self.do("count", "trio", c=c, thr=self.thr(c, 5000), n_limit=-1)

    def append(self, kind: str, m: int, c: float, duplicate: bool = False):
        """``m`` new rows at n by one call of ``kind``; ``duplicate``: the (first) new row coincides with a live row"""
        n = self.n
        if kind == "update_rows":
            rows = self.rows(m)
            if duplicate:
                rows[0] = self.X[self.rint(0, n - 1)]
            self.do("update_rows", r0=n, rows=rows)
        elif kind == "merge_append":
            assert m == 1
            i, j = (int(v) for v in self.rng.choice(n, 2, replace=False))
            self.do("merge_append", i=i, j=j, w=0.0 if duplicate else float(np.float32(self.rng.uniform(0.1, 0.9))), c=c, new_row=n)
        else:
            independent = kind == "batch_independent"
            I, J = np.empty(m, np.int32), np.empty(m, np.int32)
            for t in range(m):
                I[t], J[t] = self.rng.choice(n if independent else n + t, 2, replace=False)
            if not independent and m > 1:
                J[m - 1] = n + m - 2         # the chain: the last merge reads the row written just before it
                if I[m - 1] == J[m - 1]:
                    I[m - 1] = 0
            W = self.rng.uniform(0.1, 0.9, m).astype(np.float32)
            if duplicate:
                W[0] = 0.0
            self.do("merge_batch", I=I, J=J, W=W, c=c, first_row=n, independent=independent)

    def append_some(self, total: int, c: float, pieces: int):
        """``total`` new rows in ``pieces`` appends of mixed kinds"""
        n_before = self.n
        cuts = sorted(self.rng.choice(np.arange(1, total), size=min(pieces - 1, total - 1), replace=False).tolist()) if total > 1 else []
        sizes = np.diff([0] + cuts + [total]).tolist()
        for m in sizes:
            kind = B_KINDS[self.rint(0, 3)]
            if kind == "merge_append" and m != 1:
                kind = "batch_chain"
            self.append(kind, int(m), c)
        return n_before

    # -- motifs --------------------------------------------------------------------------------------------
    def motif_A(self):
        c = self.curvature()
        thr = self.thr(c, 500)
        want = self.do("argmin", "setup", c=c, thr=thr, rb=0, re=-1)
        kinds = [self.deck("A", A_KINDS) for _ in range(5)]          # two A motifs deal all nine kinds
        for t, kind in enumerate(kinds):
            self.read(kind, c)
            self.cover["A"].add(kind)
            got = self.do("argmin", "probe" if t == len(kinds) - 1 else "check", c=c, thr=thr, rb=0, re=-1)
            assert got == want
        self.trio()

    def motif_B(self):
        for rnd in range(2):
            self.room(8)
            c = self.curvature()
            thr = self.thr(c, 500)
            self.do("argmin", "setup", c=c, thr=thr, rb=0, re=-1)
            kind = self.deck("B", B_KINDS)
            self.append(kind, 1 if kind == "merge_append" else self.rint(1, 6), c, duplicate=bool(self.rint(0, 1)))
            self.cover["B"].add(kind)
            self.do("argmin", "probe", c=c, thr=thr, rb=0, re=-1)
        self.trio()

    def motif_C(self):
        flipped = False
        for rnd in range(2):
            c = self.curvature()
            thr = self.thr(c, 500)
            hit = self.do("argmin", "setup", c=c, thr=thr, rb=0, re=-1)
            kind = self.deck("C", C_KINDS)
            n = self.n
            end = (hit[2], hit[3])[self.rint(0, 1)] if hit[0] else self.rint(0, n - 1)
            if kind == "overwrite_pair_end":
                self.do("update_rows", r0=end, rows=self.rows(1))
            elif kind == "merge_into_existing":
                i, j = (int(v) for v in self.rng.choice(n, 2, replace=False))
                self.do("merge_append", i=i, j=j, w=float(np.float32(self.rng.uniform(0.1, 0.9))), c=c, new_row=end)
            elif kind == "truncate":
                self.do("truncate", n_rows=min(n - 1, max(hit[2], hit[3], n - 20) if self.rint(0, 1) else n - self.rint(1, 20)))
            elif kind == "project_table":
                self.do("project_table", n_rows=n, c=(1.0, 0.7)[self.rint(0, 1)])
            elif kind == "set_table_other_count":
                m = min(self.max_rows - 40, max(self.n0 - 40, n + (self.rint(1, 30) if self.rint(0, 1) else -self.rint(1, 30))))
                self.do("set_table", rows=self.rows(m))
            else:
                self.do("set_prefilter")
                flipped = not flipped
            self.cover["C"].add(kind)
            self.do("argmin", "probe", c=c, thr=thr, rb=0, re=-1)
            if kind != "set_prefilter":      # ... and at a threshold that suits the table as it is now
                self.do("argmin", "probe", c=c, thr=self.thr(c, 500), rb=0, re=-1)
        self.trio()
        if flipped:
            self.do("set_prefilter", role="setup")

    def _list(self, c: float, k: int):
        """whole-table uncounted top-k that fills k -> threshold used"""
        thr = self.thr(c, 8 * k)
        for _ in range(6):
            got = self.do("topk", "setup", c=c, thr=thr, k=k, rb=0, re=-1, count=False)
            if got[0] == -1:
                return thr
            thr = float(np.float32(thr * 1.5))
        raise AssertionError("the list of a refresh motif does not fill k")

    def _note_cross(self, n_before: int):
        for tile, key in ((64, "cross64"), (256, "cross256")):
            if (self.n - 1) // tile > (n_before - 1) // tile:
                self.cover[key] += 1

    def motif_D(self, first: bool):
        c = self.curvature()
        k = (50, 700)[self.rint(0, 1)]
        if first:                            # the multiple of 256 above n0: what the shape exists for
            edge = (self.n0 // 256 + 1) * 256
        else:
            edge = 64 * self.rint((self.n0 - 40) // 64 + 1, (self.n0 + 280) // 64)
        start = edge - self.rint(1, 12)
        self.goto(start)
        thr = self._list(c, k)
        n_list = self.n
        self.do("count", c=c, thr=thr, n_limit=self.rint(max(2, n_list - 50), n_list))
        for rnd in range(2):
            total = (edge - start) + self.rint(1, 10) if rnd == 0 else self.rint(1, 25)
            before = self.append_some(total, c, self.rint(1, 3))
            self._note_cross(before)
            bigger = self.rint(0, 1)
            if bigger:
                thr = float(np.float32(thr * 1.25))
            self.do("refresh", "probe", c=c, thr=thr, k=k, grown=True)
            self.cover["d_probes_grown"] += 1
        self.trio()

    def motif_E(self):
        flipped = False
        for rnd in range(2):
            self.room(40)
            c = self.curvature()
            k = (50, 700)[self.rint(0, 1)]
            thr = self._list(c, k)
            if self.rint(0, 1):
                self.append_some(self.rint(1, 20), c, self.rint(1, 2))
            kind = self.deck("E", E_KINDS)
            n = self.n
            pc, pk, pthr = c, k, thr
            if kind == "overwrite":
                top = self.m.eng.topk(c, thr, 1)
                self.do("update_rows", r0=int(top[1][0]) if len(top[1]) else self.rint(0, n - 1), rows=self.rows(1))
            elif kind == "truncate":
                self.do("truncate", n_rows=n - self.rint(1, 10))
            elif kind == "project_table":
                self.do("project_table", n_rows=n, c=(1.0, 0.7)[self.rint(0, 1)])
            elif kind == "ranged_topk":
                self.do("topk", c=c, thr=thr, k=k, rb=self.rint(1, 9), re=n - self.rint(2, 9), count=False)
            elif kind == "set_prefilter":
                self.do("set_prefilter")
                flipped = not flipped
            elif kind == "other_c":
                pc = [v for v in CURVATURES if v != c][self.rint(0, 1)]
                pthr = float(np.float32(thr * np.sqrt(c / pc)))
            elif kind == "other_k":
                pk = 750 - k
            else:
                pthr = float(np.float32(thr * 0.9))
            self.cover["E"].add(kind)
            self.do("refresh", "probe", c=pc, thr=pthr, k=pk, grown=False)
        self.trio()
        if flipped:
            self.do("set_prefilter", role="setup")

    def motif_F(self):
        n = self.n
        row = self.rint(0, n - 1)
        self.do("update_rows", r0=row, rows=self.rows(1, scale=300.0))
        self.searches()
        self.do("update_rows", r0=row, rows=self.rows(1))
        self.searches()
        self.do("set_table", rows=self.rows(self.rint(self.n0 - 20, self.n0 + 20)))
        self.searches()
        c = self.curvature()
        self.do("argmin", "probe", c=c, thr=self.thr(c, 500), rb=0, re=-1)
        self.trio()

    def motif_G(self):
        self.room(90)
        for kind in (G_KINDS[t] for t in self.rng.permutation(3)):
            n = self.n
            if kind == "nan_row":
                self.do("update_rows", r0=self.rint(0, n - 1), rows=np.full((1, self.d1), np.nan, np.float32))
            elif kind == "tie_flood":
                block = np.repeat(self.X[self.rint(0, n - 1)][None, :], self.rint(3, 70), axis=0).copy()
                self.do("update_rows", r0=n if self.rint(0, 1) else self.rint(0, n - block.shape[0]), rows=block)
            else:                            # a write that starts beyond n: the rows between read as zero rows
                gap = self.rint(1, 5)
                if self.rint(0, 1):
                    self.do("update_rows", r0=n + gap, rows=self.rows(1))
                else:
                    i, j = (int(v) for v in self.rng.choice(n, 2, replace=False))
                    self.do("merge_append", i=i, j=j, w=0.5, c=1.0, new_row=n + gap)
            self.cover["G"].add(kind)
        self.searches()
        c = self.curvature()
        self.do("argmin", "probe", c=c, thr=self.thr(c, 500), rb=0, re=-1)
        self.trio()
        # leave an ordinary table behind: the refresh motifs need a k-th distance above 0
        self.do("set_table", role="setup", rows=self.rows(self.rint(self.n0 - 20, self.n0 + 20)))

    def _steps(self, op: str, c: float, thr: float, steps: int, role: str, **extra):
        got = self.do(op, role, c=c, thr=thr, steps=steps, lens=list(self.lens), **extra)
        for (_, i, j) in got[1]:
            self.lens.append(self.lens[i] + self.lens[j])
        self.cover["steps_merged"] += len(got[1])
        assert len(self.lens) == self.n
        return got

    def motif_H(self):
        self.room(24)
        c = self.curvature()
        thr = self.thr(c, 300)
        lens = [1 + (r * 7 + self.n) % 3 for r in range(self.n)]
        self.do("set_lens", "setup", lens=lens)
        self.lens = lens
        self._steps("std_steps", c, thr, self.rint(2, 6), "perturb")
        self.read("topk_uncounted", c, role="check")
        self.read("argmin_other", c, role="check")
        best = self.do("argmin", "check", c=c, thr=thr, rb=0, re=-1)
        if best[0]:
            d = float(np.array([best[1]], np.uint32).view(np.float32)[0])
            self._steps("incr_steps", c, thr, self.rint(1, 6), "perturb", best=(d, best[2], best[3]))
        self.read("count", c, role="check")
        self._steps("std_steps", c, thr, self.rint(2, 6), "probe")
        self.do("argmin", "probe", c=c, thr=thr, rb=0, re=-1)
        self.trio()

    def motif_K(self):
        self.room(8)
        c = self.curvature()
        thr = self.thr(c, 500)
        before = (self.n, self.do("argmin", "setup", c=c, thr=thr, rb=0, re=-1), self.do("topk", "setup", c=c, thr=thr, k=50, rb=0, re=-1, count=True))
        for rnd in range(3):
            kind = self.deck("K", K_KINDS)
            self.do("refused", kind=kind, thr=thr)
            self.cover["K"].add(kind)
            after = (self.n, self.do("argmin", "probe", c=c, thr=thr, rb=0, re=-1), self.do("topk", "check", c=c, thr=thr, k=50, rb=0, re=-1, count=True))
            assert same(before, after)
        self.trio()

    # -- the walk ------------------------------------------------------------------------------------------
    def build(self) -> Trace:
        self.motif = "init"
        self.do("set_table", role="setup", rows=self.rows(self.n0))
        order = [SCHEDULE[t] for t in self.rng.permutation(len(SCHEDULE))]
        seen_d = False
        for t, kind in enumerate(order):
            self.motif = "-"
            for _ in range(self.rint(0, 3)):
                filler = ("argmin", "row_argmin", "topk_counted", "topk_uncounted", "topk_ranged", "candidates", "count", "pair_distance",
                          "midpoint", "argmin_into")[self.rint(0, 9)]
                self.read(filler, self.curvature(), role="filler")
            self.motif = f"{kind}{t}"
            self.cover["motifs"][kind] += 1
            if kind == "D":
                self.motif_D(first=not seen_d)
                seen_d = True
            else:
                getattr(self, "motif_" + kind)()
        self.trace.cover = self.cover
        return self.trace


@functools.lru_cache(maxsize=None)
def build_trace(seed: int, n0: int, d: int, mode: str) -> Trace:
    """The walk of one seed with the model's answers.  Cached: the model's side is computed once per process and shared,
    unchanged, by every test that replays it."""
    return _Gen(seed, n0, d, mode).build()


def replay(seed: int, n0: int, d: int, mode: str, form: str = "f32", upto: Optional[int] = None,
           make_side: Callable[[int, int, str, str], Side] = oracle_side, fresh=None) -> Side:
    """Rerun the first ``upto`` calls of a walk on a new subject (``make_side(max_rows, d1, mode, form)``; the default is
    an oracle-backed one) -> the subject, for a look at its state."""
    trace = build_trace(seed, n0, d, mode)
    return run_trace(trace, make_side(trace.max_rows, d + 1, mode, form), fresh=fresh, upto=upto)


# the walks the GPU suite runs: (seed, n0, d) per shape, in both sign modes
SHAPES = ((11, 250, 10), (12, 1015, 37), (13, 2040, 100))
