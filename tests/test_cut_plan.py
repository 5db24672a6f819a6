"""The top-k search's emission-cut policy (CutSearch and hm_zoom_decide, hyptokenizer_amd/csrc/hm_cut_plan.h; DESIGN.md 5.4,
5.7) without a GPU: a stand-alone C++ program (tests/cut_plan_driver.cpp) runs the plan against scripted histograms and
pass outcomes, and the actions it takes are compared, line for line, with a Python transcription of the two functions the
plan was lifted from -- hm_topk_core_form and hm_estimate_cut as they stood in hm_search.hip before the lift, branch for
branch.  Both run against a synthetic table model (below)."""
import collections
import os
import shutil
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

ONE, ALL, NO_TIE, INF_BITS = 0x3F800000, 0xFFFFFFFF, 0x7FFFFFFF, 0x7F800000
E_CAPACITY, E_STATE = -2, -3
M32 = 0xFFFFFFFF
MSG_UNBOUNDED = "top-k: could not bound the emission"
MSG_LISTING = "candidate listing: more candidates than the emission buffer holds"
MSG_CONVERGE = "top-k: emission cut did not converge"
MSG_MARGIN = ("pair scan: prefilter margin violated (an entry classified as surely below the "
              "threshold is not); table holds non-finite rows other than all-NaN rows?")


def tie_slack(ubits):
    if ubits >= 0x40000000:
        return 1024
    return 32 + ((ubits - ONE if ubits > ONE else 0) >> 16)


def fbits(x):
    return np.asarray(x, np.float32).view(np.uint32).astype(np.int64)


# ------------------------------------------------------------------------------------------------
# the table model
# ------------------------------------------------------------------------------------------------
class Model:
    """Groups of pairs: bit pattern of u' (prefilter and canonical value alike), row i, multiplicity.  A pair is a
    candidate when bits < thr_bits; the prefilter is sure of it when bits + shell < thr_bits, and every pair it is not sure
    of is emitted whatever the cut says.  No group lies above thr_bits + shell (the scan never sees those).  The table has
    n rows and the search covers rows [row_begin, row_end): `pairs` pairs, nearly all of them far above the threshold."""

    def __init__(self, bits, rows, mult, thr_bits, shell, n, ent_cap, margin=0):
        self.bits, self.rows, self.mult = (np.asarray(v, np.int64) for v in (bits, rows, mult))
        assert self.bits.max() <= thr_bits + shell and self.bits.min() >= ONE and self.rows.max() < n - 1
        self.thr_bits, self.shell, self.n, self.ent_cap, self.margin = thr_bits, shell, n, ent_cap, margin
        self.row_begin, self.row_end = 0, n - 1
        self.pairs = n * (n - 1) // 2
        self.hi_bits = thr_bits + shell + 1

    def hist(self, lo, shift, stride):
        """What a sampled histogram pass reads back: 256 bins of width 1 << shift from lo on, every stride-th pair."""
        q = (self.bits - lo) >> shift
        sel = (self.bits >= lo) & (q < 256)
        h = np.zeros(256, np.int64)
        np.add.at(h, q[sel], self.mult[sel])
        return [int(v) for v in h // stride]

    def scan(self, cut, tie, count_sure):
        """What one pass with (cut_bits, tie_imax) reports: (emitted, valid, borderline, sure, complete, margin)."""
        b, r, m = self.bits, self.rows, self.mult
        valid, sure, zero = b < self.thr_bits, b + self.shell < self.thr_bits, b <= ONE
        emit = (b <= cut) | ~sure
        if tie != NO_TIE:
            emit = np.where(zero, r <= tie, emit)
            complete = zero & (r <= tie)
        else:
            complete = zero | (b + tie_slack(cut) <= cut if cut != ALL else np.ones_like(zero))
        tot = lambda mask: int(m[mask].sum())
        return (tot(emit), tot(emit & valid), tot(emit & valid & ~sure), tot(sure) if count_sure else 0,
                tot(emit & valid & complete), self.margin)


# ------------------------------------------------------------------------------------------------
# the transcription: hm_estimate_cut and hm_topk_core_form of the parent commit (4e7ab11), branch for branch
# ------------------------------------------------------------------------------------------------
class Walk:
    """One search: the log of actions (what the driver must print), the script (what the driver is fed) and the labels
    of the branches taken."""

    def __init__(self, labels):
        self.log, self.script, self.labels = [], [], labels

    def hit(self, label):
        self.labels[label] += 1


def estimate_cut(w, env, target):
    """hm_estimate_cut.  env: pairs, ent_cap, hi_bits, n, row_begin, row_end, hist(lo, shift, stride)."""
    cut_bits, tie_imax = ALL, NO_TIE
    pairs = env.pairs
    if pairs <= env.ent_cap // 2:
        w.hit("est.fits")
        w.log.append("fits")
        return cut_bits, tie_imax
    lo_bits, hi_bits = ONE, env.hi_bits
    stride = 1
    while stride < 64 and pairs // (stride * 2) > 40000000:
        w.hit("est.stride_sample")
        stride *= 2
    while pairs // stride > (1 << 30):
        w.hit("est.stride_2^30")
        stride *= 2
    base = 0.0
    for _zoom in range(6):
        span = hi_bits - lo_bits
        shift = 0
        while (span >> shift) > 256:
            shift += 1
        w.log.append("hist %d %d %d" % (lo_bits, shift, stride))
        h = env.hist(lo_bits, shift, stride)
        w.script.append("h %d %s" % (sum(1 for v in h if v), " ".join("%d %d" % (q, v) for q, v in enumerate(h) if v)))
        cum = base
        bsel = -1
        for q in range(256):
            cum += float(h[q]) * stride
            if cum >= float(target):
                bsel = q
                break
        if bsel < 0:
            w.hit("est.emit_all")
            return cut_bits, tie_imax
        before = cum - float(h[bsel]) * stride
        edge_lo = (lo_bits + (bsel << shift)) & M32
        edge_hi = (lo_bits + ((bsel + 1) << shift)) & M32
        if cum <= float(env.ent_cap) * 0.5 or shift == 0:
            cut_bits = (edge_hi - 1) & M32
            if cum > float(env.ent_cap) * 0.5:
                w.hit("est.tie_flood")
                per_row = (float(h[bsel]) * stride) / float(env.row_end - env.row_begin)
                rows = (float(target) - before) / (per_row if per_row > 1e-9 else 1e-9)
                pad = 64
                while pad > 1 and pad * env.n > env.ent_cap // 2:
                    w.hit("est.pad_shrink")
                    pad >>= 1
                imax = env.row_begin + int(rows * 2.0) + pad
                if imax > env.row_end:
                    w.hit("est.imax_clamp")
                    imax = env.row_end
                tie_imax = imax
            else:
                w.hit("est.cut")
            return cut_bits, tie_imax
        w.hit("est.zoom")
        lo_bits, hi_bits, base = edge_lo, edge_hi, before
    w.hit("est.zooms_exhausted")
    return cut_bits, tie_imax


def core_form(w, env, k, list_all, count_sure, remembered=None, estimate=estimate_cut):
    """hm_topk_core_form from behind hm_prepare_scan on.  remembered: the remembered cut's bits with the slack added, when
    one applies.  Returns (status, total, valid)."""
    def fail(status, msg):
        w.log.append("fail %d %s" % (status, msg))
        return status, 0, 0

    def est(target):
        w.log.append("estimate %d" % target)
        c, t = estimate(w, env, target)
        w.log.append("cut %d %d" % (c, t))
        return c, t

    cut_bits, tie_imax = ALL, NO_TIE
    if not list_all and k == 0:
        w.hit("core.start_count")
        cut_bits, tie_imax = ONE, -1
    elif not list_all:
        if remembered is not None:
            w.hit("core.start_remembered")
            cut_bits = remembered
        else:
            w.hit("core.start_estimate")
            cut_bits, tie_imax = est(4 * k + 4096)
    else:
        w.hit("core.start_list_all")
    tight_bits, loose_bits = 0, ALL
    stuck = 0
    for attempt in range(40):
        w.log.append("scan %d %d" % (cut_bits, tie_imax))
        emitted, valid, borderline, sure, complete, margin = env.scan(cut_bits, tie_imax, count_sure)
        w.script.append("p %d %d %d %d %d %d" % (emitted, valid, borderline, sure, complete, margin))
        if margin != 0:
            w.hit("core.margin")
            return fail(E_STATE, MSG_MARGIN)
        overflow = emitted > env.ent_cap
        emitted_all = cut_bits == ALL and tie_imax == NO_TIE
        if overflow:
            if list_all:
                w.hit("core.overflow_list_all")
                return fail(E_CAPACITY, MSG_LISTING)
            if tie_imax == NO_TIE and tight_bits != 0:
                if cut_bits < loose_bits:
                    w.hit("core.bisect_lowers_loose")
                    loose_bits = cut_bits
                if loose_bits <= tight_bits + 1:
                    w.hit("core.unsplittable_on_overflow")
                    return fail(E_CAPACITY, MSG_UNBOUNDED)
                w.hit("core.bisect_on_overflow")
                cut_bits = tight_bits + (loose_bits - tight_bits) // 2
                continue
            if tie_imax == NO_TIE and cut_bits < loose_bits:
                w.hit("core.overflow_lowers_loose")
                loose_bits = cut_bits
            w.hit("core.reestimate")
            target = max((2 * k + 1024) >> min(attempt, 20), k + 64)
            cut_bits, tie_imax = est(target)
            if cut_bits == ALL:
                w.hit("core.reestimate_emit_all")
                return fail(E_CAPACITY, MSG_UNBOUNDED)
            if tie_imax == NO_TIE and target == k + 64 and cut_bits >= loose_bits:
                w.hit("core.stuck_counted")
                stuck += 1
                if stuck >= 2:
                    w.hit("core.stuck")
                    return fail(E_CAPACITY, MSG_UNBOUNDED)
            continue
        total = valid if emitted_all else (sure + borderline if count_sure else -1)
        want = min(k, total) if total >= 0 else k
        if not emitted_all and complete < want:
            if tie_imax != NO_TIE:
                w.hit("core.widen_rows")
                tie_imax = NO_TIE if tie_imax >= env.row_end else min(tie_imax * 4 + 256, env.row_end)
                if tie_imax >= env.row_end:
                    w.hit("core.widen_rows_to_all")
                    tie_imax = NO_TIE
            else:
                if cut_bits > tight_bits:
                    w.hit("core.raises_tight")
                    tight_bits = cut_bits
                span = cut_bits - ONE
                nb = cut_bits + max(span, 4 * tie_slack(cut_bits))
                if loose_bits != ALL and nb >= loose_bits:
                    if loose_bits <= tight_bits + 1:
                        w.hit("core.unsplittable_on_widening")
                        return fail(E_CAPACITY, MSG_UNBOUNDED)
                    w.hit("core.bisect_on_widening")
                    cut_bits = tight_bits + (loose_bits - tight_bits) // 2
                elif nb >= INF_BITS:
                    w.hit("core.widen_to_all")
                    cut_bits = ALL
                else:
                    w.hit("core.widen_geometric")
                    cut_bits = nb
            continue
        w.hit("core.done")
        w.log.append("done %d %d" % (total, valid))
        return 0, total, valid
    w.hit("core.not_converged")
    return fail(E_CAPACITY, MSG_CONVERGE)


ALL_LABELS = {
    "est.fits", "est.stride_sample", "est.stride_2^30", "est.emit_all", "est.tie_flood", "est.pad_shrink", "est.imax_clamp",
    "est.cut", "est.zoom",
    "core.start_count", "core.start_remembered", "core.start_estimate", "core.start_list_all", "core.margin",
    "core.overflow_list_all", "core.bisect_lowers_loose", "core.unsplittable_on_overflow", "core.bisect_on_overflow",
    "core.overflow_lowers_loose", "core.reestimate", "core.reestimate_emit_all", "core.stuck_counted", "core.stuck",
    "core.widen_rows", "core.widen_rows_to_all", "core.raises_tight", "core.unsplittable_on_widening",
    "core.bisect_on_widening", "core.widen_to_all", "core.widen_geometric", "core.done", "core.not_converged",
}
# The one label no table can reach: "est.zooms_exhausted", the fall out of the six-zoom loop.  The first window is
# [bits(1.0), hi_bits) with hi_bits <= bits(+inf): at most 2^30 patterns, so its shift is at most 22 (2^30 >> 22 = 256 bins).
# A zoom narrows the window to ONE bin, 1 << shift patterns, whose own shift is max(shift - 8, 0): 22, 14, 6, 0.  The fourth
# window at the latest has shift 0, and a window of shift 0 always ends in "cut" / "tie flood" or "emit all".
UNREACHABLE = {"est.zooms_exhausted"}


# ------------------------------------------------------------------------------------------------
# the cases
# ------------------------------------------------------------------------------------------------
def spread(count, lo_x, hi_x, rows=50, power=1.0, seed=0):
    """count pairs with u' - 1 = x, P(x' < x) ~ (x / hi_x)^power on [lo_x, hi_x), rows cycling."""
    u = np.random.RandomState(seed).rand(count)
    x = np.maximum(hi_x * u ** (1.0 / power), lo_x)
    return np.sort(fbits(1.0 + x)), np.arange(count) % rows, np.ones(count, np.int64)


def flood(rows_with, per_row, tail=300, tail_x=(0.01, 0.3)):
    """per_row zero-distance pairs (u' = 1) in each row of rows_with, and a thin spread of other candidates."""
    tb, tr, tm = spread(tail, tail_x[0], tail_x[1])
    rows_with = np.asarray(rows_with, np.int64)
    return (np.concatenate([np.full(len(rows_with), ONE, np.int64), tb]), np.concatenate([rows_with, tr]),
            np.concatenate([np.full(len(rows_with), per_row, np.int64), tm]))


def case_list():
    cases = []

    def add(name, model, k, list_all=False, count_sure=True, remembered=None):
        cases.append(dict(name=name, model=model, k=k, list_all=list_all, count_sure=count_sure, remembered=remembered))

    thr = int(fbits(1.3))
    b, r, m = spread(2000, 1e-4, 0.299, rows=60)
    # 64 rows: 2016 pairs <= ent_cap / 2 -- the estimate answers "emit all" without a histogram
    add("everything fits", Model(b, r, m, thr, 64, 64, 8192), 10)
    uniform = Model(*spread(3000, 1e-4, 0.299), thr, 64, 3000, 2048)
    add("estimated cut accepted", Model(*spread(30000, 1e-4, 0.299), thr, 64, 3000, 16384), 10, count_sure=False)
    add("remembered cut accepted", uniform, 10, remembered=int(fbits(1.05)))
    add("remembered cut widened geometrically", uniform, 200, count_sure=False, remembered=int(fbits(1.002)))
    # d = 50: P(u - 1 < x) ~ x^25.  A cut at half the range holds nothing, twice that everything: bracketed, bisected
    dense = Model(*spread(3000, 1e-4, 0.299, power=25.0), thr, 64, 3000, 1024)
    add("dense: bracketed and bisected", dense, 10, remembered=int(fbits(1.15)))
    add("dense: estimated", dense, 10)
    # a spike of more than ent_cap pairs at one pattern S, next to nothing below it: every cut < S is tight, every cut >= S
    # overflows.  Which of the two sides closes the bracket depends on S
    for s_bits in range(int(fbits(1.2)), int(fbits(1.2)) + 4):
        sb = np.array([int(fbits(1.0001)), s_bits])
        add("bracket cannot be split (S = %d)" % s_bits, Model(sb, [0, 1], [3, 5000], thr, 64, 3000, 1024), 10,
            remembered=int(fbits(1.01)))
    # the same spike far out, approached from bits(1.0) + 1: ~27 widenings, then a bracket of 2^29 patterns to bisect
    far = np.array([int(fbits(1.0001)), 0x7F000000])
    add("never satisfied: 40 attempts", Model(far, [0, 1], [3, 5000], 0x7F000100, 64, 3000, 1024), 10, remembered=ONE + 1)
    add("widened to emit all", Model(far, [0, 1], [3, 500], 0x7F000100, 64, 3000, 1024), 10, remembered=0x60000000)
    # ent_cap / 2 pairs at the smallest pattern and a shell of undecided pairs that alone overflows the buffer: every
    # estimate returns that pattern, every scan overflows
    sb = np.concatenate([[int(fbits(1.01))], np.arange(thr - 60, thr + 60)])
    add("stuck at the smallest target", Model(sb, np.arange(len(sb)) % 50, [8192] + [200] * 120, thr, 64, 3000, 16384), 1000)
    # more pairs than the buffer, fewer than any target
    add("estimate after an overflow says emit all", Model(*spread(150, 1e-4, 0.299), thr, 64, 3000, 120), 100,
        remembered=int(fbits(1.29)))
    # tie floods: 20 pairs at distance 0 per row
    add("tie flood: row limit accepted", Model(*flood(np.arange(20000), 20), thr, 64, 20001, 65536), 100)
    add("tie flood: row limit widened once", Model(*flood(np.arange(600, 20000), 20), thr, 64, 20001, 65536), 100)
    add("tie flood: widened to all rows", Model(*flood(np.arange(500, 1000), 40), thr, 64, 1001, 4096), 100)
    add("tie flood: row limit clamped", Model(*flood(np.arange(90), 40), thr, 64, 100, 4096), 2500)
    add("pure count", uniform, 0)
    add("pure count of a tie flood", Model(*flood(np.arange(500, 1000), 40), thr, 64, 1001, 4096), 0)
    add("list_all fits", Model(*spread(1500, 1e-4, 0.299), thr, 64, 3000, 2048), 0, list_all=True)
    add("list_all overflows", uniform, 0, list_all=True)
    add("margin violation", Model(*spread(3000, 1e-4, 0.299), thr, 64, 3000, 2048, margin=1), 10)
    # 2^20 rows: ~2^39 pairs, the stride grows past 64 until pairs / stride <= 2^30
    b, r, m = spread(4000, 1e-4, 0.299, rows=1000)
    add("more than 2^30 * 64 pairs", Model(b, r, m * 100000, thr, 64, 1 << 20, 1 << 24), 1000)
    return cases


def walk_case(case, labels):
    w = Walk(labels)
    env = case["model"]
    result = core_form(w, env, case["k"], case["list_all"], case["count_sure"], case["remembered"])
    head = "case %d %d %d %d %d %d %d %d %d %d %d" % (
        case["k"], case["list_all"], case["count_sure"], env.ent_cap, env.n, env.row_begin, env.row_end,
        case["remembered"] is not None, case["remembered"] or 0, env.pairs, env.hi_bits)
    return [head] + w.script, ["case"] + w.log, result


@pytest.fixture(scope="module")
def walked():
    labels = collections.Counter()
    return [walk_case(case, labels) for case in case_list()], labels


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("cut_plan") / "cut_plan_driver")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", os.path.join(HERE, "cut_plan_driver.cpp"), "-o", exe]
    if subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True).returncode != 0:
        subprocess.run(base, check=True, capture_output=True)        # a compiler without the sanitizer runtimes
    return exe


def test_cut_plan_takes_the_actions_of_the_functions_it_was_lifted_from(driver, walked):
    script = [line for s, _, _ in walked[0] for line in s]
    want = [line for _, log, _ in walked[0] for line in log]
    out = subprocess.run([driver], input="\n".join(script) + "\n", capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, (out.stdout[-400:], out.stderr[-2000:])
    got = out.stdout.split("\n")[:-1]
    for n, (g, x) in enumerate(zip(got, want)):
        assert g == x, (n, got[max(0, n - 5):n + 1], want[max(0, n - 5):n + 1])
    assert len(got) == len(want)


def test_the_cases_take_every_branch_of_the_transcription(walked):
    results = {case["name"]: res for case, (_, _, res) in zip(case_list(), walked[0])}
    labels = walked[1]
    assert set(labels) <= ALL_LABELS and not (set(labels) & UNREACHABLE)
    assert sorted(ALL_LABELS - set(labels)) == []
    # and the cases end as their names say
    assert results["everything fits"][0] == 0 and results["estimated cut accepted"][:2] == (0, -1)
    assert results["dense: bracketed and bisected"][0] == 0 and results["tie flood: row limit widened once"][0] == 0
    assert results["list_all fits"] == (0, 1500, 1500) and results["pure count"][:2] == (0, 3000)
    for name in ("never satisfied: 40 attempts", "stuck at the smallest target", "list_all overflows",
                 "estimate after an overflow says emit all"):
        assert results[name][0] == E_CAPACITY, name
    assert results["margin violation"][0] == E_STATE


class Scripted:
    """An environment that answers from a list: scan outcomes in order, the estimates' answers in order."""
    pairs, ent_cap, n, row_begin, row_end, hi_bits = 10 ** 9, 1000, 50000, 0, 49999, int(fbits(2.0))

    def __init__(self, scans, cuts=()):
        self.scans, self.cuts, self.targets, self.asked = list(scans), list(cuts), [], []

    def scan(self, cut, tie, count_sure):
        self.asked.append((cut, tie))
        return self.scans.pop(0) if len(self.scans) > 1 else self.scans[0]

    def estimate(self, w, env, target):
        self.targets.append(target)
        return self.cuts.pop(0) if len(self.cuts) > 1 else self.cuts[0]


def run_scripted(env, k, **kw):
    w = Walk(collections.Counter())
    return core_form(w, env, k, kw.pop("list_all", False), kw.pop("count_sure", True), estimate=env.estimate, **kw), w


def test_the_transcription_itself():
    """What the issue of the refactor fixed in words, checked on the transcription the program is compared with."""
    fits = lambda complete: (500, 400, 10, 390, complete, 0)
    over = (1001, 0, 0, 0, 0, 0)
    # a pure count starts at bits(1.0) with no zero-distance ties and asks for no estimate; list-all starts at emit all
    env = Scripted([fits(0)])
    assert run_scripted(env, 0)[0] == (0, 400, 400) and env.asked == [(ONE, -1)] and env.targets == []
    env = Scripted([fits(0)])
    assert run_scripted(env, 0, list_all=True)[0] == (0, 400, 400) and env.asked == [(ALL, NO_TIE)] and env.targets == []
    # a margin violation is HM_E_STATE before anything else is looked at -- an overflow included
    res, w = run_scripted(Scripted([(5000, 0, 0, 0, 0, 1)]), 10, remembered=ONE + 5)
    assert res[0] == E_STATE and w.log[-1] == "fail %d %s" % (E_STATE, MSG_MARGIN)
    # the re-estimate target: (2k + 1024) >> min(attempt, 20), floor k + 64; the attempt advances on every retry
    env = Scripted([over], cuts=[(ONE + 100 - q, NO_TIE) for q in range(60)])
    res, w = run_scripted(env, 1000)
    assert res[0] == E_CAPACITY and w.log[-1].endswith(MSG_CONVERGE) and len(env.asked) == 40
    assert env.targets == [4 * 1000 + 4096] + [max(3024 >> a, 1064) for a in range(40)]
    # ... and an "emit all" answer after an overflow ends the search
    env = Scripted([over], cuts=[(ONE + 100, NO_TIE), (ALL, NO_TIE)])
    res, w = run_scripted(env, 1000)
    assert res[0] == E_CAPACITY and w.log[-1].endswith(MSG_UNBOUNDED) and len(env.asked) == 1
    # stuck: the smallest target (attempt >= 2 at k = 1000) returning a cut at or above the loose side, twice
    env = Scripted([over], cuts=[(ONE + 100, NO_TIE)])
    res, w = run_scripted(env, 1000)
    assert res[0] == E_CAPACITY and env.targets == [8096, 3024, 1512, 1064, 1064] and len(env.asked) == 4
    # ... which a tie flood never is: loose_bits is lowered, and the stuck counter runs, only without a row limit
    env = Scripted([over], cuts=[(ONE, 700)])
    res, w = run_scripted(env, 1000)
    assert w.log[-1].endswith(MSG_CONVERGE) and len(env.asked) == 40 and w.labels["core.overflow_lowers_loose"] == 0
    # the bisection on overflow needs a tight side: without one every overflow goes back to the estimate
    assert w.labels["core.bisect_on_overflow"] == 0 and w.labels["core.reestimate"] == 40
    # widening: max(span, 4 * slack) in the ulp domain; with a loose side in reach, the midpoint instead
    env = Scripted([fits(0), fits(0), over, fits(10)])
    res, w = run_scripted(env, 10, remembered=ONE + 1)
    c1 = ONE + 1 + 4 * tie_slack(ONE + 1)
    c2 = c1 + max(c1 - ONE, 4 * tie_slack(c1))
    assert res == (0, 400, 400) and env.asked == [(ONE + 1, NO_TIE), (c1, NO_TIE), (c2, NO_TIE), (c1 + (c2 - c1) // 2, NO_TIE)]
    # a bracket that cannot be split
    env = Scripted([fits(0), over], cuts=[(ONE + 1, NO_TIE)])
    env.scan = lambda cut, tie, cs, env=env: (env.asked.append((cut, tie)), over if cut > ONE + 200 else fits(0))[1]
    res, w = run_scripted(env, 10, remembered=ONE + 1)
    assert res[0] == E_CAPACITY and w.log[-1].endswith(MSG_UNBOUNDED) and env.asked[-1][0] in (ONE + 200, ONE + 201)
    # a tie flood is widened by rows: * 4 + 256, "all rows" once that reaches the end of the range
    env = Scripted([fits(0), fits(0), fits(0), fits(0), fits(0), fits(10)], cuts=[(ONE, 100)])
    res, w = run_scripted(env, 10)
    assert [t for _, t in env.asked] == [100, 656, 2880, 11776, 47360, NO_TIE] and res == (0, 400, 400)
    # the uncounted form: total -1, want = k
    env = Scripted([fits(9), fits(10)])
    res, w = run_scripted(env, 10, count_sure=False, remembered=ONE + 1)
    assert res == (0, -1, 400) and len(env.asked) == 2
