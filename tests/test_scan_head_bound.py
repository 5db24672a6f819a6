"""CPU: the inequality behind the argmin scan's head test (hm_scan.hip, HEAD > 0), in numpy.

The kernel drops a column group after its head k-steps when every head value is at or above the bound that the complete
prefilter value is compared with.  That is exact as long as, for EVERY pair,

    head_f  <=  u_c + delta

where head_f is the head form  x0 y0 - sum_{k in H} x_k y_k - r^ r^'  evaluated on the bf16 image in fp32 (whatever order
the matrix cores accumulate in), u_c the canonical fp32 value of the pair (products rounded one by one, summed in torch's
reduction order, fl(fl(x0 y0) - S): hm_img_u in hm_common.h) and delta the margin of hm_scan_delta (hm_common.h).  In
the accumulators' sign (they hold -head) the same statement reads: the head value stays at or above -(u_c + delta).

bf16 is emulated by rounding float32 bit patterns to nearest even; the image layout, the head set and the rest norm r^
restate these functions of hm_common.h: hm_bf16_ksteps, hm_head_steps, hm_rest_begin, hm_rest_end (the head set);
hm_rest_norm_round, hm_rest_sq, hm_rest_norm_bf16 and its wave form hm_wave_rest_norm_bf16, which adds the same four
interleaved sums in the same order (the rest norm); hm_bf16_chunk (the row layout); the stationary side's r^' = max(r^, smallest normal) restates load_a of hm_scan.hip."""
from fractions import Fraction

import numpy as np
import pytest
import torch

HEAD = 3                                        # HM_SCAN_HEAD
KCS = (2, 4, 8, 13, 14, 16)                     # kSupportedKC, hm_engine.hip


def bf16_bits(x):
    """float32 -> bf16 bit pattern, round to nearest even (NaN stays NaN)"""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint32)
    nan = np.isnan(x)
    return np.where(nan, np.uint32(0x7FC0), r).astype(np.uint32)


def bf16_val(bits):
    return (np.asarray(bits, dtype=np.uint32) << 16).view(np.float32)


def bf16(x):
    return bf16_val(bf16_bits(x))


def layout(d):
    kc = next(v for v in KCS if v >= (d + 4 + 7) // 8)
    ksteps = (kc + 1) // 2
    head = HEAD if ksteps >= HEAD + 1 else 0
    rest = (16 * (head - 1), 16 * (ksteps - 1)) if head else (0, 0)
    return kc, ksteps, head, rest


def rest_norm_bits(S, d, kc):
    """hm_rest_norm_bf16 with hm_rest_norm_round (hm_common.h) for every row of the spatial part S [n, d], in float64 as on the device"""
    _, ksteps, head, (s0, s1) = layout(d)
    s1 = min(s1, d)
    ss = np.zeros((S.shape[0], 4), np.float64)
    with np.errstate(all="ignore"):
        for s in range(s0, s1):
            v = bf16(S[:, s]).astype(np.float64)
            ss[:, s & 3] = ss[:, s & 3] + v * v
        t = (ss[:, 0] + ss[:, 1]) + (ss[:, 2] + ss[:, 3])
        rn = np.sqrt(t) * (1.0 + 2.0 ** -40)
        f = rn.astype(np.float32)
        b = (f.view(np.uint32) >> 16).astype(np.uint32)
        b = np.where(bf16_val(b).astype(np.float64) < rn, b + 1, b).astype(np.uint32)
    b = np.minimum(b, 0x7F7F)
    b = np.maximum(b, 0x0080)
    b = np.where(rn > 0.0, b, 0)
    return np.where(np.isnan(rn), 0x7FC0, b).astype(np.uint32)


def orders(terms, rs):
    """fp32 accumulations of the term list [T, n, n] (terms in k-step order, the time step first) in several orders"""
    T = terms.shape[0]
    out = []
    with np.errstate(all="ignore"):
        for perm in (np.arange(T), np.arange(T)[::-1], rs.permutation(T), rs.permutation(T)):
            acc = np.zeros(terms.shape[1:], np.float32)
            for t in perm:
                acc = (acc + terms[t]).astype(np.float32)
            out.append(acc)
        # k-step by k-step, every step's 16 (8) products summed exactly and rounded once (a wide internal accumulator)
        acc = np.zeros(terms.shape[1:], np.float32)
        for s in range(0, T, 16):
            acc = (acc.astype(np.float64) + terms[s:s + 16].astype(np.float64).sum(axis=0)).astype(np.float32)
        out.append(acc)
        # pairwise tree inside a k-step, sequential across k-steps
        acc = np.zeros(terms.shape[1:], np.float32)
        for s in range(0, T, 16):
            blk = [terms[t] for t in range(s, min(s + 16, T))]
            while len(blk) > 1:
                blk = [(blk[i] + blk[i + 1]).astype(np.float32) if i + 1 < len(blk) else blk[i] for i in range(0, len(blk), 2)]
            acc = (acc + blk[0]).astype(np.float32)
        out.append(acc)
    return out


def check_table(X, d, seed=0):
    """every pair of the table X [n, d + 1]: head_f <= u_c + delta in every accumulation order; returns the largest
    head_f - u_c seen among the pairs with a finite canonical value, in units of delta"""
    X = np.ascontiguousarray(X, dtype=np.float32)
    n = X.shape[0]
    kc, ksteps, head, (s0, s1) = layout(d)
    assert head == HEAD, "a width without a head has nothing to check"
    x0, S = X[:, 0], X[:, 1:]
    Sb = np.zeros((n, 8 * kc - 4), np.float32)
    Sb[:, :d] = bf16(S)
    with np.errstate(all="ignore"):
        hi = bf16(x0)
        lo = bf16((x0 - hi).astype(np.float32))
        rb = rest_norm_bits(S, d, kc)
        rhat = bf16_val(rb)
        rstat = bf16_val(np.maximum(rb, 0x0080))               # stationary side: max(r^, smallest normal)
        # canonical u: torch's reduction order over the separately rounded products
        St = torch.from_numpy(S)
        Ssum = (St[:, None, :] * St[None, :, :]).sum(dim=-1).numpy()
        u_c = ((x0[:, None] * x0[None, :]).astype(np.float32) - Ssum).astype(np.float32)
        # delta (hm_scan_delta, bf16 form, kterms = 8 * KC) from the norm bounds of the finite rows (hm_rownorm_kernel);
        # taken a hair SMALLER than the device's fmaf chains can make them
        s2 = (S.astype(np.float64) ** 2).sum(axis=1)
        r2 = s2 + x0.astype(np.float64) ** 2
        ok = r2 < 3.0e38
        rmax2 = np.float32(r2[ok].max() * (1 - 1e-5))
        smax2 = np.float32(s2[ok].max() * (1 - 1e-5))
        delta = np.float32(np.float32((8 * kc + 8) * np.float32(1.1920929e-07)) * rmax2 * np.float32(1.0001)) \
            + np.float32(0.00782) * smax2 + np.float32(4.7e-5) * rmax2
        # the head's terms as the accumulators see them (acc = -head): the time k-step (its spatial slots, then the
        # rewritten time slots [-hi, -hi, -lo, +r^'] x [hi, lo, hi, r^]), then k-steps 0 .. HEAD - 2
        tslots = list(range(16 * (ksteps - 1), 8 * kc - 4))
        terms = [Sb[:, None, k] * Sb[None, :, k] for k in tslots]
        terms += [-hi[:, None] * hi[None, :], -hi[:, None] * lo[None, :], -lo[:, None] * hi[None, :], rstat[:, None] * rhat[None, :]]
        terms += [np.zeros((n, n), np.float32)] * (16 - len(terms) % 16 if len(terms) % 16 else 0)
        terms += [Sb[:, None, k] * Sb[None, :, k] for k in range(0, 16 * (HEAD - 1))]
        terms = np.stack([np.asarray(t, dtype=np.float32) for t in terms])
    assert set(tslots) | set(range(0, s0)) | set(range(s0, s1)) == set(range(8 * kc - 4)), "head and rest cover every spatial slot"
    rs = np.random.RandomState(seed)
    fin = np.isfinite(u_c) & ok[:, None] & ok[None, :]
    assert fin.any()
    worst = -np.inf
    for acc in orders(terms, rs):
        head_f = -acc
        with np.errstate(all="ignore"):
            bad = fin & ~(head_f <= u_c + delta)               # (a NaN head value of a pair with a finite u_c is a failure too)
        assert not bad.any(), (d, int(bad.sum()), np.argwhere(bad)[:3].tolist())
        with np.errstate(all="ignore"):
            worst = max(worst, float(np.nanmax(np.where(fin, (head_f.astype(np.float64) - u_c) / np.float64(delta), -np.inf))))
    return worst, rb


def lorentz_rows(rs, n, d, scale):
    S = (rs.randn(n, d) * scale).astype(np.float32)
    X = np.zeros((n, d + 1), np.float32)
    X[:, 1:] = S
    with np.errstate(all="ignore"):
        X[:, 0] = np.sqrt(np.float32(1.0) + (S * S).sum(axis=1, dtype=np.float32)).astype(np.float32)
    return X


def reproject(X):
    with np.errstate(all="ignore"):
        X[:, 0] = np.sqrt(np.float32(1.0) + (X[:, 1:] ** 2).sum(axis=1, dtype=np.float32)).astype(np.float32)
    return X


WIDTHS = [36, 100, 108, 124]      # 8 chunks (even), 13 (odd: half step), 14 (even), 16 (even); d = 24 has 4 chunks: no head


def test_widths_without_a_head():
    assert layout(24)[2] == 0 and layout(20)[2] == 0 and layout(12)[2] == 0
    S = np.random.RandomState(0).randn(5, 24).astype(np.float32)
    assert (rest_norm_bits(S, 24, layout(24)[0]) == 0).all()
    assert [layout(d)[0] for d in WIDTHS] == [8, 13, 14, 16] and layout(100)[3] == (32, 96) and layout(124)[3] == (32, 112)


@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("scale", [0.05, 0.5, 1e-3])
def test_random_tables(d, scale):
    rs = np.random.RandomState(d)
    X = lorentz_rows(rs, 96, d, scale)
    X[50] = X[3]                                    # an exact duplicate: u_c at 1
    worst, _ = check_table(X, d)
    assert worst <= 1.0


@pytest.mark.parametrize("d", WIDTHS)
def test_energy_in_the_rest_in_the_head_and_zero_rest(d):
    rs = np.random.RandomState(1000 + d)
    _, _, _, (s0, s1) = layout(d)
    s1 = min(s1, d)
    X = lorentz_rows(rs, 96, d, 0.05)
    rest = np.arange(s0, s1)
    head = np.setdiff1d(np.arange(d), rest)
    X[0:24][:, 1 + head] = 0.0                      # all energy in the rest slots
    X[0:24][:, 1 + rest] *= 4.0
    X[12:24] = X[0:12]                              # ... in pairs of duplicates: Cauchy-Schwarz is tight there
    X[24:48][:, 1 + rest] = 0.0                     # all energy in the head, zero rest
    X[48:52, 1:] = 0.0                              # the origin
    X[52:60][:, 1 + rest[1:]] = 0.0                 # one rest coordinate only
    X[60:64] = X[52:56]
    worst, rb = check_table(reproject(X), d)
    assert worst <= 1.0
    assert (rb[24:52] == 0).all() and (rb[:24] >= 0x0080).all()


@pytest.mark.parametrize("d", WIDTHS)
def test_large_entries_and_tiny_entries(d):
    rs = np.random.RandomState(2000 + d)
    X = lorentz_rows(rs, 96, d, 1.0)
    X[:, 1:] *= rs.choice(np.array([1.0, 30.0, 2.0e3, 8.0e5], np.float32), size=(96, 1))        # entries up to 8e5
    X[90:96, 1:] = (rs.randn(6, d) * 1e-30).astype(np.float32)                                   # squares underflow in fp32
    X[88, 1:] = np.float32(1e-42)                                                                # round to 0 as bf16
    X[89, 1:] = np.float32(4e-40)                                                                # subnormal as bf16
    X[40] = X[7]
    worst, rb = check_table(reproject(X), d)
    assert worst <= 1.0
    assert rb[88] == 0 and (rb[89:96] >= 0x0080).all()                                           # never subnormal; 0 only for a zero rest


@pytest.mark.parametrize("d", WIDTHS)
def test_huge_row_and_nonfinite_rows(d):
    rs = np.random.RandomState(3000 + d)
    _, _, _, (s0, s1) = layout(d)
    X = lorentz_rows(rs, 96, d, 0.05)
    X[10, 1:] = np.float32(1.0e19)                  # |x|^2 overflows fp32: x0 = inf, the row is no candidate ...
    X[11, 1 + s0] = np.float32(1.0e19)              # ... one such entry does not: 1e38 < 3e38, delta becomes huge
    X[12, 1 + s0 + 1] = np.nan
    X[13, 2] = np.nan
    X[14, 1 + s0 + 2] = np.inf
    X[15, 3] = -np.inf
    X = reproject(X)
    X[16, 0] = np.nan
    X[17, 0] = np.inf
    X[18] = np.nan
    X[20] = X[21]
    worst, rb = check_table(X, d)
    assert worst <= 1.0
    r = bf16_val(rb)
    assert np.isnan(r[12]) and np.isnan(r[18]) and np.isfinite(np.delete(r, [12, 18])).all()      # finite unless a rest entry is NaN
    assert rb[14] == 0x7F7F and rb[10] < 0x7F7F         # an inf rest entry is clamped; 8e19 is an ordinary bf16


@pytest.mark.parametrize("d", WIDTHS)
def test_rest_norm_is_an_upper_bound(d):
    """r^ as the device computes it against the exact norm of the bf16-rounded rest entries (rational arithmetic)"""
    rs = np.random.RandomState(4000 + d)
    kc, _, _, (s0, s1) = layout(d)
    s1 = min(s1, d)
    n = 48
    S = (rs.randn(n, d) * rs.choice([1e-30, 1e-12, 1e-3, 0.05, 1.0, 3e4, 8e5, 1e18], size=(n, 1))).astype(np.float32)
    S[0] = 0.0
    S[1, s0:s1] = 0.0
    S[2] = np.float32(4e-40)
    S[3] = np.float32(3.0e38)
    rb = rest_norm_bits(S, d, kc)
    r = bf16_val(rb)
    assert np.isfinite(r).all() and rb[0] == 0 and rb[1] == 0 and rb[2] == 0x0080 and rb[3] == 0x7F7F
    vals = bf16(S[:, s0:s1])
    for i in range(n):
        if i == 3:
            continue                                 # clamped: the one row whose rest norm no finite bf16 holds
        exact = sum(Fraction(float(v)) ** 2 for v in vals[i])
        assert Fraction(float(r[i])) ** 2 >= exact, i
        if rb[i] > 0x0080:                           # and tight: the bf16 below r^ is below the norm (up to the helper's margin)
            below = Fraction(float(bf16_val(np.uint32(rb[i] - 1))))
            assert below ** 2 < exact * (1 + Fraction(1, 2 ** 38)), i
