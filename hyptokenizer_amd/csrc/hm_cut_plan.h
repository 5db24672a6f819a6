// hm_cut_plan.h -- the emission cut of a top-k search: which pass comes next, and with which cut.
// Plain host C++, no HIP, no engine, no allocation: the driver (hm_topk_core_form, hm_search.hip) does what the plan names --
// a cut estimate from sampled histograms (hm_estimate_cut) or a scan pass --, reports what came back and asks again.
//
// The cut is a bit pattern of u' (entries with bits(u') <= cut are emitted) plus, for a tie flood at u' = 1, a row limit
// (zero-distance pairs are emitted for rows i <= tie_imax only).  CutSearch keeps a bracket of the cut: `tight`, the largest
// cut whose complete region held fewer than `want` entries, and `loose`, the smallest cut that overflowed the buffer.
//
//   last action   what came back                                         next
//   (start)       list_all                                               scan, emit all
//   (start)       k == 0 (a pure count)                                  scan, cut = bits(1.0), tie_imax = -1
//   (start)       a remembered cut applies                               scan, that cut (slack added by the caller)
//   (start)       otherwise                                              estimate, target 4k + 4096; then scan what it gives
//   scan          a margin violation                                     fail HM_E_STATE (before anything else is looked at)
//   scan          overflow, list_all                                     fail HM_E_CAPACITY
//   scan          overflow, no tie flood, tight known (!= 0)             loose = min(loose, cut); loose <= tight + 1: fail
//                                                                        HM_E_CAPACITY; else scan the midpoint
//   scan          overflow otherwise                                     (no tie flood: loose = min(loose, cut)) estimate,
//                                                                        target max((2k + 1024) >> min(attempt, 20), k + 64)
//   estimate      (after an overflow) emit all                           fail HM_E_CAPACITY
//   estimate      (after an overflow) no tie flood, target == k + 64,    fail HM_E_CAPACITY: the same overflowing cut at the
//                 cut >= loose, for the second time                      smallest target again (stuck)
//   estimate      (after an overflow) otherwise                          scan that cut
//   scan          fits; not everything emitted and complete < want:
//                   tie flood                                            tie_imax * 4 + 256, "all rows" from row_end on; scan
//                   no tie flood                                         tight = max(tight, cut); nb = cut + max(cut - bits(1.0),
//                                                                        4 * hm_tie_slack(cut)) in 64 bits; nb >= loose (known):
//                                                                        loose <= tight + 1: fail HM_E_CAPACITY, else the
//                                                                        midpoint; otherwise nb (emit all from +inf on); scan
//   scan          fits otherwise                                         done (total, valid)
//
// want = min(k, total) when the total is known (everything emitted: the valid entries; counted: sure + borderline), else k.
// Every scan but the first costs one attempt -- whether it follows a bisection, a widening or a fresh estimate --; instead of
// the 41st scan the search fails with HM_E_CAPACITY.  `loose` is lowered only while no tie flood is active.
#pragma once
#include <stdint.h>

#include "../../include/hypmerge.h"
#include "hm_tie_slack.h"

#define HM_CUT_ALL 0xffffffffu        // cut: every candidate is emitted
#define HM_CUT_ONE 0x3f800000u        // bits(1.0f): u' = 1, distance 0
#define HM_TIE_ALL_ROWS 0x7fffffff    // tie_imax: no row limit (no tie flood)
#define HM_CUT_ATTEMPTS 40

// First bin at which the running count, starting from `below`, reaches `want`: the bin, the count below it and the count in
// it; bin = -1 (and below = everything) when it is never reached.  ACC = double with a scale for sampled histograms, the
// bins' own integer type otherwise.
template <class ACC>
struct BinHit { int bin; ACC below, in; };
template <class ACC, class BIN>
inline BinHit<ACC> hm_first_bin(const BIN* hist, uint32_t nbins, ACC below, ACC want, ACC scale = 1)
{
    ACC cum = below;
    for (uint32_t q = 0; q < nbins; ++q) {
        const ACC in = (ACC)hist[q] * scale;
        if (cum + in >= want) return {(int)q, cum, in};
        cum += in;
    }
    return {-1, cum, 0};
}

// ---- one zoom of the cut estimate (hm_estimate_cut) ----
// sample stride of the histogram passes: every stride-th tile.  Past C(131 072, 2) pairs a tie flood puts every sample into
// one 32-bit bin -- at most ~pairs / stride of them (plus one tile per row block), so the stride keeps growing until that
// stays below 2^30
inline int hm_estimate_stride(int64_t pairs)
{
    int stride = 1;
    while (stride < 64 && pairs / (stride * 2) > 40000000) stride *= 2;
    while (pairs / stride > ((int64_t)1 << 30)) stride *= 2;
    return stride;
}

struct CutWindow { uint32_t lo_bits, hi_bits; double base; };      // bits of u' in [lo, hi); estimated entries below lo

inline uint32_t hm_zoom_shift(const CutWindow& w, uint32_t nbins)
{
    uint32_t shift = 0;
    while (((w.hi_bits - w.lo_bits) >> shift) > nbins) ++shift;
    return shift;
}

struct ZoomDecision {
    enum Kind { EMIT_ALL, ZOOM, CUT, CUT_TIE_FLOOD } kind;
    uint32_t cut_bits;          // CUT, CUT_TIE_FLOOD
    int tie_imax;               // CUT_TIE_FLOOD
    CutWindow window;           // ZOOM: the bin to look into
};

// hist: the nbins bins of window w read back (bin width 1 << hm_zoom_shift(w, nbins)), every stride-th tile sampled.
// (The sums are integers below 2^53, exact in double: `below` of the selected bin is what the caller's running sum was.)
inline ZoomDecision hm_zoom_decide(const uint32_t* hist, uint32_t nbins, int stride, const CutWindow& w, int64_t target,
                                   uint32_t ent_cap, int n, int row_begin, int row_end)
{
    ZoomDecision z = {ZoomDecision::EMIT_ALL, HM_CUT_ALL, HM_TIE_ALL_ROWS, w};
    const BinHit<double> hit = hm_first_bin<double>(hist, nbins, w.base, (double)target, (double)stride);
    if (hit.bin < 0) return z;                                  // fewer than target below u_hi: emit all
    const uint32_t shift = hm_zoom_shift(w, nbins);
    const double cum = hit.below + hit.in;
    const uint32_t edge_lo = w.lo_bits + ((uint32_t)hit.bin << shift);
    const uint32_t edge_hi = w.lo_bits + (((uint32_t)hit.bin + 1u) << shift);   // exclusive
    if (cum > (double)ent_cap * 0.5 && shift != 0) {
        z.kind = ZoomDecision::ZOOM;
        z.window = {edge_lo, edge_hi, hit.below};
        return z;
    }
    z.kind = ZoomDecision::CUT;
    z.cut_bits = edge_hi - 1u;
    if (cum > (double)ent_cap * 0.5) {
        // a single value of u' holds more entries than the buffer: tie flood.  Emit the tie
        // value only for the first rows; rows are visited in row-major order by the selection.
        const double per_row = hit.in / (double)(row_end - row_begin);
        const double rows = ((double)target - hit.below) / (per_row > 1e-9 ? per_row : 1e-9);
        // (a slack of 64 rows, fewer where 64 rows of partners would fill more than half the buffer)
        int64_t pad = 64;
        while (pad > 1 && pad * (int64_t)n > (int64_t)ent_cap / 2) pad >>= 1;
        int64_t imax = row_begin + (int64_t)(rows * 2.0) + pad;
        if (imax > row_end) imax = row_end;
        z.kind = ZoomDecision::CUT_TIE_FLOOD;
        z.tie_imax = (int)imax;
    }
    return z;
}

// ---- the search for a cut that completes `want` entries and fits the buffer ----
struct PassOutcome {                 // what one scan pass + exact distances reported
    uint64_t emitted;                // entries the scan emitted (may exceed the buffer: overflow)
    int64_t valid;                   // emitted entries below the threshold
    int64_t borderline;              // valid entries the prefilter was not sure of
    int64_t sure;                    // pairs the prefilter counted as surely below the threshold
    int64_t complete;                // valid entries of the complete region
    uint32_t margin_violations;      // sure entries that are not valid: must be 0
};

struct CutAction {
    enum Kind { ESTIMATE, SCAN, DONE, FAIL } kind;
    int64_t target;                  // ESTIMATE
    uint32_t cut_bits;               // SCAN
    int tie_imax;
    int64_t total, valid;            // DONE: exact candidate count (-1: not counted, at least k) and valid entries emitted
    int status;                      // FAIL
    const char* message;
};

struct CutSearchInput {
    int64_t k;
    bool list_all, count_sure;
    uint32_t ent_cap;
    int row_begin, row_end;
    bool have_cut;                   // a remembered cut applies
    uint32_t cut_bits;               //   its bits, slack added
};

class CutSearch {
public:
    explicit CutSearch(const CutSearchInput& in) : in_(in)
    {
        if (!in.list_all && in.k == 0) { cut_ = HM_CUT_ONE; tie_ = -1; }     // nothing has to be emitted but the undecided shell
        else if (!in.list_all && in.have_cut) cut_ = in.cut_bits;
        if (in.list_all || in.k == 0 || in.have_cut) scan();
        else estimate(4 * in.k + 4096);
    }

    const CutAction& next() const { return act_; }

    // the estimate asked for came back (hm_estimate_cut starts from "emit all": that is its answer when it finds no cut)
    void estimated(uint32_t cut_bits, int tie_imax)
    {
        cut_ = cut_bits;
        tie_ = tie_imax;
        if (!after_overflow_) return scan();
        after_overflow_ = false;
        if (cut_ == HM_CUT_ALL) return fail_unbounded();
        // the smallest target already, and its cut is one that is known to overflow: estimating again would give the same
        // cut (a table too dense for any cut of this prefilter form -- the caller moves on to the next form / the exact path)
        if (tie_ == HM_TIE_ALL_ROWS && act_.target == in_.k + 64 && cut_ >= loose_ && ++stuck_ >= 2) return fail_unbounded();
        retry();
    }

    // the scan asked for came back
    void scanned(const PassOutcome& o)
    {
        if (o.margin_violations != 0)
            return fail(HM_E_STATE, "pair scan: prefilter margin violated (an entry classified as surely below the "
                                    "threshold is not); table holds non-finite rows other than all-NaN rows?");
        const bool flood = tie_ != HM_TIE_ALL_ROWS;
        if (o.emitted > in_.ent_cap) {
            if (in_.list_all) return fail(HM_E_CAPACITY, "candidate listing: more candidates than the emission buffer holds");
            if (!flood && cut_ < loose_) loose_ = cut_;
            // In high dimensions the distances are so concentrated that P(u - 1 < x) grows like x^(d/2): widening a tight cut
            // geometrically overshoots by orders of magnitude and a fresh estimate undershoots again -- once both sides are
            // known the cut is bisected between them
            if (!flood && tight_ != 0u) return bisect();
            // estimate was too generous (or none was made): estimate with a smaller target
            after_overflow_ = true;
            const int64_t t = (2 * in_.k + 1024) >> (attempt_ < 20 ? attempt_ : 20);
            return estimate(t > in_.k + 64 ? t : in_.k + 64);
        }
        // exact total (when counted): sure + valid borderline; everything emitted: the valid ones
        const bool emitted_all = cut_ == HM_CUT_ALL && !flood;
        const int64_t total = emitted_all ? o.valid : (in_.count_sure ? o.sure + o.borderline : -1);
        const int64_t want = (total >= 0 && total < in_.k) ? total : in_.k;
        if (emitted_all || o.complete >= want) {
            act_ = CutAction{CutAction::DONE, 0, cut_, tie_, total, o.valid, HM_OK, nullptr};
            return;
        }
        // fewer than `want` entries lie in the region that is known to be complete: the cut was too tight.
        // Widen geometrically in the ulp domain (rows for a tie flood) and retry.
        if (flood) {
            const int64_t wider = (int64_t)tie_ * 4 + 256;
            tie_ = (tie_ >= in_.row_end || wider >= in_.row_end) ? HM_TIE_ALL_ROWS : (int)wider;
            return retry();
        }
        if (cut_ > tight_) tight_ = cut_;
        const uint32_t span = cut_ - HM_CUT_ONE, slack4 = 4u * hm_tie_slack(cut_);
        const uint64_t nb = (uint64_t)cut_ + (span > slack4 ? span : slack4);
        if (loose_ != HM_CUT_ALL && nb >= (uint64_t)loose_) return bisect();
        cut_ = nb >= 0x7f800000ull ? HM_CUT_ALL : (uint32_t)nb;
        retry();
    }

private:
    void estimate(int64_t target) { act_ = CutAction{CutAction::ESTIMATE, target, cut_, tie_, 0, 0, HM_OK, nullptr}; }
    void scan()
    {
        if (attempt_ >= HM_CUT_ATTEMPTS) return fail(HM_E_CAPACITY, "top-k: emission cut did not converge");
        act_ = CutAction{CutAction::SCAN, 0, cut_, tie_, 0, 0, HM_OK, nullptr};
    }
    void retry() { ++attempt_; scan(); }
    void fail(int status, const char* message) { act_ = CutAction{CutAction::FAIL, 0, cut_, tie_, 0, 0, status, message}; }
    void fail_unbounded() { fail(HM_E_CAPACITY, "top-k: could not bound the emission"); }
    // (a bracket that cannot be split: the shell of undecided pairs around the cut alone overflows the buffer -- the caller
    // retries with the fp32 prefilter, whose shell is ~100x thinner)
    void bisect()
    {
        if (loose_ <= tight_ + 1u) return fail_unbounded();
        cut_ = tight_ + (loose_ - tight_) / 2u;
        retry();
    }

    const CutSearchInput in_;
    CutAction act_ = {};
    uint32_t cut_ = HM_CUT_ALL;
    int tie_ = HM_TIE_ALL_ROWS;
    uint32_t tight_ = 0u, loose_ = HM_CUT_ALL;
    int stuck_ = 0, attempt_ = 0;
    bool after_overflow_ = false;
};
