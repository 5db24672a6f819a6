// Stand-alone driver of CutSearch and hm_zoom_decide (hyptokenizer_amd/csrc/hm_cut_plan.h) for tests/test_cut_plan.py: no
// HIP, no engine.  It does what hm_topk_core_form / hm_estimate_cut (hm_search.hip) do with the plan, minus the device work.
// stdin:  per case a line "case K LIST_ALL COUNT_SURE ENT_CAP N ROW_BEGIN ROW_END HAVE_CUT CUT_BITS PAIRS HI_BITS", then, as
//         the plan asks for them, "h NNZ (BIN COUNT)*" -- one sampled histogram -- and
//         "p EMITTED VALID BORDERLINE SURE COMPLETE MARGIN_VIOLATIONS" -- one scan pass.
// stdout: per case "case", then the actions: "estimate TARGET" followed by "fits" or one "hist LO SHIFT STRIDE" per
//         histogram pass and "cut BITS TIE_IMAX"; "scan BITS TIE_IMAX"; last "done TOTAL VALID" or "fail STATUS MESSAGE".
//         "starved" when the script ends before the plan does.
#include <stdio.h>
#include <string.h>

#include "../hyptokenizer_amd/csrc/hm_cut_plan.h"

#define BINS 256u

static bool read_hist(uint32_t* hist)
{
    unsigned nnz = 0;
    memset(hist, 0, sizeof(uint32_t) * BINS);
    if (scanf(" h %u", &nnz) != 1) return false;
    for (unsigned t = 0; t < nnz; ++t) {
        unsigned bin = 0, count = 0;
        if (scanf(" %u %u", &bin, &count) != 2 || bin >= BINS) return false;
        hist[bin] = count;
    }
    return true;
}

// hm_estimate_cut without its launches
static bool estimate(long long pairs, uint32_t hi_bits, long long target, uint32_t ent_cap, int n, int row_begin, int row_end,
                     uint32_t* cut_bits, int* tie_imax)
{
    static uint32_t hist[BINS];
    *cut_bits = HM_CUT_ALL;
    *tie_imax = HM_TIE_ALL_ROWS;
    if (pairs <= (long long)ent_cap / 2) { printf("fits\n"); return true; }
    CutWindow w = {HM_CUT_ONE, hi_bits, 0.0};
    const int stride = hm_estimate_stride(pairs);
    for (int zoom = 0; zoom < 6; ++zoom) {
        printf("hist %u %u %d\n", w.lo_bits, hm_zoom_shift(w, BINS), stride);
        if (!read_hist(hist)) return false;
        const ZoomDecision z = hm_zoom_decide(hist, BINS, stride, w, target, ent_cap, n, row_begin, row_end);
        if (z.kind != ZoomDecision::ZOOM) {
            *cut_bits = z.cut_bits;
            *tie_imax = z.tie_imax;
            return true;
        }
        w = z.window;
    }
    return true;
}

int main()
{
    long long k = 0, pairs = 0;
    int list_all = 0, count_sure = 0, n = 0, row_begin = 0, row_end = 0, have_cut = 0;
    unsigned ent_cap = 0, cut_bits = 0, hi_bits = 0;
    while (scanf(" case %lld %d %d %u %d %d %d %d %u %lld %u", &k, &list_all, &count_sure, &ent_cap, &n, &row_begin, &row_end, &have_cut,
                 &cut_bits, &pairs, &hi_bits) == 11) {
        printf("case\n");
        const CutSearchInput in = {k, list_all != 0, count_sure != 0, ent_cap, row_begin, row_end, have_cut != 0, cut_bits};
        CutSearch plan(in);
        for (int asked = 0;; ++asked) {
            const CutAction act = plan.next();
            if (asked > 200) { printf("runaway\n"); return 1; }
            if (act.kind == CutAction::DONE) { printf("done %lld %lld\n", (long long)act.total, (long long)act.valid); break; }
            if (act.kind == CutAction::FAIL) { printf("fail %d %s\n", act.status, act.message); break; }
            if (act.kind == CutAction::ESTIMATE) {
                printf("estimate %lld\n", (long long)act.target);
                uint32_t cut = 0;
                int tie = 0;
                if (!estimate(pairs, hi_bits, act.target, ent_cap, n, row_begin, row_end, &cut, &tie)) { printf("starved\n"); return 1; }
                printf("cut %u %d\n", cut, tie);
                plan.estimated(cut, tie);
                continue;
            }
            printf("scan %u %d\n", act.cut_bits, act.tie_imax);
            unsigned long long emitted = 0;
            long long valid = 0, borderline = 0, sure = 0, complete = 0;
            unsigned margin = 0;
            if (scanf(" p %llu %lld %lld %lld %lld %u", &emitted, &valid, &borderline, &sure, &complete, &margin) != 6) { printf("starved\n"); return 1; }
            const PassOutcome o = {emitted, valid, borderline, sure, complete, margin};
            plan.scanned(o);
        }
    }
    return 0;
}
