// hm_scan_plan.h -- the pair scan's host policy: which rows and columns a launch covers, its block shape, and the list of work
// items its blocks walk -- encode (hm_scan_plan, host) and decode (HM_SCAN_ITEM_DECODE: the kernel; hm_scan_item: the host) in
// one place.  Plain C++, no HIP, no engine, no allocation: hm_prepare_scan (hm_scan.hip) copies the plan into
// ScanArgs, the kernel expands the decode, and tests/scan_plan_driver.cpp runs both on the CPU.  Search results never depend
// on the list's geometry.
//
// The list: a 1-D grid of items in up to HM_SCAN_PHASES phases.  Phase q covers the row blocks from rb0[q] up to the next
// phase's first; each of its items[q] items takes ch[q] column tiles (item b of the phase: row block rb0[q] + b / chunks[q],
// tiles from ctmin[q] + (b % chunks[q]) * ch[q]).  Chunk lengths shrink from phase to phase: long items first, ever shorter
// ones behind them, so that the slots that free up late are filled with work that still ends with the rest (the launch's
// tail is made of the shortest blocks).  An item's tile range is clamped on decode: to the diagonal of its row block (left
// of it there is no i < j), to col_begin, and to the table's last tile; what is left may be empty.
#pragma once
#include <stdint.h>

#include <algorithm>

#include "hm_scan_geom.h"

#define HM_SCAN_PHASES 6

struct ScanItems {
    int n_ph;
    int items[HM_SCAN_PHASES], rb0[HM_SCAN_PHASES], chunks[HM_SCAN_PHASES], ch[HM_SCAN_PHASES], ctmin[HM_SCAN_PHASES];
};

// work-decomposition knobs (hm_debug_set_knob; tuning builds also read HM_TUNE_<NAME>)
struct ScanPlanKnobs {
    int chunk_f32 = 32, chunk_bf16 = 128, tail_div = 4;   // (bf16: 96 with the static grid; 112-144 measure alike with the item queue)
    double tail_fraction = 0.20;
    // phases of the item list: work share of each phase from the top of the triangle (the last one takes the rest), chunk
    // length divisor per phase.  phases = 2 is the round-2 list: [1 - tail_fraction, tail_fraction] at [1, tail_div]
    int phases = 4;                      // (measured, interleaved A/B at V = 50 k / 100 k: +1.3 % / +2.6 % over the two-phase list)
    double ph_share[HM_SCAN_PHASES - 1] = {0.70, 0.15, 0.10, 0.0, 0.0};
    int ph_div[HM_SCAN_PHASES] = {1, 2, 4, 8, 16, 32};
    int force_shape = -1;                 // HM_TUNE_SHAPE: bf16 block shape of every launch (tuning builds)
    int64_t big_min_rows = 80000;         // bf16 form: launches covering at least the pairs of this many rows use 512-row blocks
};

// what a search asks for: a table of n rows, rows [row_begin, row_end) against partners j >= col_begin among the first
// n_limit rows (n_limit < 0: all; rows are only ever appended: the pairs of an earlier table), in which prefilter form
// head: 1 = an argmin search whose launch takes a head kernel (hm_scan.hip, HEAD > 0: 64-row waves only)
struct ScanRequest { int64_t n, row_begin, row_end, n_limit, col_begin; int bf16, KC; int head = 0; };
// ok = false: the row range is empty (nothing else is set)
struct ScanPlan {
    bool ok;
    int n, row_begin, row_end, col_begin;       // clamped
    int shape, rb_first, nct;                   // block shape (kScanShapes), first row block, column tiles = ceil(n / cols per tile)
    ScanItems items;
    int n_items;                                // the grid: one block per item (at least 1)
};

// pairs (i, j), i < j < n, with i in [r0, r1)
inline int64_t hm_pairs_in_range(int64_t n, int64_t r0, int64_t r1)
{
    // sum_{i=r0}^{r1-1} (n - 1 - i)
    const int64_t cnt = r1 - r0;
    return cnt * (n - 1) - (r0 + r1 - 1) * cnt / 2;
}

inline ScanPlan hm_scan_plan(const ScanPlanKnobs& k, const ScanRequest& rq)
{
    ScanPlan pl = {};
    const int64_t n = (rq.n_limit >= 0 && rq.n_limit < rq.n) ? rq.n_limit : rq.n;
    int64_t row_begin = rq.row_begin, row_end = rq.row_end;
    if (row_end < 0 || row_end > n) row_end = n;
    if (row_begin < 0) row_begin = 0;
    if (row_end > n - 1) row_end = n - 1;        // the last row has no partner j > i
    if (row_begin >= row_end) return pl;
    pl.ok = true;
    // large launches: 512-row blocks halve the L2 -> LDS fill traffic, which is what limits the bf16 form once the
    // launch tail no longer does (decided by the pairs this launch covers: a row-range search of a sharded run is
    // a small launch)
    const bool shaped = rq.bf16 && rq.KC <= HM_SCAN_BIG_MAX_KC;
    pl.shape = (shaped && hm_pairs_in_range(n, row_begin, row_end) >= k.big_min_rows * (k.big_min_rows - 1) / 2) ? 1 : 0;
    // ... but not where the launch takes a head kernel: that one exists for 256-row blocks only and beats the 512-row
    // kernel without the test at every size (100 000 rows: 0.569 against 0.773 ms per scan, profiles/scan_head_ring_ab.json)
    if (rq.head) pl.shape = 0;
    if (shaped && k.force_shape >= 0) pl.shape = k.force_shape;
    const int block_rows = hm_shape_rows(pl.shape);
    const int cols = 32 * (rq.bf16 ? HM_SUB_BF16 : HM_SUB_F32);     // partner rows per streamed tile
    pl.n = (int)n;
    pl.row_begin = (int)row_begin;
    pl.row_end = (int)row_end;
    pl.rb_first = (int)(row_begin / block_rows);
    pl.nct = (int)((n + cols - 1) / cols);
    const int rb_last = (int)((row_end - 1) / block_rows);
    const int nrb = rb_last - pl.rb_first + 1;
    // diagonal advance per row block in tiles (rounded down: the decode clamps to the exact diagonal)
    const int tiles_per_rb = std::max(1, block_rows / cols);
    // column tiles per block: amortise the stationary-row load, but keep enough blocks in flight.
    // (the knob is in 64-column units)
    int ch = (rq.bf16 ? k.chunk_bf16 : k.chunk_f32) * 64 / cols;
    if (ch < 1) ch = 1;
    while (ch > 4 && (int64_t)nrb * ((pl.nct + ch - 1) / ch) < 1024) ch >>= 1;
    // phases: cut the launch's row blocks (top down: longest rows first) at the cumulative work shares; chunk lengths
    // ch, ch / div[1], ch / div[2], ... (a small launch keeps one phase)
    pl.col_begin = (int)std::max<int64_t>(rq.col_begin, 0);
    const int ct_lo = pl.col_begin / cols;
    int nph = 1;
    double share[HM_SCAN_PHASES] = {1.0};
    int div[HM_SCAN_PHASES];
    for (int q = 0; q < HM_SCAN_PHASES; ++q) div[q] = 1;
    if (ch >= 8 && nrb >= 16) {
        if (k.phases <= 2) {
            nph = 2;
            share[0] = 1.0 - k.tail_fraction; share[1] = k.tail_fraction;
            div[1] = k.tail_div;
        } else {
            nph = std::min(k.phases, HM_SCAN_PHASES);
            double rest = 1.0;
            for (int q = 0; q < nph - 1; ++q) { share[q] = k.ph_share[q]; rest -= share[q]; }
            share[nph - 1] = std::max(rest, 0.0);
            for (int q = 0; q < nph; ++q) div[q] = k.ph_div[q];
        }
    }
    double total = 0.0;
    for (int rb = pl.rb_first; rb <= rb_last; ++rb) total += (double)std::max(0, pl.nct - rb * tiles_per_rb);
    ScanItems& it = pl.items;
    it.n_ph = nph;
    int rb_at = pl.rb_first, n_items = 0;
    double acc = 0.0, want = 0.0;
    for (int q = 0; q < nph; ++q) {
        want += share[q] * total;
        int rb_end = rb_at;
        if (q == nph - 1) rb_end = rb_last + 1;
        else while (rb_end <= rb_last && acc < want) { acc += (double)std::max(0, pl.nct - rb_end * tiles_per_rb); ++rb_end; }
        const int chq = std::max(1, ch / std::max(1, div[q]));
        it.rb0[q] = rb_at;
        it.ch[q] = chq;
        it.ctmin[q] = std::max((int)((int64_t)rb_at * block_rows / cols), ct_lo);
        it.chunks[q] = std::max(1, (pl.nct - it.ctmin[q] + chq - 1) / chq);
        it.items[q] = (rb_end - rb_at) * it.chunks[q];
        n_items += it.items[q];
        rb_at = rb_end;
    }
    pl.n_items = std::max(1, n_items);
    return pl;
}

// item -> its row block RB and its run of column tiles [CT0, CT1), clamped; CT0 >= CT1: nothing right of the diagonal.
// The statements stand in a macro because the kernel has to expand them in place: through a call -- an inlined one
// included -- hipcc allocates the registers of every scan kernel differently (SGPRs of the HIST kernels 60 -> 66), and this
// policy is not allowed to move the device code.  L: a ScanItems; every other argument an int expression, RB / CT0 / CT1 lvalues.
#define HM_SCAN_ITEM_DECODE(L, ITEM, BLOCK_ROWS, COLS, NCT, COL_BEGIN, RB, CT0, CT1)                                   \
    {                                                                                                                   \
        int it = (ITEM), ph = 0;                                                                                        \
        while (ph + 1 < (L).n_ph && it >= (L).items[ph]) { it -= (L).items[ph]; ++ph; }                                 \
        RB = (L).rb0[ph] + it / (L).chunks[ph];                                                                         \
        CT0 = (L).ctmin[ph] + (it % (L).chunks[ph]) * (L).ch[ph];                                                       \
        CT1 = CT0 + (L).ch[ph];                                                                                         \
    }                                                                                                                   \
    if (CT0 < (RB * (BLOCK_ROWS)) / (COLS)) CT0 = (RB * (BLOCK_ROWS)) / (COLS);   /* left of the diagonal: no i < j */ \
    if (CT0 < (COL_BEGIN) / (COLS)) CT0 = (COL_BEGIN) / (COLS);   /* partner rows in front of col_begin are not asked for */ \
    if (CT1 > (NCT)) CT1 = (NCT);

// the decode as a function: the host's (and the tests') form of the statements the kernel expands
inline void hm_scan_item(const ScanItems& l, int item, int block_rows, int cols, int nct, int col_begin, int* rb, int* ct0, int* ct1)
{
    HM_SCAN_ITEM_DECODE(l, item, block_rows, cols, nct, col_begin, *rb, *ct0, *ct1)
}
