// hm_scan_geom.h -- the pair scan's geometry, once: what follows from a kernel's template arguments (row and tile sizes, the
// LDS map, threads per block), the table of block shapes and the list of instantiated widths.
// Constexpr values only; compiles for host and device and without HIP.  The kernel (hm_scan.hip) reads its constants from
// ScanGeom, the launch sizes the dynamic LDS with ScanGeom::lds_bytes, the item plan (hm_scan_plan.h) takes a shape's rows
// per block from the table the dispatch instantiates from, and the engine picks a table's width from the list the dispatch
// switches over.
#pragma once
#include "hm_tie_slack.h"

#define HM_MAX_BLOCK_ROWS 1024     // rows of the largest block shape (kScanShapes): the slack of the images' rows_alloc
#define HM_MODE_TOPK 0
#define HM_MODE_ARGMIN 1
#define HM_MODE_HIST 2
#define HM_HIST_BINS 256

#ifndef HM_SUB_BF16
#define HM_SUB_BF16 4              // bf16 form: 32-column groups per streamed tile (128 partner rows per barrier)
#endif
#ifndef HM_SUB_F32
#define HM_SUB_F32 2
#endif
#ifndef HM_DIST_BF16
#define HM_DIST_BF16 1             // tiles in flight ahead of the computed one (ring of DIST + 1 slots)
#endif
#ifndef HM_SCAN_INSTANTIATE_ALL
#define HM_SCAN_INSTANTIATE_ALL 1  // 0: only d = 100 (13 chunks / NG = 25) -- quick builds for tuning runs
#endif
#ifndef HM_SCAN_ALL_SHAPES
#define HM_SCAN_ALL_SHAPES 0       // 1: block shapes 2 .. 4 as well (tuning builds only)
#endif

// floats per fp32 image row
HM_HOST_DEVICE_INLINE constexpr int hm_row_floats(int NG) { return 4 * NG + 4 + (((NG + 1) % 2 == 0) ? 4 : 0); }
// 16-byte chunks per bf16 image row: KC chunks of 8 K-slots (+ the [x0] chunk that makes an even count odd)
HM_HOST_DEVICE_INLINE constexpr int hm_row16_chunks(int KC) { return KC + ((KC & 1) ? 0 : 1); }

// ---- instantiated widths: X(width) for every width a table can have, ascending; REST(...) wraps the ones a quick build
// (HM_SCAN_INSTANTIATE_ALL = 0) leaves out.  The engine's tables (hm_pick_ng / hm_pick_kc) list every width (HM_SCAN_WIDTHS_ALL);
// the dispatch of hm_launch_scan switches over the built ones (HM_SCAN_WIDTHS_BUILT).
// fp32 form: NG = groups of 4 spatial coordinates
#define HM_SCAN_NG_LIST(X, REST) REST(X(1) X(2) X(3) X(4) X(6) X(8) X(10) X(13) X(16) X(20)) X(25) REST(X(28) X(32))
// bf16 form: KC = chunks of 8 K-slots (two per k-step; 13 ends on a half step)
#define HM_SCAN_KC_LIST(X, REST) REST(X(2) X(4) X(8)) X(13) REST(X(14) X(16))
#define HM_SCAN_WIDTHS_ALL(...) __VA_ARGS__
#if HM_SCAN_INSTANTIATE_ALL
#define HM_SCAN_WIDTHS_BUILT(...) __VA_ARGS__
#else
#define HM_SCAN_WIDTHS_BUILT(...)
#endif

// ---- block shapes: index = ScanArgs::shape, entry = {TM, WPB}: WPB waves of 32 * TM stationary rows each.
//   0  4 waves x  64 rows = 256-row blocks, two accumulator sets; the fp32 form's only shape
//   1  4 waves x 128 rows = 512-row blocks: half the L2 -> LDS fill traffic and half the LDS fragment reads per flop,
//      one accumulator set (bf16 form, large launches: ScanPlanKnobs::big_min_rows)
//   2  8 x 64, 3  8 x 128, 4  4 x 96 (HM_SCAN_ALL_SHAPES builds only)
struct ScanShape { int tm, wpb; };
#define HM_SCAN_SHAPES 5
constexpr ScanShape kScanShapes[HM_SCAN_SHAPES] = {{2, 4}, {4, 4}, {2, 8}, {4, 8}, {3, 4}};
#define HM_SCAN_BIG_MAX_KC 14      // shapes other than 0 exist up to this width (16 chunks would not fit the registers of the 128-row waves)
HM_HOST_DEVICE_INLINE constexpr int hm_shape_rows(int shape) { return 32 * kScanShapes[shape].tm * kScanShapes[shape].wpb; }
HM_HOST_DEVICE_INLINE constexpr int hm_shape_rows_max(int shape = 0)
{
    return shape == HM_SCAN_SHAPES ? 0 : (hm_shape_rows(shape) > hm_shape_rows_max(shape + 1) ? hm_shape_rows(shape) : hm_shape_rows_max(shape + 1));
}
static_assert(hm_shape_rows_max() == HM_MAX_BLOCK_ROWS, "the images are allocated with one largest block of slack rows");

// ---- what follows from a kernel's template arguments.  LDS map of a block (dynamic shared memory, from offset 0):
//   ring    NBUF slots of TILE_LDS bytes: the streamed partner tiles
//   slack   32 rows: the early request of "the next group's" first fragments behind the last group of the last slot lands
//           here and is never used.  HIST mode keeps its HM_HIST_BINS bins at the same offset (they are only read by that
//           request) and the slack's bytes behind them
//   queue   16 bytes: the item queue's broadcast word
template <int NG, int BF, int TM, int WPB, int SUB>
struct ScanGeom {
    static constexpr int COLS = 32 * SUB;                   // partner rows per streamed tile
    static constexpr int RS = hm_row_floats(NG);            // fp32 image: floats per row
    static constexpr int RB16 = 16 * hm_row16_chunks(NG);   // bf16 image: bytes per row (NG chunks of 8 bf16 [+ the [x0 fp32] chunk])
    static constexpr int ROW_BYTES = BF ? RB16 : RS * 4;
    static constexpr int TILE_BYTES = COLS * ROW_BYTES;
    static constexpr int NP = BF ? (NG + 1) / 2 : NG + 1;   // k-steps: fp32: NG spatial groups + time; bf16: two chunks per step
    static constexpr int NPIECE = TILE_BYTES / 1024;        // 1 KiB pieces per tile
    static constexpr int PPW = (NPIECE + WPB - 1) / WPB;    // LDS-DMA pieces per wave and tile (slot padded to PPW * WPB KiB)
    static constexpr int TILE_LDS = PPW * WPB * 1024;       // LDS bytes per ring slot
    static constexpr int DIST = BF ? HM_DIST_BF16 : 1;      // tiles in flight ahead of the one being computed
    static constexpr int NBUF = DIST + 1;                   // ring slots
    static constexpr int WAVE_ROWS = 32 * TM;
    static constexpr int BLOCK_ROWS = WPB * WAVE_ROWS;
    static constexpr int NTHREADS = 64 * WPB;
    static_assert(TILE_BYTES % 1024 == 0, "tiles are moved in 1 KiB pieces");
    static_assert(DIST * PPW <= 60, "the counted wait must fit vmcnt");

    static constexpr int RING_BYTES = NBUF * TILE_LDS;
    static constexpr int SLACK_BYTES = 32 * ROW_BYTES;
    static constexpr int HIST_OFF = RING_BYTES;
    static constexpr int QUEUE_BYTES = 16;
    HM_HOST_DEVICE_INLINE static constexpr int queue_off(int mode)
    {
        return RING_BYTES + SLACK_BYTES + (mode == HM_MODE_HIST ? 4 * HM_HIST_BINS : 0);
    }
    HM_HOST_DEVICE_INLINE static constexpr int lds_bytes(int mode) { return queue_off(mode) + QUEUE_BYTES; }
};
