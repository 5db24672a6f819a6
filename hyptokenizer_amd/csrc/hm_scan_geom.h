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

// ---- partner-tile rings: index = the kernels' RING argument, entry = {sub, dist, exact, blocks}.  A ring slot holds `sub`
// 32-column groups (0: the kernel's SUB), `dist` tiles are in flight ahead of the computed one (0: HM_DIST_BF16 / 1), and
// with `exact` every wave moves its exact share of the tile's pieces and a slot is as large as the tile (otherwise every
// wave moves PPW pieces and the slot is padded to PPW * WPB KiB).  Ring 0 is every kernel's but the head kernels' of the
// argmin scan, which compute a 64-column tile in a third of the time its landing takes: they keep narrower slots and
// more of them in flight in the same LDS (two blocks per CU: at most 80 KiB per block).  The item plan's tile
// (hm_scan_plan.h) stays 32 * SUB columns for every ring; a kernel with narrower slots walks an item's run in its own tiles.
//   1  64-column slots padded to 16 KiB: 4 slots, 3 tiles (40 KB at 13 chunks) in flight
//   2  64-column slots of the tile's own 13 KiB: 5 slots, 4 tiles (53 KB) in flight
//   3  64-column slots of the tile's own size, four of them and no slack region behind them (`blocks` = 3): 52 KiB + the
//      queue word at 13 chunks, so that THREE blocks share a CU -- its kernels are built for three waves per SIMD.  Defined
//      for span 2 and for the widths at which three blocks fit (2, 4, 8 and 13 chunks); asked for at another width or with
//      span 1 it IS ring 1 (ScanGeom::RING, a constant of the instantiation: nothing is decided at run time)
struct ScanRing { int sub, dist, exact, blocks; };     // blocks: resident blocks per CU the LDS map is cut for (0: two, with the slack region)
#define HM_SCAN_RINGS 4
#define HM_SCAN_RINGS_TWO_BLOCK 3      // rings 0 .. 2, the values of the knob `head_ring`; ring 3 is the knob `head_blocks` = 3
constexpr ScanRing kScanRings[HM_SCAN_RINGS] = {{0, 0, 0, 0}, {2, 3, 0, 0}, {2, 4, 1, 0}, {2, 3, 1, 3}};
#define HM_LDS_PER_CU (160 * 1024)
#define HM_LDS_GRANULE 1280            // a block's LDS is allocated in units of this many bytes
HM_HOST_DEVICE_INLINE constexpr int hm_lds_alloc(int bytes) { return (bytes + HM_LDS_GRANULE - 1) / HM_LDS_GRANULE * HM_LDS_GRANULE; }
// the head kernels' ring (knob `head_ring`).  Measured at 50 000 rows, interleaved in one process (profiles/scan_head_ring_ab.json):
// ring 1 takes 2.5 - 4 % off the scan launch of ring 0; ring 2 -- a third more in flight and no padding traffic -- none.
// Ring 3 (three blocks per CU), interleaved with ring 1 x span 2 and with the parent's library (profiles/scan_head_ring3_ab.json):
// 4 % off the scan launch at 50 000 rows and 7 % at 100 000 in every run; level at 30 000 and 40 000, 1 - 4 % behind at 20 000
// and 70 000 (the item list's phases were cut for 512 resident blocks, not 768)
#define HM_SCAN_HEAD_RING_DEFAULT 3
// slots the head kernels compute per barrier (knob `head_span`; ring 0 has none to choose).  Measured at 50 000 and 100 000
// rows, interleaved in one process (profiles/scan_head_span_ab.json): span 2 takes 16 % and 12 % off the scan launch of
// span 1 on ring 1, and ring 2 x span 2 is within half a percent of ring 1 x span 2 at either size
#define HM_SCAN_HEAD_SPAN_DEFAULT 2
#define HM_LDS_PER_BLOCK (80 * 1024)  // half of a CU's 160 KiB: what a block may use with two blocks resident

// ---- the walk of a run over a ring: `span` consecutive slots are computed between two barriers (a compute tile); span 1
// is the walk of every kernel but the span-2 head kernels (knob `head_span`).  A run of `ntile` slots over `nbuf` ring
// slots, slot s in ring slot s % nbuf:
//   prologue    requests slots 0 .. nbuf - span - 1 (those the run has) and waits for all of them
//   tile k      computes slots k * span .. (an odd run ends on a tile of fewer); at its start it requests the slots
//               nbuf + (k - 1) * span .. nbuf + k * span - 1 -- into the ring slots tile k - 1 computed, which every wave left
//               at the barrier in between --; its wait, in front of the barrier that ends it, lets the slots of tile k + 1 land
// Tile 0 computes slots the prologue requested and tile k's requests must not touch the slots it computes: nbuf >= 2 * span.
// What the wait of tile k leaves outstanding was requested in tile k itself, behind the tile's key load and queue draw: a
// counted wait that names those slots' pieces has passed both (vector-memory loads return in order).
// The kernel (hm_scan.hip) and tests/scan_span_driver.cpp run this code.
struct ScanRun {
    int ntile, nbuf, span;
    HM_HOST_DEVICE_INLINE constexpr int clamp(int s) const { return s < 0 ? 0 : (s > ntile ? ntile : s); }
    HM_HOST_DEVICE_INLINE constexpr int tiles() const { return (ntile + span - 1) / span; }
    HM_HOST_DEVICE_INLINE constexpr int prologue() const { return clamp(nbuf - span); }                  // slots requested before tile 0
    HM_HOST_DEVICE_INLINE constexpr int first(int k) const { return k * span; }                          // tile k computes [first, first + count)
    HM_HOST_DEVICE_INLINE constexpr int count(int k) const { return clamp((k + 1) * span) - clamp(k * span); }
    HM_HOST_DEVICE_INLINE constexpr int req_first(int k) const { return clamp(nbuf + (k - 1) * span); }  // tile k requests [req_first, req_first + req_count)
    HM_HOST_DEVICE_INLINE constexpr int req_count(int k) const { return clamp(nbuf + k * span) - req_first(k); }
    // slots still in flight behind the wait of tile k: everything requested so far but the slots of tile k + 1
    HM_HOST_DEVICE_INLINE constexpr int outstanding(int k) const { return clamp(nbuf + k * span) - clamp((k + 2) * span); }
    // the most that can be: what the counted waits are written out for
    HM_HOST_DEVICE_INLINE static constexpr int outstanding_max(int nbuf, int span) { return nbuf - 2 * span; }
};

// ---- what follows from a kernel's template arguments.  LDS map of a block (dynamic shared memory, from offset 0):
//   ring    NBUF slots of TILE_LDS bytes: the streamed partner tiles
//   slack   32 rows: the early request of "the next group's" first fragments behind the last group of the last slot lands
//           here and is never used.  HIST mode keeps its HM_HIST_BINS bins at the same offset (they are only read by that
//           request) and the slack's bytes behind them
//   queue   16 bytes: the item queue's broadcast word
// A ring cut for three blocks per CU (kScanRings::blocks = 3) has no slack: ring and queue word only.
template <int NG, int BF, int TM, int WPB, int SUB, int RING_ASK = 0, int SPAN_ASK = 1>
struct ScanGeom {
    static_assert(RING_ASK >= 0 && RING_ASK < HM_SCAN_RINGS && (RING_ASK == 0 || BF != 0), "rings other than 0: bf16 form");
    static constexpr int RS = hm_row_floats(NG);            // fp32 image: floats per row
    static constexpr int RB16 = 16 * hm_row16_chunks(NG);   // bf16 image: bytes per row (NG chunks of 8 bf16 [+ the [x0 fp32] chunk])
    static constexpr int ROW_BYTES = BF ? RB16 : RS * 4;
    static constexpr int QUEUE_BYTES = 16;
    // the ring of this instantiation: the one asked for, but ring 1 where a three-block ring was asked for with another span
    // than 2 or at a width whose blocks, each rounded up to the allocation granule, do not fit a CU's LDS three at a time
    static constexpr int ASK_BLOCKS = kScanRings[RING_ASK].blocks;
    static constexpr int ASK_LDS = (kScanRings[RING_ASK].dist + 1) * 32 * kScanRings[RING_ASK].sub * ROW_BYTES + QUEUE_BYTES;
    static constexpr int RING = (ASK_BLOCKS == 3 && !(SPAN_ASK == 2 && 3 * hm_lds_alloc(ASK_LDS) <= HM_LDS_PER_CU)) ? 1 : RING_ASK;
    static constexpr int BLOCKS = kScanRings[RING].blocks ? kScanRings[RING].blocks : 2;   // resident blocks per CU the LDS map is cut for
    static constexpr int RSUB = kScanRings[RING].sub ? kScanRings[RING].sub : SUB;   // 32-column groups per ring slot
    static constexpr bool EXACT = kScanRings[RING].exact != 0;
    static constexpr int PLAN_COLS = 32 * SUB;              // partner rows per tile of the item plan
    static constexpr int COLS = 32 * RSUB;                  // partner rows per streamed tile
    static_assert(SUB % RSUB == 0, "an item's run of plan tiles is a whole number of ring tiles");
    static constexpr int TILE_BYTES = COLS * ROW_BYTES;
    static constexpr int NP = BF ? (NG + 1) / 2 : NG + 1;   // k-steps: fp32: NG spatial groups + time; bf16: two chunks per step
    static constexpr int NPIECE = TILE_BYTES / 1024;        // 1 KiB pieces per tile
    static constexpr int PPW = (NPIECE + WPB - 1) / WPB;    // LDS-DMA pieces per wave and tile (slot padded to PPW * WPB KiB), at most
    // exact shares: wave w moves wave_pieces(w) pieces from piece wave_first(w) on (the first NPIECE % WPB waves one more)
    HM_HOST_DEVICE_INLINE static constexpr int wave_pieces(int w) { return EXACT ? NPIECE / WPB + (w < NPIECE % WPB ? 1 : 0) : PPW; }
    HM_HOST_DEVICE_INLINE static constexpr int wave_first(int w)
    {
        return EXACT ? w * (NPIECE / WPB) + (w < NPIECE % WPB ? w : NPIECE % WPB) : w * PPW;
    }
    static constexpr int TILE_LDS = EXACT ? TILE_BYTES : PPW * WPB * 1024;       // LDS bytes per ring slot
    // tiles in flight ahead of the one being computed.  A ring other than 0 asks for its depth and gets what fits the
    // block's half of a CU's LDS beside the slack and the queue word (wide rows: 17 chunks keep 3 in flight where 13 keep 4)
    static constexpr int SLOTS_MAX = (HM_LDS_PER_BLOCK - 32 * ROW_BYTES - 16) / TILE_LDS;
    // (a three-block ring exists only where its full depth fits: RING above)
    static constexpr int DIST = RING == 0 ? (BF ? HM_DIST_BF16 : 1)
                                          : (BLOCKS == 3 || kScanRings[RING].dist + 1 <= SLOTS_MAX ? kScanRings[RING].dist : (SLOTS_MAX > 2 ? SLOTS_MAX - 1 : 1));
    static constexpr int NBUF = DIST + 1;                   // ring slots
    // slots computed per barrier (ScanRun): what was asked for where the ring has the slots for it (16 chunks keep 3 padded
    // slots: span 1), and 1 on ring 0
    static_assert(SPAN_ASK == 1 || SPAN_ASK == 2, "the walks that are written out");
    static constexpr int SPAN = (RING != 0 && NBUF >= 2 * SPAN_ASK) ? SPAN_ASK : 1;
    static_assert(SPAN == 1 || NBUF >= 2 * SPAN, "a compute tile's slots and the next one's are in the ring together");
    static constexpr int WAVE_ROWS = 32 * TM;
    static constexpr int BLOCK_ROWS = WPB * WAVE_ROWS;
    static constexpr int NTHREADS = 64 * WPB;
    static_assert(TILE_BYTES % 1024 == 0, "tiles are moved in 1 KiB pieces");
    static_assert(DIST * PPW <= 60, "the counted wait must fit vmcnt");
    static_assert(SPAN == 1 || ScanRun::outstanding_max(NBUF, SPAN) <= DIST - SPAN, "a span's waits leave less in flight than span 1's");

    static constexpr int RING_BYTES = NBUF * TILE_LDS;
    static constexpr int SLACK_BYTES = BLOCKS == 3 ? 0 : 32 * ROW_BYTES;
    static constexpr int HIST_OFF = RING_BYTES;
    HM_HOST_DEVICE_INLINE static constexpr int queue_off(int mode)
    {
        return RING_BYTES + SLACK_BYTES + (mode == HM_MODE_HIST ? 4 * HM_HIST_BINS : 0);
    }
    HM_HOST_DEVICE_INLINE static constexpr int lds_bytes(int mode) { return queue_off(mode) + QUEUE_BYTES; }
    static_assert(BLOCKS != 3 || (EXACT && NBUF == 4 && SPAN == 2 && RING_BYTES + QUEUE_BYTES == 4 * TILE_BYTES + 16), "a three-block ring: four exact slots and the queue word");
    static_assert(BLOCKS != 3 || 3 * hm_lds_alloc(RING_BYTES + QUEUE_BYTES) <= HM_LDS_PER_CU, "three blocks, each rounded up to the allocation granule, fit a CU's LDS");
    static_assert(BLOCKS != 3 || ScanRun::outstanding_max(NBUF, SPAN) == 0, "a three-block ring: every tile wait is vmcnt(0)");
};
