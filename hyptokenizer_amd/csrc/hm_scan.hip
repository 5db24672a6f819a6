// hm_scan.hip -- the pair scan: X.G.X^T on the matrix cores as a PREFILTER for the exact search.
//
// Replaces the N x N distance matrix of the reference (batch_distance + triu + "< thr" + nonzero,
// tokenizer/hyperbolic_merge.py:247-269, fast_hyperbolic_merge.py:336-355); never materialises it.
//
// Shape.  Block = WPB waves; each wave keeps 32*TM *stationary* rows as MFMA A-fragments in registers for the
// whole block; the *partner* rows stream through LDS as tiles of 32*SUB rows, filled by LDS-DMA
// (global_load_lds_dwordx4, 1 KiB per wave-instruction) into a ring of slots.  Every wave issues the same
// number of pieces per tile, so "tile landed" is a counted s_waitcnt vmcnt(N) followed by one s_barrier per tile.
// A tile is walked as SUB groups of 32 columns.  Two accumulator sets alternate between groups: while the MFMAs
// of group g fill one set, the bound test of group g-1 (v_max3 tree, compare, ballot) runs on the other, in the
// same basic block -- the matrix pipe never drains for an epilogue, and the first LDS fragment of group g+1 is
// requested before the branch that ends group g.
//
// Two prefilter forms, one result (every reported distance is re-evaluated canonically, hm_search.hip):
//   BF = 0  v_mfma_f32_32x32x2_f32 on the fp32 image (exact fmaf chain; NG = groups of 4 spatial coordinates)
//   BF = 1  v_mfma_f32_32x32x16_bf16 on the bf16 image (NG = chunks of 8 K-slots, two per k-step; an odd count ends on
//           one v_mfma_f32_32x32x8_bf16_1k half step: d = 100 -> 13 chunks; time coordinate in split slots)
// A bound delta >= |u_f - u_c| (hm_scan_delta) widens every comparison.
#include <type_traits>

#include "hm_common.h"

#pragma clang fp contract(off)

// (HM_SUB_BF16, HM_SUB_F32, HM_DIST_BF16, HM_SCAN_INSTANTIATE_ALL, HM_SCAN_ALL_SHAPES: hm_scan_geom.h)

// CNT (1..4) consecutive 1 KiB LDS-DMA pieces in one statement: one M0 write; the immediate offset of
// global_load_lds applies to the global and to the LDS address alike, so the pieces share both bases.
template <int CNT>
__device__ __forceinline__ void hm_dma_group(const char* src, uint32_t dst)
{
    uint32_t keep;
    if constexpr (CNT == 4)
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\t"
                     "global_load_lds_dwordx4 %1, off offset:1024\n\tglobal_load_lds_dwordx4 %1, off offset:2048\n\t"
                     "global_load_lds_dwordx4 %1, off offset:3072\n\ts_mov_b32 m0, %0"
                     : "=&s"(keep) : "v"(src), "s"(dst) : "memory");
    else if constexpr (CNT == 3)
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\t"
                     "global_load_lds_dwordx4 %1, off offset:1024\n\tglobal_load_lds_dwordx4 %1, off offset:2048\n\t"
                     "s_mov_b32 m0, %0"
                     : "=&s"(keep) : "v"(src), "s"(dst) : "memory");
    else if constexpr (CNT == 2)
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\t"
                     "global_load_lds_dwordx4 %1, off offset:1024\n\ts_mov_b32 m0, %0"
                     : "=&s"(keep) : "v"(src), "s"(dst) : "memory");
    else
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                     : "=&s"(keep) : "v"(src), "s"(dst) : "memory");
}

// PIECES consecutive pieces starting at piece index FIRST, four per statement
template <int PIECES, int FIRST = 0>
__device__ __forceinline__ void hm_dma_run(const char* src, uint32_t dst)
{
    if constexpr (FIRST < PIECES) {
        hm_dma_group<(PIECES - FIRST < 4 ? PIECES - FIRST : 4)>(src + FIRST * 1024, dst + FIRST * 1024u);
        hm_dma_run<PIECES, FIRST + 4>(src, dst);
    }
}

#ifndef HM_SCAN_PIPE_MAX_TM
#define HM_SCAN_PIPE_MAX_TM 2
#endif
#ifndef HM_SCAN_DEEP_PREFETCH
#define HM_SCAN_DEEP_PREFETCH 1
#endif
// WK (ARGMIN mode only): the engine's running key is wide -- shift amounts from ScanArgs; narrow: (i << 15) | (j >> 2)
//
// HEAD > 0 (bf16 form, lorentz sign, ARGMIN, two accumulator sets): the head test.  A pair's u is x0 y0 - sum_k x_k y_k;
// with the spatial K-slots split into a head set H and the rest R (hm_head_steps / hm_rest_begin / hm_rest_end of
// hm_common.h), Cauchy-Schwarz gives  u >= x0 y0 - sum_{k in H} x_k y_k - r r',  r = ||x_R||.  Every image row carries
// r^ >= ||bf16(x)_R|| in its last K-slot (hm_rest_norm_bf16), which all other kernels multiply by a stationary 0.  Here the
// stationary side keeps +r^ there and only the HEAD k-steps of H in registers, the time step first: after HEAD k-steps the
// accumulators hold -(a lower bound of the group's u), which is reduced and compared with the bound of finish_group.
// When no lane is below it the group is done after HEAD of its NP k-steps; otherwise the group is recomputed by the
// complete chain (k-steps 0 .. NP-1 in order, stationary fragments re-read from the image, fourth slot 0: the operands
// and the order of the kernel without the test, hence its values bit for bit) and goes through finish_group as ever.
// Why the same delta (hm_scan_delta) is enough: let U_b be the exact value of the complete form on the bf16 operands and
// H_b that of the head form; H_b <= U_b by the inequality above, applied to the operands the matrix cores see (the time
// products are the same three terms in both; r^ r^' is exact in fp32; a flushed subnormal operand only shrinks a rest
// product, and r^ is never subnormal).  delta's bf16 part bounds |U_b - u_exact|.  Its fp32 part, (kterms + 8) ulps
// of rmax2, was sized for the roundings of a chain of kterms products whose absolute values sum to <= rmax2 plus those of the
// canonical value; the head chain has at most 16 * HEAD + 1 <= kterms - 7 products, and their absolute values sum to
// <= (1 + 2^-6) rmax2 (r^ exceeds ||x_R|| by at most two bf16 roundings): (kterms - 7) * 1.016 <= kterms for kterms <= 437.
// So head_f <= H_b + (that part) <= u_c + delta: a group whose lanes all have head_f >= bound holds no pair that the
// complete chain could have reported.  tests/test_scan_head_bound.py checks the inequality in numpy.
//
// RING > 0 (head kernels only; kScanRings of hm_scan_geom.h): a head kernel's wave is done with a 128-column tile in a
// fraction of the time the tile takes to land, so its ring keeps 64-column slots (RSUB = 2 groups: one pass of the head
// walk) and DIST = 3 or 4 of them in flight.  What changes with the depth: the item's run is counted in ring tiles; the
// counted waits leave (DIST - 1) tiles' pieces outstanding -- a wave's own number of pieces, which with exact shares
// depends on the (wave-uniform) wave index, so the waits branch on it and every immediate stays a constant; the
// asynchronous key load is picked up DIST - 1 tiles after it went out (vector-memory loads return in order: by then the
// wait of that tile has passed the tile requested right behind it); and the queue draw is picked up behind the run's
// closing vmcnt(0).
//
// SPAN = 2 (head kernels on rings 1 and 2; ScanRun of hm_scan_geom.h): two ring slots -- four groups, one pipeline -- between
// two barriers.  The slots keep their place in the ring and a failed group is still recomputed from the slot it sits in, in
// front of the barrier that frees it; what changes is the grain of everything paid per barrier: one request of two slots,
// one counted wait, one fresh group and one reduction outside the MFMAs' shadow per 128 columns, and for tiles right of
// the block's rows a straight-line body (head_tile_lean).  The key load of a tile is picked up behind that tile's own wait.
//
// RING = 3 (head kernels at span 2; kScanRings::blocks = 3): THREE blocks per CU, three waves per SIMD.  The LDS is the ring's
// four exact slots and the queue word -- no slack: the slot-by-slot walk takes its groups one at a time and requests no
// fragment behind a slot's last group -- and the kernel is built for at most 168 VGPRs.  Every tile's wait is a vmcnt(0) (ScanRun:
// nothing stays in flight behind it), so the two asynchronous results need no fixed registers: they are ordinary loads the
// compiler sees, issued ahead of the tile's requests, and in/out operands of the wait statement.  Whatever copy the compiler
// makes of them, it makes behind a wait of its own for the load, and that wait can only fall where the tile waits anyway.
template <int NG, int SIGN, int MODE, int BF, int TM, int WPB, int SUB, bool WK = false, int HEAD = 0, int RING = 0, int SPAN = 1>
__global__ __launch_bounds__(64 * WPB, (HEAD > 0 && kScanRings[RING].blocks == 3) ? 3 : 2) void hm_scan_kernel(const ScanArgs p)
{
    static_assert(SUB % 2 == 0, "the two accumulator sets alternate between column groups: an even number per tile");
    static_assert(RING == 0 || HEAD > 0, "rings other than 0 belong to the head kernels");
    constexpr bool PIPE = (TM <= HM_SCAN_PIPE_MAX_TM);   // two accumulator sets fit the registers (128 stationary rows per wave: one set)
    // the geometry of this instantiation (hm_scan_geom.h: sizes, ring, LDS map)
    using G = ScanGeom<NG, BF, TM, WPB, SUB, RING, SPAN>;
    static_assert(G::SPAN == SPAN, "a span the ring has no slots for is the dispatch's to replace (hm_launch_scan_ng)");
    static_assert(G::RING == RING, "a ring the width or the span has no room for is the dispatch's to replace (hm_launch_scan_ng)");
    constexpr bool TRI = (G::BLOCKS == 3);         // three blocks per CU: no slack behind the ring, no fixed registers
    static_assert(!TRI || (HEAD > 0 && SPAN == 2), "the three-block ring is the span-2 head kernels'");
    constexpr int COLS = G::COLS, RS = G::RS, RB16 = G::RB16, TILE_BYTES = G::TILE_BYTES, NP = G::NP;
    constexpr int PPW = G::PPW, TILE_LDS = G::TILE_LDS, DIST = G::DIST, NBUF = G::NBUF;
    constexpr int RSUB = G::RSUB;                  // 32-column groups per ring slot (SUB: per tile of the item plan)
    static_assert(RSUB % 2 == 0, "the head walk takes the groups of a slot in pairs");
    constexpr int WAVE_ROWS = G::WAVE_ROWS, BLOCK_ROWS = G::BLOCK_ROWS, NTHREADS = G::NTHREADS;
    constexpr bool HALF_LAST = (BF != 0) && (NG & 1);   // the last k-step covers one chunk only (8 K-slots)
    constexpr int TCH = RS / 4 - 1;                // fp32 image: chunk index of the time group
    static_assert(HEAD == 0 || (BF != 0 && SIGN != 0 && MODE == HM_MODE_ARGMIN && PIPE && HEAD == hm_head_steps(NG)),
                  "the head test: bf16 form, lorentz sign, argmin, two accumulator sets, the head set the image's r^ was built for");
    extern __shared__ __attribute__((aligned(16))) char smem[];   // G::lds_bytes(MODE)

    if (p.stop != nullptr && *p.stop != 0u) return;     // a device-resident loop has ended
    if (p.order_seen != nullptr && __hip_atomic_load(p.order_seen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < p.order_need) {
        if (threadIdx.x == 0) __hip_atomic_store(p.order_fault, 5u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;                                         // (pipelined loop: inputs not written yet -- see ScanArgs)
    }

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r = lane & 31, h = lane >> 5;

    uint32_t sure_total = 0;             // per-lane partial of the sure count
    unsigned long long gk = ~0ull;       // last value read of the running argmin key
    unsigned long long gk_raw = ~0ull;   // destination of the asynchronous key load
    bool gk_pending = false;
    const uint32_t lds_base = (uint32_t)(size_t)((__attribute__((address_space(3))) char*)smem);

    uint32_t* lhist = nullptr;
    if (MODE == HM_MODE_HIST) {
        lhist = reinterpret_cast<uint32_t*>(smem + G::HIST_OFF);
        for (int t = threadIdx.x; t < HM_HIST_BINS; t += NTHREADS) lhist[t] = 0;
    }

    // (row block, run of column tiles) being processed; the stationary rows in registers belong to row block rb_cur
    int rb = 0, ct0 = 0, ct1 = 0, rb_cur = -1;
    int i0w = 0;                        // first stationary row of this wave
    bool wave_active = false, rows_full = false;

    // The MFMA result u_f (plain fmaf chain) and the canonical u_c (torch reduction order) are two
    // roundings of the same exact form; |u_f - u_c| <= delta (gamma_n bound on both, |terms| <= rmax2).
    const float delta = hm_scan_delta(BF != 0, BF ? 8 * NG : RS, p.rmax2_bits);
    const float pre_f = p.u_hi + delta;              // candidate prefilter on u_f
    const float lo_f = p.u_lo - delta;               // u_f below this: canonical d < thr for sure
    const float zmax_f = 1.0f - delta;               // u_f at or below this: canonical u <= 1, d == 0
    const bool cut_all = (p.cut_bits == 0xffffffffu);
    const float cut_f = cut_all ? p.u_hi : hm::bitsf(p.cut_bits) + delta;
    static_assert(!WK || MODE == HM_MODE_ARGMIN, "only the argmin search keeps a running key");
    const int key_si = WK ? p.key_si : 32 - HM_KEY_IB_NARROW, key_sj = WK ? p.key_sj : 2 * HM_KEY_IB_NARROW - 32;

    // the running argmin key as it stands when the block starts (seeded, or found by earlier blocks)
    if (MODE == HM_MODE_ARGMIN) {
        const unsigned long long g0 = __hip_atomic_load(&p.ctr64[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (g0 < gk) gk = g0;
    }

    int hg_tot = 0, hc_tot = 0;          // head test: groups this wave ran / had to recompute (reported at the end, ScanArgs::head_bad)

    // ---- stationary A fragments: lane (r, h) keeps its operands of every k-step in registers ----
    float2 a[BF ? 1 : TM][BF ? 1 : NP];            // fp32 form: 2 operands (two k-steps) per group
    uint4 a16[BF ? TM : 1][BF ? NP : 1];           // bf16 form: 8 bf16 per 16-wide k-step
    uint4 a16t[HEAD ? TM : 1];                     // head test: the time k-step's fragment with +r^' in the fourth time slot
    // bf16 form: the k-step g operand of a lane from its row pointer (row start + 16 * h): 8 K-slots = one 16-byte chunk;
    // the half step of an odd chunk count holds 4 slots per lane (8 bytes at chunk start + 8 * h)
    auto frag_at = [&](const auto* base, int g) __attribute__((always_inline)) -> uint4 {
        const char* q = reinterpret_cast<const char*>(base);
        if (HALF_LAST && g == NP - 1) {
            const uint2 v = *reinterpret_cast<const uint2*>(q + 32 * g - 8 * h);
            return make_uint4(v.x, v.y, 0u, 0u);
        }
        return *reinterpret_cast<const uint4*>(q + 32 * g);
    };
    auto mfma16 = [&](const uint4& av, const uint4& bv, const f32x16& cv, int g) __attribute__((always_inline)) -> f32x16 {
        if (HALF_LAST && g == NP - 1) {
            typedef short s16x4 __attribute__((ext_vector_type(4)));
            const uint2 a2 = make_uint2(av.x, av.y), b2 = make_uint2(bv.x, bv.y);
            return __builtin_amdgcn_mfma_f32_32x32x8bf16_1k(__builtin_bit_cast(s16x4, a2), __builtin_bit_cast(s16x4, b2), cv, 0, 0, 0);
        }
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, av), __builtin_bit_cast(bf16x8, bv), cv, 0, 0, 0);
    };
    auto load_a = [&]() __attribute__((always_inline)) {
    if constexpr (BF) {
#pragma unroll
        for (int tm = 0; tm < TM; ++tm) {
            const unsigned char* src = p.img16 + (int64_t)(i0w + 32 * tm + r) * RB16 + 16 * h;
#pragma unroll
            for (int g = 0; g < NP; ++g) a16[tm][g] = frag_at(src, g);
            // stationary side of the time product: [hi, lo, hi, 0] -> [-hi, -hi, -lo, 0] (last 4 slots,
            // held by the h = 1 half of the last k-step)
            if (h == 1) {
                const uint32_t z = HALF_LAST ? a16[tm][NP - 1].x : a16[tm][NP - 1].z;
                const uint32_t hi16 = z & 0xffffu, lo16 = z >> 16;
                const uint32_t t0 = (hi16 | (hi16 << 16)) ^ 0x80008000u, t1 = lo16 ^ 0x8000u;
                if (HALF_LAST) { a16[tm][NP - 1].x = t0; a16[tm][NP - 1].y = t1; }
                else { a16[tm][NP - 1].z = t0; a16[tm][NP - 1].w = t1; }
            }
            if constexpr (HEAD > 0) {
                // head test: the same fragment with the row's rest norm in the fourth time slot, [-hi, -hi, -lo, +r^'],
                // r^' = max(r^, smallest normal): a zero r^ must not turn a huge r^ of the partner into 0
                uint32_t rh = (uint32_t)*reinterpret_cast<const unsigned short*>(p.img16 + (int64_t)(i0w + 32 * tm + r) * RB16 + 16 * NG - 2);
                rh = rh < 0x0080u ? 0x0080u : rh;
                a16t[tm] = a16[tm][NP - 1];
                if (h == 1) {
                    if (HALF_LAST) a16t[tm].y |= rh << 16;
                    else a16t[tm].w |= rh << 16;
                }
            }
        }
    } else {
#pragma unroll
        for (int tm = 0; tm < TM; ++tm) {
            const float* src = p.img + (int64_t)(i0w + 32 * tm + r) * RS + 2 * h;
#pragma unroll
            for (int g = 0; g < NP; ++g) a[tm][g] = *reinterpret_cast<const float2*>(src + 4 * (g < NG ? g : TCH));
            a[tm][NG].x = -a[tm][NG].x;            // time step: acc = S - x0*y0 = -M
        }
    }
    };

    // ---- LDS-DMA of one tile: wave w moves the PPW consecutive pieces [w * PPW, (w + 1) * PPW), four per
    // statement, through inline asm so that hipcc neither sees nor drains them; pieces past NPIECE (slot padding)
    // read the first KiB of the next tile: in bounds (the image is allocated with slack rows), unused.
    // Exact shares (G::EXACT): the slot is the tile, the first PREM waves move PQ + 1 pieces and the others PQ -- two code
    // sites chosen by the wave-uniform `wave`, so that each wave's piece count is a constant its counted waits can name.
    constexpr int PQ = G::NPIECE / WPB, PREM = G::EXACT ? G::NPIECE % WPB : 0;
    auto dma_tile = [&](int ct, int buf) __attribute__((always_inline)) {
        if constexpr (G::EXACT) {
            const int first = wave * PQ + (wave < PREM ? wave : PREM);
            const char* src = reinterpret_cast<const char*>(p.img16) + (int64_t)ct * TILE_BYTES + lane * 16 + first * 1024;
            const uint32_t dst = __builtin_amdgcn_readfirstlane(lds_base + (uint32_t)buf * (uint32_t)TILE_LDS + (uint32_t)first * 1024u);
            if (PREM != 0 && wave < PREM) hm_dma_run<PQ + 1>(src, dst);
            else hm_dma_run<PQ>(src, dst);
        } else {
        const char* src = (BF ? reinterpret_cast<const char*>(p.img16) : reinterpret_cast<const char*>(p.img)) +
                          (int64_t)ct * TILE_BYTES + lane * 16 + wave * (PPW * 1024);
        const uint32_t dst = __builtin_amdgcn_readfirstlane(lds_base + (uint32_t)buf * (uint32_t)TILE_LDS + (uint32_t)wave * (PPW * 1024u));
        hm_dma_run<PPW>(src, dst);
        }
    };

    // ---- per-group pieces ----
    f32x16 acc[PIPE ? 2 : 1][TM];                   // two accumulator sets (see the header) where they fit
    uint4 bpre16 = make_uint4(0, 0, 0, 0);          // first B fragment of the NEXT group, requested by the previous one
    // bf16 form with two accumulator sets: ALL k-step fragments of a column group are in registers before its MFMAs
    // start -- requested while the previous group of the tile computes (two register sets, alternating like the
    // accumulators).  With the fragments requested one k-step ahead, hipcc issued the LDS reads in pairs right
    // before their first use and the matrix pipe drained while they were in flight (ISA: ds_read x2, s_waitcnt,
    // 2 MFMA, s_waitcnt, 2 MFMA, ds_read x2, ...).
    constexpr bool DEEP = (BF != 0) && PIPE && (TM <= 2) && HM_SCAN_DEEP_PREFETCH;
    // (the one-set kernels -- 128-row waves -- have no registers left for a second fragment set: 60 spills when tried;
    // requesting all fragments of a group behind its first k-step measured 0.5 % slower than one-ahead requests there)
    static_assert(HEAD == 0 || DEEP, "the head walk keeps its fragments in bfr[][]: needs the two fragment register sets");
    uint4 bfr[2][DEEP ? NP : 1];
    float2 bpre = make_float2(0.f, 0.f);

    // all k-steps of column group `sub` of ring slot `buf` into acc[set].  `fresh`: the first fragment was not
    // requested by the previous group (first group of a tile, or the previous group was skipped).  The last k-step
    // always requests the first fragment of group sub + 1 (for the last group of a tile that lands in the slack
    // behind the slot and is never used).
    // `red_c` = true: the bound test's reduction over the OTHER accumulator set (the group finished before) is
    // folded into the k-steps, a few elements behind each step's MFMAs -- written into the same straight-line code
    // so that the vector ALU work rides in the matrix instructions' issue shadow; its result goes to `ext`.
    auto mma_group = [&](auto set_c, auto red_c, int buf, int sub, bool fresh, float& ext) __attribute__((always_inline)) {
        constexpr int set = decltype(set_c)::value;
        constexpr bool RED = decltype(red_c)::value;
        constexpr int QN = 16 * TM;
        if constexpr (RED) ext = acc[PIPE ? (set ^ 1) : 0][0][0];
        auto fold = [&](int g) {
            if constexpr (RED) {
#pragma unroll
                for (int q = (g * QN) / NP; q < ((g + 1) * QN) / NP; ++q) {
                    const float v = acc[PIPE ? (set ^ 1) : 0][q / 16][q % 16];
                    ext = SIGN ? __builtin_fmaxf(ext, v) : __builtin_fminf(ext, v);
                }
            }
        };
        if constexpr (BF) {
            const char* bt = smem + buf * TILE_LDS + (sub * 32 + r) * RB16 + 16 * h;
            if (fresh) bpre16 = frag_at(bt, 0);
            uint4 bc = bpre16, bn = bc;
#pragma unroll
            for (int g = 0; g < NP; ++g) {
                bn = g + 1 < NP ? frag_at(bt, g + 1) : frag_at(bt + 32 * RB16, 0);
#pragma unroll
                for (int tm = 0; tm < TM; ++tm) {
                    if (g == 0) {
                        f32x16 z;
#pragma unroll
                        for (int e = 0; e < 16; ++e) z[e] = 0.0f;
                        acc[set][tm] = mfma16(a16[tm][g], bc, z, g);
                    } else {
                        acc[set][tm] = mfma16(a16[tm][g], bc, acc[set][tm], g);
                    }
                }
                fold(g);
                bc = bn;
            }
            bpre16 = bn;
            // acc = S - x0*y0 (= -M): the time product came out of the last k-step's split slots
        } else {
            const float* bt = reinterpret_cast<const float*>(smem + buf * TILE_LDS) + (sub * 32 + r) * RS + 2 * h;
            if (fresh) bpre = *reinterpret_cast<const float2*>(bt);
            float2 bc = bpre, bn = bc;
#pragma unroll
            for (int g = 0; g < NP; ++g) {
                bn = *reinterpret_cast<const float2*>(bt + (g + 1 < NP ? 4 * (g + 1 < NG ? g + 1 : TCH) : 32 * RS));
#pragma unroll
                for (int tm = 0; tm < TM; ++tm) {
                    if (g == 0) {
                        f32x16 z;
#pragma unroll
                        for (int e = 0; e < 16; ++e) z[e] = 0.0f;
                        acc[set][tm] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[tm][g].x, bc.x, z, 0, 0, 0);
                    } else {
                        acc[set][tm] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[tm][g].x, bc.x, acc[set][tm], 0, 0, 0);
                    }
                }
                if (g < NG) {
#pragma unroll
                    for (int tm = 0; tm < TM; ++tm)
                        acc[set][tm] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[tm][g].y, bc.y, acc[set][tm], 0, 0, 0);
                }
                fold(g);
                bc = bn;
            }
            bpre = bn;
        }
        if constexpr (RED) ext = SIGN ? -ext : ext;
    };

    // The hot form of the bf16 kernel (both groups of a pass run and a finished group is pending): all k-step fragments
    // of the group are in bfr[set] before its MFMAs start -- requested by the previous group (`fresh` = false) -- and
    // the next group's go out to bfr[set ^ 1] behind the first k-step, always, so the LDS latency is paid behind fourteen
    // MFMAs instead of in front of every second pair.  The other set's bound-test reduction rides along as in mma_group.
    auto mma_group_deep = [&](auto set_c, int buf, int sub, bool fresh, float& ext) __attribute__((always_inline)) {
        constexpr int set = decltype(set_c)::value;
        constexpr int QN = 16 * TM;
        if constexpr (DEEP) {
            const char* bt = smem + buf * TILE_LDS + (sub * 32 + r) * RB16 + 16 * h;
            if (fresh) {
#pragma unroll
                for (int g = 0; g < NP; ++g) bfr[set][g] = frag_at(bt, g);
            }
            ext = acc[set ^ 1][0][0];
            auto kstep = [&](int g) {
#pragma unroll
                for (int tm = 0; tm < TM; ++tm) {
                    if (g == 0) {
                        f32x16 z;
#pragma unroll
                        for (int e = 0; e < 16; ++e) z[e] = 0.0f;
                        acc[set][tm] = mfma16(a16[tm][g], bfr[set][g], z, g);
                    } else {
                        acc[set][tm] = mfma16(a16[tm][g], bfr[set][g], acc[set][tm], g);
                    }
                }
#pragma unroll
                for (int q = (g * QN) / NP; q < ((g + 1) * QN) / NP; ++q) {
                    const float v = acc[set ^ 1][q / 16][q % 16];
                    ext = SIGN ? __builtin_fmaxf(ext, v) : __builtin_fminf(ext, v);
                }
            };
            // the first k-step goes out before the next group's requests: LDS data returns in order, and a wait placed
            // behind fresh requests would hold the first MFMA until the first of THEM is back
            kstep(0);
            __builtin_amdgcn_sched_barrier(0);
            // unconditional (behind the last group of a tile the addresses fall into the next slot or the slack behind
            // the ring and the data is never used): a branch here makes hipcc count the waits of the MFMAs below for
            // the path WITHOUT the requests, which in the path with them means waiting for the requests themselves
#pragma unroll
            for (int g = 0; g < NP; ++g) bfr[set ^ 1][g] = frag_at(bt + 32 * RB16, g);
            __builtin_amdgcn_sched_barrier(0);      // the requests stay in front of the remaining MFMAs
#pragma unroll
            for (int g = 1; g < NP; ++g) kstep(g);
            ext = SIGN ? -ext : ext;
        }
    };

    // the lane's most promising u of accumulator set `set` (acc = -M: u = acc under the reference sign, -acc under lorentz)
    auto reduce_group = [&](auto set_c) __attribute__((always_inline)) -> float {
        constexpr int set = decltype(set_c)::value;
        float ext = acc[set][0][0];
#pragma unroll
        for (int tm = 0; tm < TM; ++tm)
#pragma unroll
            for (int e = 0; e < 16; ++e) ext = SIGN ? __builtin_fmaxf(ext, acc[set][tm][e]) : __builtin_fminf(ext, acc[set][tm][e]);
        return SIGN ? -ext : ext;
    };

    // bound test of a finished group and, when some lane is below the bound, the slow path: one 32x32 MFMA tile at
    // a time (a rolled loop: the hot loop must not inherit its register pressure).  Per-element predicates are
    // evaluated twice (count, then write); the second evaluation runs on laundered copies of the bounds so that the
    // compiler does not keep the predicates alive across the wave scan.
    auto finish_group = [&](auto set_c, float ext_u, int j0s) __attribute__((always_inline)) {
        constexpr int set = decltype(set_c)::value;
        float bound_f = pre_f;
        uint32_t best_bits = 0xffffffffu, best_low = 0xffffffffu;
        if (MODE == HM_MODE_TOPK && !p.count_sure && !cut_all && cut_f < bound_f) bound_f = cut_f;   // nothing above the cut is visited
        if (MODE == HM_MODE_ARGMIN) {
            // an entry can only order before the running best if its u_f is within 2*delta (+ a few ulps of acosh
            // wiggle) of the best u_f
            best_bits = (uint32_t)(gk >> 32);
            best_low = (uint32_t)gk;
            if (best_bits != 0xffffffffu) {
                const float bb = hm::bitsf(best_bits + hm_tie_slack(best_bits)) + 2.0f * delta;
                if (bb < bound_f) bound_f = bb;
            }
        }
        if (__ballot(ext_u < bound_f) == 0ull) return;
        if (MODE == HM_MODE_ARGMIN && best_bits == 0x3f7fffffu && p.thr_pos != 0) {
            // The running best is a pair at distance exactly 0 (the literal sign mode: EVERY pair is one).  A pair that is
            // certainly at distance 0 too is only emitted when its (i, j) orders before the best's (`low <= best_low`
            // below); every pair of this group has low >= lowmin.  So when the whole group is certainly-zero and starts
            // behind the best pair, the slow path would emit nothing: skip it (1.6 ms -> 0.3 ms per tie-flood scan).
            const uint32_t lowmin = hm_key_low((uint32_t)i0w, (uint32_t)j0s, key_si, key_sj);
            if (lowmin > best_low) {
                float worst = SIGN ? -acc[set][0][0] : acc[set][0][0];          // the LARGEST u of the lane's elements
#pragma unroll
                for (int tm = 0; tm < TM; ++tm)
#pragma unroll
                    for (int e = 0; e < 16; ++e) {
                        const float u = SIGN ? -acc[set][tm][e] : acc[set][tm][e];
                        worst = __builtin_fmaxf(worst, u);
                    }
                if (__ballot(!(worst <= zmax_f)) == 0ull) return;                // (NaN counts as not certainly zero)
            }
        }
        const bool full = rows_full && (j0s > i0w + WAVE_ROWS - 1) && (j0s + 31 < p.n) && (j0s >= p.col_begin);
        unsigned long long wkey = ~0ull;
        bool wrote = false;
#pragma unroll 1
        for (int st = 0; st < TM; ++st) {
            // element-wise select chain: a whole-vector `if (st == q) w = acc[q]` makes hipcc keep the accumulators
            // in scratch memory in some instantiations (3x slower hot loop)
            f32x16 w;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                float v = acc[set][0][e];
#pragma unroll
                for (int q = 1; q < TM; ++q) v = (st == q) ? acc[set][q][e] : v;
                w[e] = v;
            }
            if (TM > 1) {
                float e1 = w[0];
#pragma unroll
                for (int e = 1; e < 16; ++e) e1 = SIGN ? __builtin_fmaxf(e1, w[e]) : __builtin_fminf(e1, w[e]);
                if (__ballot((SIGN ? -e1 : e1) < bound_f) == 0ull) continue;
            }
            uint32_t n_emit = 0, n_sure = 0;
            float bnd = bound_f;
            float cutv = cut_f;
            unsigned long long slot = 0;
            const int ib = i0w + 32 * st + 4 * h;
            const int j = j0s + r;
            auto visit = [&](const float wv, const int e, const bool write) {
                const float u = SIGN ? -wv : wv;
                const int i = ib + (e & 3) + 8 * (e >> 2);
                bool pass = u < bnd;
                if (!full) pass = pass && (i < j) && (j < p.n) && (j >= p.col_begin) && (i >= p.row_begin) && (i < p.row_end);
                if (!pass) return;
                const float up = u < 1.0f ? 1.0f : u;
                const uint32_t ub = hm::fbits(up);
                if (MODE == HM_MODE_HIST) {
                    if (ub >= p.hist_lo) {
                        uint32_t bin = (ub - p.hist_lo) >> p.hist_shift;
                        if (bin > HM_HIST_BINS - 1) bin = HM_HIST_BINS - 1;
                        atomicAdd(&lhist[bin], 1u);
                    }
                    return;
                }
                bool emit;
                uint32_t flag = 0;
                const bool zero = (u <= zmax_f) && (p.thr_pos != 0);     // certainly d == 0 < thr
                if (MODE == HM_MODE_TOPK) {
                    const bool sure = zero || (up < lo_f);
                    if (sure && !write) ++n_sure;
                    flag = sure ? 1u : 0u;
                    // zero-distance ties order by (i, j): a tie flood is cut by rows (tie_imax)
                    emit = zero ? (i <= p.tie_imax) : ((!sure && p.count_sure) || cut_all || up <= cutv);
                } else {
                    const uint32_t ubz = zero ? 0x3f7fffffu : ub;
                    const uint32_t low = hm_key_low((uint32_t)i, (uint32_t)j, key_si, key_sj);
                    emit = !(zero && best_bits == 0x3f7fffffu) || (low <= best_low);
                    if (emit && !write) {
                        const unsigned long long k = ((unsigned long long)ubz << 32) | low;
                        wkey = k < wkey ? k : wkey;
                    }
                }
                if (!emit) return;
                if (!write) { ++n_emit; return; }
                if (slot < (unsigned long long)p.ent_cap) p.ent[slot] = make_uint4(ub, (uint32_t)i, (uint32_t)j, flag);
                ++slot;
            };
#pragma unroll
            for (int e = 0; e < 16; ++e) visit(w[e], e, false);
            if (MODE == HM_MODE_HIST) continue;
            sure_total += n_sure;
            const uint32_t incl = hm_wave_incl_scan(n_emit, lane);
            const uint32_t total = __shfl(incl, 63, 64);
            if (total == 0) continue;
            unsigned long long base = 0;
            if (lane == 63) base = atomicAdd(&p.ctr64[2], (unsigned long long)total);     // 64-bit: a tie flood cannot wrap it
            base = __shfl(base, 63, 64);
            slot = base + incl - n_emit;
            asm volatile("" : "+v"(bnd), "+v"(cutv));      // opaque: no CSE with the count pass
#pragma unroll
            for (int e = 0; e < 16; ++e) visit(w[e], e, true);
            wrote = true;
        }
        if (MODE == HM_MODE_ARGMIN && wrote) {
            const unsigned long long wk = hm_wave_min_u64(wkey);
            if (lane == 0) atomicMin(&p.ctr64[1], wk);
            // the slow path has drained the vector-memory queue anyway: refresh the running key now
            gk = __hip_atomic_load(&p.ctr64[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (wk < gk) gk = wk;
        }
    };

    // ---- the head test (HEAD > 0; see the kernel's header) ----
    // the HEAD k-steps of column group `sub` into acc[set], software-pipelined like mma_group_deep: the fragments are in
    // bfr[set] before the MFMAs start (requested by the previous group unless `fresh`), the next group's go out to
    // bfr[set ^ 1] behind the first k-step, and with RED the reduction of the other set -- the head values of the group
    // before -- rides in the issue shadow of the MFMAs; its result goes to `ext`
    // `bt`: the lane's row of the group in its ring slot (head_at); `btn`: of the group whose fragments go out (NEXT)
    auto head_at = [&](int buf, int sub) __attribute__((always_inline)) -> const char* { return smem + buf * TILE_LDS + (sub * 32 + r) * RB16 + 16 * h; };
    auto head_group = [&](auto set_c, auto red_c, auto next_c, const char* bt, const char* btn, bool fresh, float& ext) __attribute__((always_inline)) {
        constexpr int set = decltype(set_c)::value;
        constexpr bool RED = decltype(red_c)::value, NEXT = decltype(next_c)::value;
        constexpr int QN = 16 * TM;
        if constexpr (HEAD > 0) {
            if (fresh) {
#pragma unroll
                for (int k = 0; k < HEAD; ++k) bfr[set][k] = frag_at(bt, hm_head_kstep(k, NP));
            }
            if constexpr (RED) ext = acc[set ^ 1][0][0];
            auto kstep = [&](auto k_c) {                 // (k as a type: every register array index below is a constant)
                constexpr int k = decltype(k_c)::value;
                constexpr int g = hm_head_kstep(k, NP);
#pragma unroll
                for (int tm = 0; tm < TM; ++tm) {
                    if constexpr (k == 0) {
                        f32x16 z;
#pragma unroll
                        for (int e = 0; e < 16; ++e) z[e] = 0.0f;
                        acc[set][tm] = mfma16(a16t[tm], bfr[set][k], z, g);
                    } else {
                        acc[set][tm] = mfma16(a16[tm][g], bfr[set][k], acc[set][tm], g);
                    }
                }
                if constexpr (RED) {
#pragma unroll
                    for (int q = (k * QN) / HEAD; q < ((k + 1) * QN) / HEAD; ++q)
                        ext = __builtin_fmaxf(ext, acc[set ^ 1][q / 16][q % 16]);
                }
            };
            kstep(std::integral_constant<int, 0>{});
            __builtin_amdgcn_sched_barrier(0);
            // no run-time condition, like mma_group_deep's: behind the last group of a slot of the span-1 walk the addresses
            // fall into the next slot or the slack behind the ring and the data is never used
            if constexpr (NEXT) {
#pragma unroll
                for (int k = 0; k < HEAD; ++k) bfr[set ^ 1][k] = frag_at(btn, hm_head_kstep(k, NP));
            }
            __builtin_amdgcn_sched_barrier(0);
            static_assert(HEAD <= 4, "the head k-steps are written out");
            if constexpr (HEAD > 1) kstep(std::integral_constant<int, 1>{});
            if constexpr (HEAD > 2) kstep(std::integral_constant<int, 2>{});
            if constexpr (HEAD > 3) kstep(std::integral_constant<int, 3>{});
            if constexpr (RED) ext = -ext;
        }
    };
    // bound test of a group's head values (`ext_u`: the smallest lower bound of u among the lane's elements of acc[set]); a
    // group that fails it is recomputed by the complete chain -- a rolled loop that reads the stationary fragments from
    // the image again (L2), so the hot loop inherits no registers from it -- and handed to finish_group.  The group's
    // columns must still be in ring slot `buf`: the head walk tests the last group of a tile before the tile's barrier.
    auto head_finish = [&](auto set_c, float ext_u, int buf, int sub, int j0s) __attribute__((always_inline)) -> bool {
        constexpr int set = decltype(set_c)::value;
        if constexpr (HEAD > 0) {
            float bound_f = pre_f;                       // (the ARGMIN bound of finish_group)
            const uint32_t best_bits = (uint32_t)(gk >> 32);
            if (best_bits != 0xffffffffu) {
                const float bb = hm::bitsf(best_bits + hm_tie_slack(best_bits)) + 2.0f * delta;
                if (bb < bound_f) bound_f = bb;
            }
            if (__ballot(ext_u < bound_f) == 0ull) return false;
            const char* bt = smem + buf * TILE_LDS + (sub * 32 + r) * RB16 + 16 * h;
            const unsigned char* as = p.img16 + (int64_t)(i0w + r) * RB16 + 16 * h;
#pragma unroll
            for (int tm = 0; tm < TM; ++tm)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[set][tm][e] = 0.0f;
#pragma unroll 1
            for (int g = 0; g < NP - 1; ++g) {
                const uint4 bv = *reinterpret_cast<const uint4*>(bt + 32 * g);
#pragma unroll
                for (int tm = 0; tm < TM; ++tm) {
                    const uint4 av = *reinterpret_cast<const uint4*>(as + (int64_t)(32 * tm) * RB16 + 32 * g);
                    acc[set][tm] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, av), __builtin_bit_cast(bf16x8, bv), acc[set][tm], 0, 0, 0);
                }
            }
            {
                const uint4 bv = frag_at(bt, NP - 1);
#pragma unroll
                for (int tm = 0; tm < TM; ++tm) {
                    uint4 av = frag_at(as + (int64_t)(32 * tm) * RB16, NP - 1);
                    if (h == 1) {                        // [hi, lo, hi, r^] -> [-hi, -hi, -lo, 0], as load_a of the kernels without the test
                        const uint32_t z = HALF_LAST ? av.x : av.z;
                        const uint32_t hi16 = z & 0xffffu, lo16 = z >> 16;
                        const uint32_t t0 = (hi16 | (hi16 << 16)) ^ 0x80008000u, t1 = lo16 ^ 0x8000u;
                        if (HALF_LAST) { av.x = t0; av.y = t1; }
                        else { av.z = t0; av.w = t1; }
                    }
                    acc[set][tm] = mfma16(av, bv, acc[set][tm], NP - 1);
                }
            }
            finish_group(set_c, reduce_group(set_c), j0s);
            return true;
        }
        return false;
    };

    // RING > 0: the counted wait that leaves the pieces of at most `tiles` (wave-uniform; WMAX at most count) of this wave's
    // ring slots outstanding; a key load or a queue draw among the outstanding only makes the count stricter
    constexpr int WMAX = ScanRun::outstanding_max(NBUF, SPAN);
    auto ring_wait = [&](int tiles) __attribute__((always_inline)) {
        auto wait_p = [&](auto p_c) __attribute__((always_inline)) {
            constexpr int P = decltype(p_c)::value;
            static_assert(WMAX * P <= 60, "the counted wait must fit vmcnt");
            if (tiles >= 3 && WMAX >= 3) asm volatile("s_waitcnt vmcnt(%0)" : : "n"(3 * P) : "memory");
            else if (tiles >= 2 && WMAX >= 2) asm volatile("s_waitcnt vmcnt(%0)" : : "n"(2 * P) : "memory");
            else if (tiles >= 1 && WMAX >= 1) asm volatile("s_waitcnt vmcnt(%0)" : : "n"(P) : "memory");
            else asm volatile("s_waitcnt vmcnt(0)" : : : "memory");
        };
        static_assert(RING == 0 || WMAX <= 3, "ring_wait writes out the depths");
        if constexpr (PREM != 0) {
            if (wave < PREM) wait_p(std::integral_constant<int, PQ + 1>{});
            else wait_p(std::integral_constant<int, PQ>{});
        } else {
            wait_p(std::integral_constant<int, G::EXACT ? PQ : PPW>{});
        }
    };

    // head walk of the ring slot `buf` (columns from j0 on): its groups alternate between the accumulator sets; group g's
    // head k-steps carry the reduction of group g - 1's head values, whose test follows.  Nothing is pending behind the slot
    // (the recomputation of a failed group reads its columns from the slot): the last group is reduced on its own.
    auto head_walk = [&](int buf, int j0) __attribute__((always_inline)) {
        if constexpr (TRI) {
            // three blocks per CU: the slot's groups one by one in one accumulator set, each fresh, reduced and tested before
            // the next starts.  These are the diagonal tiles, the waves without rows and a run's odd end -- a hundredth of the
            // tiles at 50 000 rows --, and this way no finished group waits in the other set while a failed one is recomputed
            // (32 accumulator and 12 fragment registers fewer at the kernel's widest point), and no fragment is requested
            // behind a slot's last group: the ring has no slack for such a request to land in
#pragma unroll 1
            for (int sub = 0; sub < RSUB; ++sub) {
                const int j0s = j0 + sub * 32;
                if (!(wave_active && (j0s + 31 > i0w))) continue;
                const char* bt = head_at(buf, sub);
                float ext_u = 0.0f;
                head_group(std::integral_constant<int, 0>{}, std::false_type{}, std::false_type{}, bt, bt, true, ext_u);
                ext_u = reduce_group(std::integral_constant<int, 0>{});
                ++hg_tot;
                hc_tot += head_finish(std::integral_constant<int, 0>{}, ext_u, buf, sub, j0s) ? 1 : 0;
            }
        } else if constexpr (HEAD > 0) {
            bool hp = false;
            int hg = 0, hc = 0;          // groups of this slot that ran / that had to be recomputed
#pragma unroll 1
            for (int sp = 0; sp < RSUB / 2; ++sp) {
                {
                    const int sub = 2 * sp;
                    const int j0s = j0 + sub * 32;
                    const bool do_c = wave_active && (j0s + 31 > i0w);
                    const char* bt = head_at(buf, sub);
                    float ext_u = 0.0f;
                    if (do_c && hp) {
                        head_group(std::integral_constant<int, 0>{}, std::true_type{}, std::true_type{}, bt, bt + 32 * RB16, false, ext_u);
                    } else {
                        if (do_c) head_group(std::integral_constant<int, 0>{}, std::false_type{}, std::true_type{}, bt, bt + 32 * RB16, true, ext_u);
                        if (hp) ext_u = reduce_group(std::integral_constant<int, 1>{});
                    }
                    if (hp) { ++hg; hc += head_finish(std::integral_constant<int, 1>{}, ext_u, buf, sub - 1, j0s - 32) ? 1 : 0; }
                    hp = do_c;
                }
                {
                    const int sub = 2 * sp + 1;
                    const int j0s = j0 + sub * 32;
                    const bool do_c = wave_active && (j0s + 31 > i0w);
                    const char* bt = head_at(buf, sub);
                    float ext_u = 0.0f;
                    if (do_c && hp) {
                        head_group(std::integral_constant<int, 1>{}, std::true_type{}, std::true_type{}, bt, bt + 32 * RB16, false, ext_u);
                    } else {
                        if (do_c) head_group(std::integral_constant<int, 1>{}, std::false_type{}, std::true_type{}, bt, bt + 32 * RB16, true, ext_u);
                        if (hp) ext_u = reduce_group(std::integral_constant<int, 0>{});
                    }
                    if (hp) { ++hg; hc += head_finish(std::integral_constant<int, 0>{}, ext_u, buf, sub - 1, j0s - 32) ? 1 : 0; }
                    hp = do_c;
                }
            }
            if (hp) { ++hg; hc += head_finish(std::integral_constant<int, 1>{}, reduce_group(std::integral_constant<int, 1>{}), buf, RSUB - 1, j0 + (RSUB - 1) * 32) ? 1 : 0; }
            hg_tot += hg; hc_tot += hc;
        }
    };

    // the interior tile of the span-2 walk (SPAN = 2): the four groups of the two slots `buf0`, `buf1` (columns from j0 on,
    // all of them right of the block's rows, on an active wave) as one pipeline in straight-line code -- no predicate per
    // group, one fresh group, one reduction outside the MFMAs' shadow, no fragment request behind the last group.  The bound
    // is built once from the key as it stands (a stale bound is only looser: the key never increases) and the four head
    // values are tested against it with one ballot.  A tile in which some group fails goes through the rolled loop behind:
    // both accumulator sets are free by then, the failed groups are recomputed from the slots they sit in -- in front of the
    // barrier that frees those -- and head_finish rebuilds the bound from the key a finish_group may have refreshed.
    auto head_tile_lean = [&](int buf0, int buf1, int j0) __attribute__((always_inline)) {
        if constexpr (HEAD > 0 && SPAN == 2) {
            static_assert(RSUB == 2, "two slots of two groups");
            float bound_f = pre_f;
            const uint32_t best_bits = (uint32_t)(gk >> 32);
            if (best_bits != 0xffffffffu) {
                const float bb = hm::bitsf(best_bits + hm_tie_slack(best_bits)) + 2.0f * delta;
                if (bb < bound_f) bound_f = bb;
            }
            const char* b0 = head_at(buf0, 0);
            const char* b1 = head_at(buf1, 0);
            float e0 = 0.0f, e1 = 0.0f, e2 = 0.0f;
            head_group(std::integral_constant<int, 0>{}, std::false_type{}, std::true_type{}, b0, b0 + 32 * RB16, true, e0);
            head_group(std::integral_constant<int, 1>{}, std::true_type{}, std::true_type{}, b0 + 32 * RB16, b1, false, e0);
            head_group(std::integral_constant<int, 0>{}, std::true_type{}, std::true_type{}, b1, b1 + 32 * RB16, false, e1);
            head_group(std::integral_constant<int, 1>{}, std::true_type{}, std::false_type{}, b1 + 32 * RB16, b1, false, e2);
            const float e3 = reduce_group(std::integral_constant<int, 1>{});
            hg_tot += 2 * RSUB;
            if (__ballot(__builtin_fminf(__builtin_fminf(e0, e1), __builtin_fminf(e2, e3)) < bound_f) != 0ull) {
#pragma unroll 1
                for (int g = 0; g < 2 * RSUB; ++g) {
                    const float eg = g == 0 ? e0 : (g == 1 ? e1 : (g == 2 ? e2 : e3));
                    hc_tot += head_finish(std::integral_constant<int, 0>{}, eg, g < RSUB ? buf0 : buf1, g % RSUB, j0 + 32 * g) ? 1 : 0;
                }
            }
        }
    };

    // ---- work distribution: block b owns item b of the host's list (hm_scan_plan.h); with the item queue (p.dyn) the grid
    // is the resident set and every block goes on drawing items of the same list, in order, from the queue word p.q_ctr ----
    volatile uint32_t* const qslot = reinterpret_cast<volatile uint32_t*>(smem + G::queue_off(MODE));      // the drawn counter value, for all waves
    const bool dyn = (MODE != HM_MODE_HIST) && (p.dyn != 0);
    unsigned long long q_raw = 0ull;     // destination of the asynchronous draw (thread 0)
    if (dyn && threadIdx.x == 0) (void)__hip_atomic_fetch_max(p.q_ctr, p.q_tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    int item = (int)blockIdx.x;
#pragma unroll 1
    for (;;) {
    bool have = true;                   // the item has tiles right of the diagonal
    HM_SCAN_ITEM_DECODE(p.items, item, BLOCK_ROWS, G::PLAN_COLS, p.nct, p.col_begin, rb, ct0, ct1)
    if constexpr (COLS != G::PLAN_COLS) {
        // the run in ring tiles: the plan's tiles are whole numbers of them; the clamps again at the finer grain
        ct0 *= G::PLAN_COLS / COLS;
        ct1 *= G::PLAN_COLS / COLS;
        if (ct0 < p.col_begin / COLS) ct0 = p.col_begin / COLS;
        if (ct1 > (p.n + COLS - 1) / COLS) ct1 = (p.n + COLS - 1) / COLS;
    }
    if (ct0 >= ct1) have = false;

    // HIST mode visits every sample_stride-th tile only (a cheap estimate of the u' distribution)
    int ct_step = 1;
    if (MODE == HM_MODE_HIST && have) {
        ct_step = p.sample_stride;
        ct0 += (ct_step - (ct0 + rb * 7) % ct_step) % ct_step;
        if (ct0 >= ct1) have = false;
    }
    if (have) {
    if (rb != rb_cur) {
        rb_cur = rb;
        i0w = rb * BLOCK_ROWS + wave * WAVE_ROWS;
        wave_active = (i0w < p.row_end) && (i0w + WAVE_ROWS - 1 >= p.row_begin) && (i0w < p.n);
        rows_full = (i0w >= p.row_begin) && (i0w + WAVE_ROWS - 1 < p.row_end);
        load_a();
    }
    const int ntile = (ct1 - ct0 + ct_step - 1) / ct_step;
    auto tile_at = [&](int t) { return ct0 + t * ct_step; };

    // ring prologue: tiles 0 .. DIST-1 in flight (a repeat of the last tile when the run is shorter), tile 0 landed
    if constexpr (RING > 0) {
        // the tiles the run has, no repeats (the loop below requests none either); everything lands before the loop is
        // entered -- the wait hipcc can see (below) would drain the prologue's tiles anyway, once per item
#pragma unroll
        for (int q = 0; q < NBUF - SPAN; ++q)              // (ScanRun::prologue: DIST slots ahead of span 1, one fewer of span 2)
            if (q < ntile) dma_tile(tile_at(q), q);
        __builtin_amdgcn_s_waitcnt(0x0F70);
    } else {
#pragma unroll
    for (int q = 0; q < DIST; ++q) dma_tile(tile_at(q < ntile ? q : ntile - 1), q);
    if (DIST - 1 <= 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(%0)" ::"n"((DIST - 1) * PPW) : "memory");
    // hipcc waits for its own loads (the A fragments above) lazily, at their first use INSIDE the loop -- with
    // vmcnt(N) instructions that also wait for the ring's LDS-DMA (which it cannot see) on every iteration.
    // A wait it can see, here, settles them before the loop is entered.
    if (DIST == 1) __builtin_amdgcn_s_waitcnt(0x0F70);      // vmcnt(0), expcnt / lgkmcnt untouched (gfx9 encoding)
    }
    __syncthreads();

    bool pend = false;               // a finished group waits in the other accumulator set for its bound test
    bool deep_valid = false;         // bfr[0] holds the fragments of the group about to run (requested by its predecessor)
    int pend_j0s = 0;
    int buf = 0;                     // ring slot of tile t
    int gk_due = 0;                  // RING > 0: the tile behind whose wait the key load in flight is complete

    if constexpr (SPAN == 2) {
        // the span-2 walk (ScanRun of hm_scan_geom.h): two ring slots per barrier.  Tile k computes the slots 2k and 2k + 1
        // of the run (an odd run ends on a tile of one), which sit in the ring slots buf and buf + 1; the slots it requests
        // go to the two ring slots behind those of tile k + 1, the ones tile k - 1 computed.
        static_assert(HEAD > 0 && RING > 0 && MODE == HM_MODE_ARGMIN, "the span-2 walk is the head kernels'");
        const ScanRun run{ntile, NBUF, SPAN};
        const int ntk = run.tiles();
        const int j_right = rb * BLOCK_ROWS + BLOCK_ROWS;      // columns from here on lie right of every row of the block
        auto ring_add = [&](int b, int q) { b += q; return b >= NBUF ? b - NBUF : b; };
#pragma unroll 1
        for (int k = 0; k < ntk; ++k) {
            const int nslot = run.count(k);
            const int j0 = (ct0 + 2 * k) * COLS;
            const int buf1 = ring_add(buf, 1);
            const bool last = (k == ntk - 1);
            // the running key every 8th tile (128 columns: a plan tile), into its fixed registers (see the span-1 walk below);
            // issued ahead of the tile's requests, so the tile's own wait covers it (ScanRun)
            const bool poll = (k & 7) == 0;
            unsigned long long k_raw = ~0ull, d_raw = 0ull;      // TRI: this tile's key load and queue draw
            if constexpr (TRI) {
                // (compiler-visible loads; picked up as operands of the tile's vmcnt(0) below)
                if (poll) k_raw = __hip_atomic_load(&p.ctr64[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (dyn && last && threadIdx.x == 0) {
                    // (the address through a vector register: hipcc rewrites an atomic on a wave-uniform address into one per
                    // wave whose result it broadcasts at once -- a wait for the draw right here, in front of the tile)
                    uint64_t qa = reinterpret_cast<uint64_t>(p.q_ctr);
                    asm volatile("" : "+v"(qa));
                    d_raw = __hip_atomic_fetch_add(reinterpret_cast<__attribute__((address_space(1))) unsigned long long*>(qa), 1ull, __ATOMIC_RELAXED,
                                                   __HIP_MEMORY_SCOPE_AGENT);      // (a global atomic: a flat one would count as an LDS access too)
                }
            } else {
            if (poll) asm volatile("global_load_dwordx2 v[252:253], %0, off sc1" : : "v"(&p.ctr64[1]) : "memory", "v252", "v253");
            if (dyn && last && threadIdx.x == 0)
                asm volatile("global_atomic_add_x2 v[254:255], %0, %1, off sc0" : : "v"(p.q_ctr), "v"(1ull) : "memory", "v254", "v255");
            }
            {
                const int rq = run.req_first(k), nrq = run.req_count(k);
                const int bq = ring_add(buf, NBUF - SPAN);
                if (nrq > 0) dma_tile(ct0 + rq, bq);
                if (nrq > 1) dma_tile(ct0 + rq + 1, ring_add(bq, 1));
            }
            if (nslot == 2 && wave_active && j0 >= j_right) {
                head_tile_lean(buf, buf1, j0);
            } else {
                // a tile on the diagonal, a wave without rows, a run's odd end: slot by slot, every group with its predicate
#pragma unroll 1
                for (int sl = 0; sl < nslot; ++sl) head_walk(sl ? buf1 : buf, j0 + sl * COLS);
            }
            if constexpr (TRI) {
                // nothing of the run stays in flight behind a tile of this ring (ScanRun::outstanding_max = 0)
                asm volatile("s_waitcnt vmcnt(0)" : "+v"(k_raw), "+v"(d_raw) : : "memory");
                if (k_raw < gk) gk = k_raw;                     // the key only ever decreases (~0 where the tile did not poll)
                if (dyn && last && threadIdx.x == 0) { qslot[0] = (uint32_t)d_raw; qslot[1] = (uint32_t)(d_raw >> 32); }
            } else {
            ring_wait(run.outstanding(k));
            if (poll) {
                uint32_t klo, khi;
                asm volatile("v_mov_b32 %0, v252\n\tv_mov_b32 %1, v253" : "=v"(klo), "=v"(khi) : : "memory", "v252", "v253");
                gk_raw = ((unsigned long long)khi << 32) | klo;
                if (gk_raw < gk) gk = gk_raw;                   // the key only ever decreases
            }
            if (dyn && last && threadIdx.x == 0) {
                uint32_t qlo, qhi;
                asm volatile("v_mov_b32 %0, v254\n\tv_mov_b32 %1, v255" : "=v"(qlo), "=v"(qhi) : : "memory", "v254", "v255");
                qslot[0] = qlo; qslot[1] = qhi;
            }
            }
            __syncthreads();                                 // every wave's pieces have landed; all reads of the tile's slots done
            buf = ring_add(buf, SPAN);
        }
    } else
    for (int t = 0; t < ntile; ++t) {
        const int ct = tile_at(t);
        const int ct_next = (t + DIST < ntile) ? tile_at(t + DIST) : ct;      // (a repeat of this tile lands in the free slot)
        int buf_next = buf + DIST;                           // slot of tile t + DIST = slot of tile t - 1:
        if (buf_next >= NBUF) buf_next -= NBUF;              // every wave left it at the previous barrier
        const int j0 = ct * COLS;

        // running best key, re-read every 8th tile by a load the compiler does not see (it would wait for it with
        // vmcnt(0) inside the MFMA loop and so drain the ring): the value is picked up behind this iteration's own
        // counted wait.  Issued ahead of the tile's DMA, so that wait covers it.
        // (RING > 0: every 8th plan tile, as ever; picked up DIST - 1 tiles later, or behind the run's last wait)
        // RING > 0: the key load stays in flight for DIST - 1 tiles and the waits in between are several statements, so its
        // destination cannot be a variable: hipcc is free to copy a variable between two statements, and a copy made
        // before the data is there carries the register's old content (seen: the queue draw's copy in front of the wait).
        // Both results land in fixed registers the compiler never allocates in these kernels -- v[252:255], named as clobbers
        // here and where they are read, above the 187 VGPRs the head kernels use (reported with the kernels' resources:
        // a build whose own allocation reached v252 must not ship) -- and are moved out behind the wait that covers them.
        if (MODE == HM_MODE_ARGMIN && (t & (8 * (G::PLAN_COLS / COLS) - 1)) == 0) {
            if constexpr (RING > 0) {
                asm volatile("global_load_dwordx2 v[252:253], %0, off sc1" : : "v"(&p.ctr64[1]) : "memory", "v252", "v253");
                gk_due = t + DIST - 1;
            } else {
            asm volatile("global_load_dwordx2 %0, %1, off sc1" : "=v"(gk_raw) : "v"(&p.ctr64[1]) : "memory");
            }
            gk_pending = true;
        }
        // item queue: the next item is drawn during this item's last tile (picked up behind the same counted wait)
        if (dyn && t == ntile - 1 && threadIdx.x == 0) {
            if constexpr (RING > 0)
                asm volatile("global_atomic_add_x2 v[254:255], %0, %1, off sc0" : : "v"(p.q_ctr), "v"(1ull) : "memory", "v254", "v255");
            else
            asm volatile("global_atomic_add_x2 %0, %1, %2, off sc0" : "=v"(q_raw) : "v"(p.q_ctr), "v"(1ull) : "memory");
        }
        if constexpr (RING > 0) {
            if (t + DIST < ntile) dma_tile(ct_next, buf_next);      // (no repeats: the waits below count what is left of the run)
        } else {
        dma_tile(ct_next, buf_next);
        }

        if constexpr (HEAD > 0) {           // a head kernel walks every tile this way
            head_walk(buf, j0);
        } else if constexpr (!PIPE) {
            // one accumulator set: MFMAs, then the bound test of the same group (the other resident block of the CU
            // fills the matrix pipe meanwhile); the first fragment of the next group is still requested early
            bool prev = false;
#pragma unroll 1
            for (int sub = 0; sub < SUB; ++sub) {
                const int j0s = j0 + sub * 32;
                const bool do_c = wave_active && (j0s + 31 > i0w);
                if (do_c) {
                    float ext_u = 0.0f;
                    mma_group(std::integral_constant<int, 0>{}, std::false_type{}, buf, sub, !prev, ext_u);
                    ext_u = reduce_group(std::integral_constant<int, 0>{});
                    finish_group(std::integral_constant<int, 0>{}, ext_u, j0s);
                }
                prev = do_c;
            }
        } else {
            // two groups per pass, the accumulator sets alternating (a rolled loop: two code sites for the slow path)
#pragma unroll 1
            for (int sp = 0; sp < SUB / 2; ++sp) {
                if constexpr (DEEP) {
                    const int ja = j0 + 2 * sp * 32, jb = ja + 32;
                    if (wave_active && (ja + 31 > i0w) && pend) {     // both groups of the pass run (jb > ja) and one is pending
                        float ea = 0.0f, eb = 0.0f;
                        mma_group_deep(std::integral_constant<int, 0>{}, buf, 2 * sp, !deep_valid, ea);
                        finish_group(std::integral_constant<int, 1>{}, ea, pend_j0s);
                        const bool more = 2 * sp + 2 < SUB;
                        mma_group_deep(std::integral_constant<int, 1>{}, buf, 2 * sp + 1, false, eb);
                        finish_group(std::integral_constant<int, 0>{}, eb, ja);
                        pend_j0s = jb;
                        deep_valid = more;                            // bfr[0] holds the fragments of the tile's next group
                        continue;
                    }
                    deep_valid = false;
                }
                {
                    const int sub = 2 * sp;
                    const int j0s = j0 + sub * 32;
                    const bool do_c = wave_active && (j0s + 31 > i0w);
                    float ext_u = 0.0f;
                    if (do_c && pend) {                           // the common case: one basic block, MFMAs + the other set's test
                        mma_group(std::integral_constant<int, 0>{}, std::true_type{}, buf, sub, sp == 0, ext_u);
                    } else {
                        if (do_c) mma_group(std::integral_constant<int, 0>{}, std::false_type{}, buf, sub, true, ext_u);
                        if (pend) ext_u = reduce_group(std::integral_constant<int, 1>{});
                    }
                    if (pend) finish_group(std::integral_constant<int, 1>{}, ext_u, pend_j0s);
                    pend = do_c;
                    pend_j0s = j0s;
                }
                {
                    const int sub = 2 * sp + 1;
                    const int j0s = j0 + sub * 32;
                    const bool do_c = wave_active && (j0s + 31 > i0w);
                    float ext_u = 0.0f;
                    if (do_c && pend) {                           // the previous group ran: its last k-step requested our first fragment
                        mma_group(std::integral_constant<int, 1>{}, std::true_type{}, buf, sub, false, ext_u);
                    } else {
                        if (do_c) mma_group(std::integral_constant<int, 1>{}, std::false_type{}, buf, sub, true, ext_u);
                        if (pend) ext_u = reduce_group(std::integral_constant<int, 0>{});
                    }
                    if (pend) finish_group(std::integral_constant<int, 0>{}, ext_u, pend_j0s);
                    pend = do_c;
                    pend_j0s = j0s;
                }
            }
        }

        // tile t+1 has landed (this wave's pieces) -- and so has the key load, if one was issued
        if constexpr (RING > 0) {
            // tiles t + 2 .. of the run may stay in flight, DIST - 1 of them at most; behind the last tile nothing does
            ring_wait(ntile - 2 - t);
            // the key load is complete once the wait has passed the tile requested right behind it (tile t_issue + DIST: loads
            // return in order), or behind the run's last wait, a vmcnt(0); the draw goes out during the last tile only
            if (gk_pending && (t >= gk_due || t == ntile - 1)) {
                uint32_t klo, khi;
                asm volatile("v_mov_b32 %0, v252\n\tv_mov_b32 %1, v253" : "=v"(klo), "=v"(khi) : : "memory", "v252", "v253");
                gk_raw = ((unsigned long long)khi << 32) | klo;
                if (gk_raw < gk) gk = gk_raw;
                gk_pending = false;
            }
            if (dyn && t == ntile - 1 && threadIdx.x == 0) {
                uint32_t qlo, qhi;
                asm volatile("v_mov_b32 %0, v254\n\tv_mov_b32 %1, v255" : "=v"(qlo), "=v"(qhi) : : "memory", "v254", "v255");
                q_raw = ((unsigned long long)qhi << 32) | qlo;
            }
        } else {
        if (DIST - 1 <= 0) asm volatile("s_waitcnt vmcnt(0)" : "+v"(gk_raw), "+v"(q_raw) : : "memory");
        else asm volatile("s_waitcnt vmcnt(%2)" : "+v"(gk_raw), "+v"(q_raw) : "n"((DIST - 1) * PPW) : "memory");
        if (MODE == HM_MODE_ARGMIN && gk_pending) {
            if (gk_raw < gk) gk = gk_raw;                   // the key only ever decreases
            gk_pending = false;
        }
        }
        if (dyn && t == ntile - 1 && threadIdx.x == 0) { qslot[0] = (uint32_t)q_raw; qslot[1] = (uint32_t)(q_raw >> 32); }
        __syncthreads();                                     // ... and every wave's; all reads of slot `buf` done
        if (++buf == NBUF) buf = 0;
    }
    if constexpr (PIPE) {
        if (pend) {                                          // the last group of the run (set (SUB - 1) % 2 = 1)
            const float ext_u = reduce_group(std::integral_constant<int, 1>{});
            finish_group(std::integral_constant<int, 1>{}, ext_u, pend_j0s);
        }
    }

    // nothing of this run may land later (RING > 0: its last wait was a vmcnt(0) already)
    if (DIST > 1 && RING == 0) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); __syncthreads(); }
    }   // have

    if (!dyn) break;
    if (!have) {
        // an item left of the diagonal: draw at once (the barrier in front keeps the slot's previous value readable
        // until every wave has it)
        __syncthreads();
        if (threadIdx.x == 0) {
            const unsigned long long v = __hip_atomic_fetch_add(p.q_ctr, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            qslot[0] = (uint32_t)v; qslot[1] = (uint32_t)(v >> 32);
        }
        __syncthreads();
    }
    {
        const uint32_t qlo = __builtin_amdgcn_readfirstlane(qslot[0]), qhi = __builtin_amdgcn_readfirstlane(qslot[1]);
        const unsigned long long q = ((unsigned long long)qhi << 32) | qlo;
        if ((q >> 24) != (p.q_tag >> 24)) break;            // (a foreign tag: never within one launch's lifetime)
        item = (int)gridDim.x + (int)(q & 0xffffffull);
        if (item >= p.n_items) break;
    }
    }   // items

    if constexpr (HEAD > 0) {
        // a wave that had to recompute most of its groups tells the host that the bound is too loose for this kernel
        if (lane == 0 && hg_tot >= 16 && 2 * hc_tot > hg_tot) __hip_atomic_store(p.head_bad, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    if (MODE == HM_MODE_TOPK) {
        // one 64-bit atomic per wave for the sure count
        unsigned long long s = sure_total;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
        if (lane == 0 && s != 0) atomicAdd(&p.ctr64[0], s);
    }
    if (MODE == HM_MODE_HIST) {
        __syncthreads();
        for (int t = threadIdx.x; t < HM_HIST_BINS; t += NTHREADS)
            if (lhist[t]) atomicAdd(&p.hist[t], lhist[t]);
    }
}

// ------------------------------------------------------------------------------------------------
// launch
// ------------------------------------------------------------------------------------------------
template <int NG, int SIGN, int MODE, int BF, int TM, int WPB, int SUB, bool WK = false, int HEAD = 0, int RING = 0, int SPAN = 1>
static hipError_t hm_launch_scan_t(hm_engine* e, const ScanArgs& a, dim3 grid, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1)
{
    using G = ScanGeom<NG, BF, TM, WPB, SUB, RING, SPAN>;
    const size_t lds = G::lds_bytes(MODE);
    static_assert(RING == 0 || G::lds_bytes(MODE) <= HM_LDS_PER_BLOCK, "a deeper ring keeps two blocks per CU");
    static_assert(G::BLOCKS != 3 || 3 * hm_lds_alloc(G::lds_bytes(MODE)) <= HM_LDS_PER_CU, "a three-block ring keeps three");
    const void* fn = reinterpret_cast<const void*>(&hm_scan_kernel<NG, SIGN, MODE, BF, TM, WPB, SUB, WK, HEAD, RING, SPAN>);
    if (lds > 48 * 1024 && e->attr_done.find(fn) == e->attr_done.end()) {     // per engine (= per device), not process-wide
        hipError_t st = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (st != hipSuccess) return st;
        e->attr_done.insert(fn);
    }
    // timed launches carry their events in the dispatch itself (start / stop timestamps of this kernel): a pair of
    // hipEventRecord calls around it costs two ~6 us bubbles on the stream
    ScanArgs b = a;
    b.n_items = (int)grid.x;
    b.dyn = 0;
    // item queue (ScanArgs::dyn): every launch with more items than resident slots, both prefilter forms (measured:
    // profiles/r03g_ab_item_queue_*: -3 % launch time for the bf16 form at V = 50 k / 100 k, -2.8 % for the fp32 form)
    if (e->dyn_queue && MODE != HM_MODE_HIST && grid.x < (1u << 24)) {
        auto it = e->scan_slots.find(fn);
        if (it == e->scan_slots.end()) {
            int per_cu = 0;
            hipError_t st = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, G::NTHREADS, lds);
            if (st != hipSuccess) return st;
            it = e->scan_slots.emplace(fn, std::max(1, per_cu) * e->n_cu).first;
        }
        const int slots = e->dyn_slots > 0 ? e->dyn_slots : it->second;
        if ((int)grid.x > slots) {
            grid.x = (unsigned)slots;
            b.dyn = 1;
            b.q_tag = (++e->scan_tag) << 24;
            b.q_ctr = e->d_queue + 16 * ((b.ctr64 == e->d_ctr64) ? 0 : 1);      // one word per counter set (the pipelined loop alternates them)
        }
    }
    if (ev0 != nullptr || ev1 != nullptr) hipExtLaunchKernelGGL((hm_scan_kernel<NG, SIGN, MODE, BF, TM, WPB, SUB, WK, HEAD, RING, SPAN>), grid, dim3(G::NTHREADS), lds, s, ev0, ev1, 0, b);
    else hipLaunchKernelGGL((hm_scan_kernel<NG, SIGN, MODE, BF, TM, WPB, SUB, WK, HEAD, RING, SPAN>), grid, dim3(G::NTHREADS), lds, s, b);
    return hipGetLastError();
}

template <int NG, int BF, int TM, int WPB, int SUB>
static hipError_t hm_launch_scan_ng(hm_engine* e, int sign, int mode, const ScanArgs& a, dim3 grid, hipStream_t s, hipEvent_t ev0,
                                    hipEvent_t ev1)
{
    if (sign) {
        if (mode == HM_MODE_TOPK) return hm_launch_scan_t<NG, 1, HM_MODE_TOPK, BF, TM, WPB, SUB>(e, a, grid, s, ev0, ev1);
        if (mode == HM_MODE_ARGMIN) {
            // the head test (knob `head`, 0 = off; hm_head_live: only when the host expects a tight bound): 64-row waves of
            // the bf16 form whose rows have more k-steps than the head.  Otherwise the unchanged HEAD = 0 kernel.
            constexpr int HD = (BF != 0 && TM <= HM_SCAN_PIPE_MAX_TM) ? hm_head_steps(NG) : 0;
            if constexpr (HD > 0) {
                if (hm_head_live(e)) {
                    // the head kernels' ring and span (kScanRings, ScanRun; knobs `head_ring`, `head_span`): the one place that gives
                    // a kernel another ring than 0 or another span than 1.  A span the width's ring has no slots for is the
                    // geometry's to replace (ScanGeom::SPAN): that launch takes the ring's span-1 kernel
#define HM_HEAD_RING_CASE(R, S)                                                                                            \
    case 4 * S + R: {                                                                                                      \
        constexpr int RG = ScanGeom<NG, BF, TM, WPB, SUB, R, S>::RING, SP = ScanGeom<NG, BF, TM, WPB, SUB, R, S>::SPAN; \
        if (a.key_wide) return hm_launch_scan_t<NG, 1, HM_MODE_ARGMIN, BF, TM, WPB, SUB, true, HD, RG, SP>(e, a, grid, s, ev0, ev1); \
        return hm_launch_scan_t<NG, 1, HM_MODE_ARGMIN, BF, TM, WPB, SUB, false, HD, RG, SP>(e, a, grid, s, ev0, ev1);      \
    }
                    // (ring 3 is ring 1 with span 1 and at the widths where three blocks do not fit a CU: ScanGeom::RING)
                    static_assert(HM_SCAN_RINGS == 4, "one case per ring and span");
                    switch (4 * (e->head_ring == 0 ? 1 : e->head_span) + e->head_ring) {      // (ring 0 ignores the span)
                        HM_HEAD_RING_CASE(0, 1) HM_HEAD_RING_CASE(1, 1) HM_HEAD_RING_CASE(2, 1) HM_HEAD_RING_CASE(3, 1)
                        HM_HEAD_RING_CASE(1, 2) HM_HEAD_RING_CASE(2, 2) HM_HEAD_RING_CASE(3, 2)
                    }
#undef HM_HEAD_RING_CASE
                    return hipErrorInvalidValue;
                }
            }
            if (a.key_wide) return hm_launch_scan_t<NG, 1, HM_MODE_ARGMIN, BF, TM, WPB, SUB, true>(e, a, grid, s, ev0, ev1);
            return hm_launch_scan_t<NG, 1, HM_MODE_ARGMIN, BF, TM, WPB, SUB>(e, a, grid, s, ev0, ev1);
        }
        return hm_launch_scan_t<NG, 1, HM_MODE_HIST, BF, TM, WPB, SUB>(e, a, grid, s, ev0, ev1);
    }
    if (mode == HM_MODE_TOPK) return hm_launch_scan_t<NG, 0, HM_MODE_TOPK, BF, TM, WPB, SUB>(e, a, grid, s, ev0, ev1);
    if (mode == HM_MODE_ARGMIN) {
        if (a.key_wide) return hm_launch_scan_t<NG, 0, HM_MODE_ARGMIN, BF, TM, WPB, SUB, true>(e, a, grid, s, ev0, ev1);
        return hm_launch_scan_t<NG, 0, HM_MODE_ARGMIN, BF, TM, WPB, SUB>(e, a, grid, s, ev0, ev1);
    }
    return hm_launch_scan_t<NG, 0, HM_MODE_HIST, BF, TM, WPB, SUB>(e, a, grid, s, ev0, ev1);
}

// Which prefilter form a scan uses.  The bf16 form's error bound 0.00782 * max||x_s||^2 only costs
// extra emissions, never correctness; auto picks it from d >= 24 (below that the fp32 form is already short).
bool hm_use_bf16(const hm_engine* e)
{
    if (!e->bf16_ok || e->force_f32) return false;
    if (e->precision == HM_PREFILTER_F32) return false;
    if (e->precision == HM_PREFILTER_BF16) return true;
    return e->d >= 24;
}

// bf16 form: the kernels of block shape S (kScanShapes), one per built width.  Shapes other than 0 exist up to
// HM_SCAN_BIG_MAX_KC chunks only; a width or shape this build has no kernel for is an error, never another kernel.
template <int S>
static hipError_t hm_launch_scan_bf16(hm_engine* e, int mode, const ScanArgs& a, dim3 grid, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1)
{
    constexpr int TM = kScanShapes[S].tm, WPB = kScanShapes[S].wpb;
    static_assert(ScanGeom<13, 1, TM, WPB, HM_SUB_BF16>::BLOCK_ROWS == hm_shape_rows(S), "the item plan counts this shape's rows per block");
#define HM_KC_CASE(KCv)                                                                                                    \
    case KCv:                                                                                                              \
        if constexpr (S == 0 || KCv <= HM_SCAN_BIG_MAX_KC)                                                                 \
            return hm_launch_scan_ng<KCv, 1, TM, WPB, HM_SUB_BF16>(e, e->sign_mode, mode, a, grid, s, ev0, ev1);          \
        break;
    switch (e->KC) { HM_SCAN_KC_LIST(HM_KC_CASE, HM_SCAN_WIDTHS_BUILT) }
#undef HM_KC_CASE
    return hipErrorInvalidValue;
}

hipError_t hm_launch_scan(hm_engine* e, int mode, const ScanArgs& a, dim3 grid, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1)
{
    if (a.bf16) {
        switch (a.shape) {
            case 0: return hm_launch_scan_bf16<0>(e, mode, a, grid, s, ev0, ev1);
            case 1: return hm_launch_scan_bf16<1>(e, mode, a, grid, s, ev0, ev1);
#if HM_SCAN_ALL_SHAPES
            case 2: return hm_launch_scan_bf16<2>(e, mode, a, grid, s, ev0, ev1);
            case 3: return hm_launch_scan_bf16<3>(e, mode, a, grid, s, ev0, ev1);
            case 4: return hm_launch_scan_bf16<4>(e, mode, a, grid, s, ev0, ev1);
#endif
        }
        return hipErrorInvalidValue;
    }
    // fp32 form: block shape 0 only
    constexpr int TM = kScanShapes[0].tm, WPB = kScanShapes[0].wpb;
#define HM_NG_CASE(NGv) case NGv: return hm_launch_scan_ng<NGv, 0, TM, WPB, HM_SUB_F32>(e, e->sign_mode, mode, a, grid, s, ev0, ev1);
    switch (e->NG) { HM_SCAN_NG_LIST(HM_NG_CASE, HM_SCAN_WIDTHS_BUILT) }
#undef HM_NG_CASE
    return hipErrorInvalidValue;
}

// common argument preparation; returns false when the row range is empty.  Every decision about the launch's geometry is
// hm_scan_plan's (hm_scan_plan.h); here the plan is copied into ScanArgs and the engine's pointers and key shifts are filled in
bool hm_prepare_scan(hm_engine* e, const Bounds& b, int64_t row_begin, int64_t row_end, ScanArgs& a, dim3& grid, int64_t n_limit,
                     int64_t col_begin, int mode)
{
    const int bf16 = hm_use_bf16(e) ? 1 : 0;
    // (the condition under which hm_launch_scan_ng picks a head kernel for a 64-row-wave launch)
    const int head = (mode == HM_MODE_ARGMIN && bf16 && e->sign_mode && hm_head_steps(e->KC) > 0 && hm_head_live(e)) ? 1 : 0;
    const ScanPlan pl = hm_scan_plan(e->plan, ScanRequest{e->n, row_begin, row_end, n_limit, col_begin, bf16, e->KC, head});
    if (!pl.ok) return false;
    memset(&a, 0, sizeof(a));
    a.img = e->img;
    a.img16 = e->img16;
    a.bf16 = bf16;
    a.shape = pl.shape;
    a.n = pl.n;
    a.row_begin = pl.row_begin;
    a.row_end = pl.row_end;
    a.col_begin = pl.col_begin;
    a.rb_first = pl.rb_first;
    a.nct = pl.nct;
    a.items = pl.items;
    a.u_hi = b.u_hi;
    a.u_lo = b.u_lo;
    a.thr_pos = b.thr_pos;
    a.count_sure = 1;
    a.cut_bits = 0xffffffffu;
    a.tie_imax = 0x7fffffff;
    a.ent = e->ent;
    a.ent_cap = e->ent_cap;
    a.ctr64 = e->d_ctr64;
    a.hist = e->d_hist;
    a.sample_stride = 1;
    a.rmax2_bits = e->d_rmax2;
    a.head_bad = &e->h->head_bad;
    a.stop = nullptr;
    a.key_wide = e->key_ib > HM_KEY_IB_NARROW ? 1 : 0;
    a.key_si = 32 - e->key_ib;
    a.key_sj = 2 * e->key_ib - 32;
    grid = dim3((unsigned)pl.n_items, 1, 1);
    return true;
}
