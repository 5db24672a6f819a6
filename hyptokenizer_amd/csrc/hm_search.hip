// hm_search.hip -- exact re-evaluation and selection of what the pair scan emitted, and the search entry
// points of the C ABI (hm_pairwise_argmin / _argmin_dev / _topk / _candidates, hm_row_argmin).
//
// The scan (hm_scan.hip) only SELECTS: every reported distance is recomputed here in the canonical fp32
// arithmetic from the fp32 image -- a half-wave per entry (coalesced 128-byte row reads,
// ATen's 32 summation chains one per lane), thresholds compare in fp32, order = (distance bits, i, j).
#include "hm_common.h"
#include "hm_cut_plan.h"
#include "hm_rows_device.h"

#pragma clang fp contract(off)

// ------------------------------------------------------------------------------------------------
// argmin tail: re-evaluation + final record + seed + arming (+ the merge itself when asked for): ONE launch
// ------------------------------------------------------------------------------------------------
struct TailArgs {
    const uint4* ent;
    unsigned long long* ctr64;       // [1] running key (re-armed), [2] emitted (read, re-armed)
    uint32_t cap;
    float* img;
    unsigned char* img16;
    int RS, d, KC, sign_mode;
    float sqrt_c, thr;
    ArgminPart* parts;
    uint32_t* ticket;
    ArgminRec* out;                  // record
    ArgminRec* out2;                 // may be NULL: {found = emitted low, dbits = emitted high}
    ArgminSeed* seed;                // may be NULL: no seed update
    int bf, kterms;
    uint32_t* rmax2_bits;
    int arm, arm_rb, arm_re;         // leave counters + running key ready for the next search of rows [arm_rb, arm_re)
    int key_si, key_sj;              // the engine's running-key layout (hm_key_low)
    MergeFuse mf;
};

__global__ __launch_bounds__(HM_TAIL_THREADS) void hm_argmin_tail_kernel(const TailArgs a)
{
    __shared__ uint32_t s0[HM_TAIL_THREADS / 64], s1[HM_TAIL_THREADS / 64], s2[HM_TAIL_THREADS / 64];
    __shared__ uint32_t s_last;
    __shared__ MidScratch ms;
    const int lane = threadIdx.x & 63;
    __builtin_amdgcn_s_setprio(3);          // in the pipelined loop this latency-bound chain shares its SIMDs with the next scan's MFMA waves
    LoopState* loop = a.mf.loop;
    if (loop != nullptr && loop->stop != 0u) {                 // the loop ended at an earlier step: this one is skipped
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            ArgminRec r; r.found = 3u; r.dbits = 0; r.i = 0xffffffffu; r.j = 0xffffffffu;
            *a.out = r;
            if (a.mf.rec_ring) *a.mf.rec_ring = r;
        }
        return;
    }
    const unsigned long long emitted = a.ctr64[2];
    // (an overflowed search reports found = 2 whatever its entries say: none of them is read.  The pipelined loop's small
    // tail grid -- it runs beside a scan -- hands a step with more than HM_PIPE_TAIL_MAX survivors back the same way: the
    // host redoes that one step through hm_pairwise_argmin and its full-size tail)
    const bool over_small = a.mf.rowkey != nullptr && emitted <= (unsigned long long)a.cap && emitted > (unsigned long long)HM_PIPE_TAIL_MAX;
    const bool over = emitted > (unsigned long long)a.cap || over_small;
    const uint32_t m = over ? 0u : (uint32_t)emitted;
    uint32_t active = (m + HM_TAIL_SOLO - 1) / HM_TAIL_SOLO;       // HM_TAIL_SOLO = entries one block takes per two rounds
    if (active < 1) active = 1;
    if (active > gridDim.x) active = gridDim.x;
    if (blockIdx.x >= active) return;

    // ---- exact distance of this block's entries, lexicographic min of (d bits, i, j) with d < thr ----
    uint32_t b0 = 0xffffffffu, b1 = 0xffffffffu, b2 = 0xffffffffu;
    // a half-wave takes HM_GATHER consecutive entries per round (hm_halfwave_gather): lane t finishes entry t
    // (the block size is the launch's: 1024 threads, or 256 in the pipelined loop where the kernel has to fit beside a scan block)
    const uint32_t hw = (blockIdx.x * blockDim.x + threadIdx.x) >> 5;               // half-wave id
    const uint32_t stride = active * (blockDim.x >> 5) * HM_GATHER;
    const int t32 = lane & 31;
    for (uint32_t base = (hw & ~1u) * HM_GATHER; base < m; base += stride) {             // wave-uniform trip count
        const uint32_t mybase = base + (hw & 1u) * HM_GATHER;
        const uint32_t mine = mybase + t32;
        const uint4 en = a.ent[mine < m ? mine : m - 1];
        const float u = hm_halfwave_gather(lane, [&](int k) {
            const uint32_t ri = __shfl(en.y, (lane & 32) + k, 64), rj = __shfl(en.z, (lane & 32) + k, 64);
            return hm_img_u_halfwave(a.img, a.RS, a.d, ri, rj, a.sign_mode, lane);
        });
        const float dd = hm::dist_from_u(u, a.sqrt_c);
        if (t32 < HM_GATHER && mine < m && dd < a.thr) {
            const uint32_t db = hm::fbits(dd);
            if (hm_key_less(db, en.y, en.z, b0, b1, b2)) { b0 = db; b1 = en.y; b2 = en.z; }
        }
    }
    hm_block_min_key(b0, b1, b2, s0, s1, s2);

    if (active > 1) {
        // several blocks took part: partial records, then the last block to arrive reduces them (agent-scope
        // release / acquire around a ticket; rare path -- more than HM_TAIL_SOLO survivors)
        if (threadIdx.x == 0) {
            ArgminPart pt; pt.dbits = b0; pt.i = b1; pt.j = b2; pt.pad = 0;
            a.parts[blockIdx.x] = pt;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            const uint32_t tk = __hip_atomic_fetch_add(a.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            s_last = (tk == active - 1) ? 1u : 0u;
            if (s_last) {
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                *a.ticket = 0u;
            }
        }
        __syncthreads();
        if (s_last == 0u) return;
        b0 = b1 = b2 = 0xffffffffu;
        if (threadIdx.x < active) {
            const ArgminPart pt = a.parts[threadIdx.x];
            b0 = pt.dbits; b1 = pt.i; b2 = pt.j;
        }
        hm_block_min_key(b0, b1, b2, s0, s1, s2);
    }

    // pipelined loop: the pairs of the newest row were searched by their own small kernel
    if (a.mf.rowkey != nullptr) {
        const unsigned long long rk = *a.mf.rowkey;
        if (rk != ~0ull) {
            const uint32_t db = (uint32_t)(rk >> 32), ri = (uint32_t)rk, rj = a.mf.rowkey_j;
            if (hm_key_less(db, ri, rj, b0, b1, b2)) { b0 = db; b1 = ri; b2 = rj; }
        }
    }
    // ---- final (one block): record, seed, arming, merge ----
    // found = 2: the emission buffer overflowed, the record is not final (the caller reruns bounded)
    const uint32_t found = over ? 2u : ((b1 != 0xffffffffu) ? 1u : 0u);
    if (threadIdx.x >= 64) return;                              // wave 0 finishes (b0, b1, b2 are block-uniform)
    const uint32_t bi = b1, bj = b2;
    if (lane == 0) {
        ArgminRec r; r.found = found; r.dbits = b0; r.i = bi; r.j = bj;
        *a.out = r;
        if (a.mf.rec_ring) *a.mf.rec_ring = r;
        if (a.out2) { a.out2->found = (uint32_t)emitted; a.out2->dbits = (uint32_t)(emitted >> 32); }
    }
    unsigned long long seed_key = ~0ull;
    uint32_t seed_row = 0xffffffffu;
    if (a.seed != nullptr) {
        if (found == 1u) {
            // a final record becomes the next search's seed: key = (bits(u_c + delta), all ones) -- the pair's own
            // prefilter value is <= u_c + delta, and an entry the scan skips on this key has u_f >= u_c + 3 delta, so it
            // cannot order before the pair -- or, for a pair at distance 0 (u_c <= 1), the exact zero-class key
            const float u = hm_img_u_halfwave(a.img, a.RS, a.d, bi, bj, a.sign_mode, lane);
            if (u <= 1.0f) seed_key = (0x3f7fffffull << 32) | (unsigned long long)hm_key_low(bi, bj, a.key_si, a.key_sj);
            else seed_key = ((unsigned long long)hm::fbits(u + hm_scan_delta(a.bf != 0, a.kterms, a.rmax2_bits)) << 32) | 0xffffffffull;
            seed_row = bi;
            if (lane == 0) { a.seed->key = seed_key; a.seed->i = bi; a.seed->valid = 1u; }
        } else if (a.seed->valid != 0u) {
            seed_key = a.seed->key;
            seed_row = a.seed->i;
        }
    }
    // arm the next search over the same row range: emitted = 0, running key = seed -- the merge loop then goes from
    // this kernel straight into the next scan
    if (a.arm && found != 2u && lane == 0) {
        const bool use = seed_row != 0xffffffffu && (int)seed_row >= a.arm_rb && (int)seed_row < a.arm_re;
        a.ctr64[0] = 0ull;
        a.ctr64[1] = use ? seed_key : ~0ull;
        a.ctr64[2] = 0ull;
        if (a.mf.rowkey != nullptr) *a.mf.rowkey = ~0ull;
    }
    // ---- fused merge of the pair just found (device-resident loop) ----
    if (a.mf.X != nullptr) {
        if (found == 1u) {
            const int32_t li = a.mf.len[bi], lj = a.mf.len[bj];
            const float w = (float)((double)lj / (double)(li + lj));     // len(tj) / (len(ti) + len(tj)), hyperbolic_merge.py:317-323
            hm_wave_stage_rows(a.img, a.RS, a.d, bi, bj, ms, lane);
            const float r2 = hm_wave_midpoint(a.d, w, a.mf.c, a.sign_mode, ms, true, lane);
            hm_wave_store_row(ms, r2, a.d, a.RS, a.KC, a.mf.X, a.mf.ld, a.img, a.img16, a.mf.new_row, a.rmax2_bits, lane);
            if (lane == 0) {
                a.mf.len_rw[a.mf.new_row] = li + lj;
                if (loop) loop->steps_done += 1u;
            }
        } else if (loop != nullptr && lane == 0) {
            loop->stop = found == 2u ? (over_small ? 6u : 2u) : 1u;       // (6: too many survivors for the pipelined loop's tail grid only)
        }
    }
    if (a.mf.rowkey != nullptr && loop != nullptr && lane == 0) loop->tails_done += 1u;      // (pipelined loop: the scans' order guard)
}

int hm_launch_argmin_tail(hm_engine* e, const ScanArgs& sa, float sqrt_c, float thr, ArgminRec* rec_out, bool with_seed,
                          int arm_rb, int arm_re, bool arm, const MergeFuse& mf, hipStream_t s)
{
    TailArgs t;
    memset(&t, 0, sizeof(t));
    t.ent = mf.pipe_ent ? mf.pipe_ent : e->ent; t.ctr64 = mf.pipe_ctr64 ? mf.pipe_ctr64 : e->d_ctr64; t.cap = e->ent_cap;
    t.img = e->img; t.img16 = e->img16; t.RS = e->RS; t.d = e->d; t.KC = e->KC; t.sign_mode = e->sign_mode;
    t.sqrt_c = sqrt_c; t.thr = thr;
    t.parts = e->d_parts; t.ticket = e->d_ctr + HM_CTR_TAIL_TICKET;
    t.out = rec_out; t.out2 = (rec_out == e->d_rec) ? e->d_rec + 1 : nullptr;
    t.seed = with_seed ? e->d_seed : nullptr;
    t.bf = sa.bf16; t.kterms = sa.bf16 ? 8 * e->KC : e->RS; t.rmax2_bits = e->d_rmax2;
    t.arm = arm ? 1 : 0; t.arm_rb = arm_rb; t.arm_re = arm_re;
    t.key_si = 32 - e->key_ib; t.key_sj = 2 * e->key_ib - 32;
    t.mf = mf;
    // Pipelined loop (mf.rowkey set): the kernel runs UNDER the next step's scan, whose two blocks per CU leave room for four
    // more waves at most -- 256-thread blocks; otherwise 1024
    // -- and four of them: every block of the grid has to find a slot before the kernel can end, whether it has entries or not
    hipLaunchKernelGGL(hm_argmin_tail_kernel, dim3(mf.rowkey != nullptr ? 4 : HM_TAIL_BLOCKS), dim3(mf.rowkey != nullptr ? 256 : HM_TAIL_THREADS), 0, s, t);
    HM_HIP(hipGetLastError());
    return HM_OK;
}

// counters + running-key seed of an argmin search that was not armed by its predecessor
__global__ void hm_seed_init_kernel(const ArgminSeed* __restrict__ seed, unsigned long long* __restrict__ ctr64, uint32_t* __restrict__ ctr,
                                    int row_begin, int row_end)
{
    if (threadIdx.x < 8) ctr[threadIdx.x] = 0u;
    if (threadIdx.x == 0) {
        const bool use = seed->valid != 0u && (int)seed->i >= row_begin && (int)seed->i < row_end;
        ctr64[0] = 0ull;
        ctr64[1] = use ? seed->key : ~0ull;
        ctr64[2] = 0ull;
        ctr64[3] = 0ull;
    }
}

int hm_launch_seed_init(hm_engine* e, const ScanArgs& a, hipStream_t s)
{
    // (a.ctr64: the engine's first counter set, or the second one of the pipelined loop)
    hipLaunchKernelGGL(hm_seed_init_kernel, dim3(1), dim3(64), 0, s, e->d_seed, a.ctr64, e->d_ctr, a.row_begin, a.row_end);
    HM_HIP(hipGetLastError());
    return HM_OK;
}

// ------------------------------------------------------------------------------------------------
// top-k: exact distances of the emitted entries
// ------------------------------------------------------------------------------------------------
// entries {bits(u_f'), i, j, sure} -> {dbits | 0xffffffff, i, j, bits(u_c')} with the canonical distance.
// counts = the engine's counters from HM_CTR_POST_FIRST on: HM_CTR_VALID, HM_CTR_BORDERLINE (valid & !sure), HM_CTR_MARGIN_BAD
// (sure & !valid, margin violated: must be 0), HM_CTR_COMPLETE = valid entries of the COMPLETE region -- the part of the pair space of which every pair was emitted:
//   without a row cut: u_c' <= 1 (distance 0) or bits(u_c') + hm_tie_slack(cut_bits) <= cut_bits (a pair with u_c' <= cut
//   has u_f' <= cut + delta and was emitted; the slack covers the few-ulp wiggle of acosh);
//   with a row cut (tie flood): the zero-distance pairs of rows i <= tie_imax.
__global__ __launch_bounds__(256) void hm_post_distance_kernel(uint4* __restrict__ ent, const unsigned long long* __restrict__ ctr64,
                                                               uint32_t cap, const float* __restrict__ img, int RS, int d, int sign_mode,
                                                               float sqrt_c, float thr, uint32_t cut_bits, int tie_imax,
                                                               uint32_t* __restrict__ counts)
{
    const unsigned long long emitted = ctr64[HM_CTR64_EMITTED];
    const uint32_t m = emitted > (unsigned long long)cap ? cap : (uint32_t)emitted;
    const int lane = threadIdx.x & 63;
    uint32_t nv = 0, nb = 0, bad = 0, nc = 0;
    const uint32_t hw = (blockIdx.x * blockDim.x + threadIdx.x) >> 5;
    const uint32_t stride = ((gridDim.x * blockDim.x) >> 5) * HM_GATHER;
    const int t32 = lane & 31;
    for (uint32_t base = (hw & ~1u) * HM_GATHER; base < m; base += stride) {
        const uint32_t mybase = base + (hw & 1u) * HM_GATHER;
        const uint32_t mine = mybase + t32;
        const uint4 en = ent[mine < m ? mine : m - 1];
        const float u = hm_halfwave_gather(lane, [&](int k) {
            const uint32_t ri = __shfl(en.y, (lane & 32) + k, 64), rj = __shfl(en.z, (lane & 32) + k, 64);
            return hm_img_u_halfwave(img, RS, d, ri, rj, sign_mode, lane);
        });
        const float uc = hm::clamp_min_one(u);
        const float dd = hm::acosh_c(uc) / sqrt_c;
        if (t32 < HM_GATHER && mine < m) {
            const bool valid = dd < thr;
            nv += valid ? 1u : 0u;
            nb += (valid && en.w == 0u) ? 1u : 0u;
            bad += (!valid && en.w != 0u) ? 1u : 0u;
            const uint32_t ub = hm::fbits(uc);
            const bool zero = ub <= 0x3f800000u;
            const bool complete = tie_imax != 0x7fffffff ? (zero && (int)en.y <= tie_imax)
                                                         : (zero || (cut_bits != 0xffffffffu ? (ub + hm_tie_slack(cut_bits) <= cut_bits) : true));
            nc += (valid && complete) ? 1u : 0u;
            ent[mine] = make_uint4(valid ? hm::fbits(dd) : 0xffffffffu, en.y, en.z, ub);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        nv += __shfl_xor(nv, off, 64); nb += __shfl_xor(nb, off, 64); bad += __shfl_xor(bad, off, 64); nc += __shfl_xor(nc, off, 64);
    }
    if (lane == 0) {
        if (nv) atomicAdd(&counts[HM_CTR_VALID - HM_CTR_POST_FIRST], nv);
        if (nb) atomicAdd(&counts[HM_CTR_BORDERLINE - HM_CTR_POST_FIRST], nb);
        if (bad) atomicAdd(&counts[HM_CTR_MARGIN_BAD - HM_CTR_POST_FIRST], bad);
        if (nc) atomicAdd(&counts[HM_CTR_COMPLETE - HM_CTR_POST_FIRST], nc);
    }
}

// radix narrowing: digit `level` (0..8) of the 96-bit key (12|12|8 bits per word)
__device__ __host__ __forceinline__ void hm_digit_pos(int level, int& word, int& shift, int& bits)
{
    word = level / 3;
    const int q = level % 3;
    shift = q == 0 ? 20 : (q == 1 ? 8 : 0);
    bits = q == 2 ? 8 : 12;
}

__global__ void hm_digit_hist_kernel(const uint4* __restrict__ ent, uint32_t m, Prefix pf, int level, uint32_t* __restrict__ hist)
{
    __shared__ uint32_t lh[HM_DIGIT_BINS];
    for (int t = threadIdx.x; t < HM_DIGIT_BINS; t += blockDim.x) lh[t] = 0;
    __syncthreads();
    int word, shift, bits;
    hm_digit_pos(level, word, shift, bits);
    for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < m; t += gridDim.x * blockDim.x) {
        const uint4 en = ent[t];
        const uint32_t k[3] = {en.x, en.y, en.z};
        if ((k[0] & pf.mask[0]) == pf.val[0] && (k[1] & pf.mask[1]) == pf.val[1] && (k[2] & pf.mask[2]) == pf.val[2])
            atomicAdd(&lh[(k[word] >> shift) & ((1u << bits) - 1u)], 1u);
    }
    __syncthreads();
    for (int t = threadIdx.x; t < HM_DIGIT_BINS; t += blockDim.x)
        if (lh[t]) atomicAdd(&hist[t], lh[t]);
}

// keep entries whose masked key <= prefix (lexicographic)
__global__ void hm_compact_prefix_kernel(const uint4* __restrict__ ent, uint32_t m, Prefix pf, uint4* __restrict__ out,
                                         uint32_t* __restrict__ out_count, uint32_t out_cap)
{
    for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < m; t += gridDim.x * blockDim.x) {
        const uint4 en = ent[t];
        const uint32_t a0 = en.x & pf.mask[0], a1 = en.y & pf.mask[1], a2 = en.z & pf.mask[2];
        const bool le = !hm_key_less(pf.val[0], pf.val[1], pf.val[2], a0, a1, a2);
        if (le) {
            const uint32_t s = atomicAdd(out_count, 1u);
            if (s < out_cap) out[s] = en;
        }
    }
}

// keep valid entries only (candidate listing)
__global__ void hm_compact_valid_kernel(const uint4* __restrict__ ent, uint32_t m, uint4* __restrict__ out,
                                        uint32_t* __restrict__ out_count, uint32_t out_cap)
{
    for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < m; t += gridDim.x * blockDim.x) {
        const uint4 en = ent[t];
        if (en.x != 0xffffffffu) {
            const uint32_t s = atomicAdd(out_count, 1u);
            if (s < out_cap) out[s] = en;
        }
    }
}

// ---- exact order of m unique keys: sorted chunks in LDS, then rank = sum of lower bounds over the chunks ----
#define HM_SORT_CHUNK 2048
// bitonic sort of HM_SORT_CHUNK keys per block (padding = all ones), 1024 threads
__device__ __forceinline__ void hm_chunk_sort_body(const uint4* __restrict__ ent, uint32_t m, uint4* __restrict__ out)
{
    __shared__ uint4 keys[HM_SORT_CHUNK];
    const uint32_t base = blockIdx.x * HM_SORT_CHUNK;
    for (uint32_t q = threadIdx.x; q < HM_SORT_CHUNK; q += 1024) {
        const uint32_t idx = base + q;
        keys[q] = idx < m ? ent[idx] : make_uint4(0xffffffffu, 0xffffffffu, 0xffffffffu, 0);
    }
    __syncthreads();
    for (uint32_t k = 2; k <= HM_SORT_CHUNK; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            const uint32_t t = threadIdx.x;
            const uint32_t lo = ((t & ~(j - 1)) << 1) | (t & (j - 1));   // index with bit j clear
            const uint32_t hi = lo | j;
            const bool up = (lo & k) == 0;
            const uint4 x = keys[lo], y = keys[hi];
            const bool swap = up ? hm_key_less(y.x, y.y, y.z, x.x, x.y, x.z) : hm_key_less(x.x, x.y, x.z, y.x, y.y, y.z);
            if (swap) { keys[lo] = y; keys[hi] = x; }
            __syncthreads();
        }
    }
    for (uint32_t q = threadIdx.x; q < HM_SORT_CHUNK; q += 1024) out[base + q] = keys[q];
}

// rank of every key = its index in its own chunk + the lower bounds in all other chunks; rank < k -> out[rank]
__device__ __forceinline__ void hm_rank_merge_body(const uint4* __restrict__ chunks, uint32_t nchunks, uint4* __restrict__ out, uint32_t k)
{
    __shared__ uint4 tile[HM_SORT_CHUNK];
    const uint32_t mine = blockIdx.x * 256 + threadIdx.x;              // position in the chunked array
    const uint32_t total = nchunks * HM_SORT_CHUNK;
    uint4 me = make_uint4(0xffffffffu, 0xffffffffu, 0xffffffffu, 0);
    if (mine < total) me = chunks[mine];
    const uint32_t my_chunk = mine / HM_SORT_CHUNK;
    uint32_t rank = mine % HM_SORT_CHUNK;                              // keys of the own chunk in front of this one
    for (uint32_t c = 0; c < nchunks; ++c) {
        __syncthreads();
        for (uint32_t q = threadIdx.x; q < HM_SORT_CHUNK; q += 256) tile[q] = chunks[c * HM_SORT_CHUNK + q];
        __syncthreads();
        if (c == my_chunk) continue;
        uint32_t lo = 0, hi = HM_SORT_CHUNK;                           // first index whose key is not less than mine
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            const uint4 o = tile[mid];
            if (hm_key_less(o.x, o.y, o.z, me.x, me.y, me.z)) lo = mid + 1; else hi = mid;
        }
        rank += lo;
    }
    if (mine < total && me.y != 0xffffffffu && rank < k) out[rank] = me;
}

__global__ __launch_bounds__(1024) void hm_chunk_sort_kernel(const uint4* __restrict__ ent, uint32_t m, uint4* __restrict__ out)
{
    hm_chunk_sort_body(ent, m, out);
}

__global__ __launch_bounds__(256) void hm_rank_merge_kernel(const uint4* __restrict__ chunks, uint32_t nchunks, uint4* __restrict__ out, uint32_t k)
{
    hm_rank_merge_body(chunks, nchunks, out, k);
}

// ---- the same two kernels with the entry count taken from device memory (m = min(*m_dev, cap) + m_add): the
// incremental refresh enqueues its whole chain -- scan, distances, union with the previous list, sort, read-back -- and
// synchronises once; grids are sized for the most it accepts (HM_RANK_LIMIT entries), surplus blocks leave at once ----
__device__ __forceinline__ uint32_t hm_dev_count(const unsigned long long* m_dev, uint32_t cap, uint32_t m_add)
{
    const unsigned long long v = *m_dev;
    return (uint32_t)(v > (unsigned long long)cap ? cap : v) + m_add;
}

__global__ __launch_bounds__(256) void hm_append_prev_kernel(uint4* __restrict__ ent, const unsigned long long* __restrict__ m_dev, uint32_t cap,
                                                             const uint4* __restrict__ prev, uint32_t k)
{
    const unsigned long long m_new = *m_dev;
    if (m_new + (unsigned long long)k > (unsigned long long)cap) return;          // the host sees the count and falls back
    for (uint32_t t = blockIdx.x * 256 + threadIdx.x; t < k; t += gridDim.x * 256) ent[(uint32_t)m_new + t] = prev[t];
}

__global__ __launch_bounds__(1024) void hm_chunk_sort_dev_kernel(const uint4* __restrict__ ent, const unsigned long long* __restrict__ m_dev,
                                                                 uint32_t cap, uint32_t m_add, uint4* __restrict__ out)
{
    const uint32_t m = hm_dev_count(m_dev, cap, m_add);
    if (blockIdx.x * HM_SORT_CHUNK >= m) return;                                  // block-uniform
    hm_chunk_sort_body(ent, m, out);
}

__global__ __launch_bounds__(256) void hm_rank_merge_dev_kernel(const uint4* __restrict__ chunks, const unsigned long long* __restrict__ m_dev,
                                                                uint32_t cap, uint32_t m_add, uint4* __restrict__ out, uint32_t k)
{
    const uint32_t nchunks = (hm_dev_count(m_dev, cap, m_add) + HM_SORT_CHUNK - 1) / HM_SORT_CHUNK;
    if (blockIdx.x * 256 >= nchunks * HM_SORT_CHUNK) return;                      // block-uniform
    hm_rank_merge_body(chunks, nchunks, out, k);
}

// exact selection of the k smallest keys among m entries of `src` (keys unique; invalid = 0xffffffff)
// result in e->sorted.  `other` is scratch of the same capacity.
int hm_select_sorted(hm_engine* e, uint4* src, uint4* other, uint32_t m, uint32_t k, hipStream_t s)
{
    if (k == 0 || m == 0) return HM_OK;
    if (k > e->sorted_cap) return hm_fail(e, HM_E_CAPACITY, "top-k: k exceeds the engine's sorted capacity (65536)");
    uint4* cur = src;
    uint4* spare = other;
    uint32_t mcur = m;
    // up to HM_RANK_LIMIT entries are sorted outright: two more kernels cost less than the two host round trips of a
    // narrowing level (measured on the refresh of the fast tokenizer: ~100 us against ~30 us)
    const uint32_t rank_limit = HM_RANK_LIMIT;
    if (mcur > rank_limit) {
        // radix narrowing on the 96-bit key, 12/12/8-bit digits per word
        Prefix pf; memset(&pf, 0, sizeof(pf));
        uint32_t below = 0;      // keys strictly below the prefix: certainly selected
        int level = 0;
        for (; level < 9; ++level) {
            int word, shift, bits;
            hm_digit_pos(level, word, shift, bits);
            HM_HIP(hipMemsetAsync(e->d_hist, 0, sizeof(uint32_t) * HM_DIGIT_BINS, s));
            hipLaunchKernelGGL(hm_digit_hist_kernel, dim3(1024), dim3(256), 0, s, cur, mcur, pf, level, e->d_hist);
            HM_HIP(hipGetLastError());
            HM_HIP(hipMemcpyAsync(e->h->hist, e->d_hist, sizeof(uint32_t) * HM_DIGIT_BINS, hipMemcpyDeviceToHost, s));
            HM_HIP(hipStreamSynchronize(s));
            const uint32_t nb = 1u << bits;
            const BinHit<uint32_t> hit = hm_first_bin<uint32_t>(e->h->hist, nb, below, k);
            const uint32_t dsel = hit.bin < 0 ? nb - 1 : (uint32_t)hit.bin;
            below = hit.below;
            pf.val[word] |= dsel << shift;
            pf.mask[word] |= ((1u << bits) - 1u) << shift;
            if (below + hit.in <= rank_limit) break;
        }
        HM_HIP(hipMemsetAsync(e->d_ctr + HM_CTR_COMPACTED, 0, sizeof(uint32_t), s));
        hipLaunchKernelGGL(hm_compact_prefix_kernel, dim3(1024), dim3(256), 0, s, cur, mcur, pf, other, e->d_ctr + HM_CTR_COMPACTED, e->ent_cap);
        HM_HIP(hipGetLastError());
        HM_HIP(hipMemcpyAsync(&e->h->ctr[HM_CTR_COMPACTED], e->d_ctr + HM_CTR_COMPACTED, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        HM_HIP(hipStreamSynchronize(s));
        cur = other;
        spare = src;
        mcur = e->h->ctr[HM_CTR_COMPACTED];
        if (mcur > 4u * HM_RANK_LIMIT) return hm_fail(e, HM_E_CAPACITY, "top-k: radix narrowing did not converge");
    }
    // (the scratch holds at least 65536 entries and mcur <= 4 * HM_RANK_LIMIT only when the buffers are 2^24 entries)
    const uint32_t nchunks = (mcur + HM_SORT_CHUNK - 1) / HM_SORT_CHUNK;
    if ((uint64_t)nchunks * HM_SORT_CHUNK > e->ent_cap) return hm_fail(e, HM_E_CAPACITY, "top-k: sort scratch too small");
    hipLaunchKernelGGL(hm_chunk_sort_kernel, dim3(nchunks), dim3(1024), 0, s, cur, mcur, spare);
    HM_HIP(hipGetLastError());
    hipLaunchKernelGGL(hm_rank_merge_kernel, dim3(nchunks * (HM_SORT_CHUNK / 256)), dim3(256), 0, s, spare, nchunks, e->sorted, k);
    HM_HIP(hipGetLastError());
    return HM_OK;
}

// Choose an emission cut from sampled histograms of bits(u') so that roughly `target` entries
// (and certainly not more than the buffer holds) are emitted.  Pure performance heuristic: the
// caller verifies the outcome (complete-region count) and widens the cut when it was too tight.
// The passes are issued here; what each histogram means is decided by hm_zoom_decide (hm_cut_plan.h).
static int hm_estimate_cut(hm_engine* e, ScanArgs a, dim3 grid, int64_t target, uint32_t* cut_bits, int* tie_imax,
                           hipStream_t s)
{
    *cut_bits = HM_CUT_ALL;
    *tie_imax = HM_TIE_ALL_ROWS;
    const int64_t pairs = hm_pairs_in_range(a.n, a.row_begin, a.row_end);
    if (pairs <= (int64_t)e->ent_cap / 2) return HM_OK;           // everything fits: emit all candidates
    union { uint32_t u; float f; } hi; hi.f = a.u_hi;
    CutWindow w = {HM_CUT_ONE, hi.f == INFINITY ? 0x7f800000u : hi.u, 0.0};
    const int stride = hm_estimate_stride(pairs);
    for (int zoom = 0; zoom < 6; ++zoom) {
        a.hist_lo = w.lo_bits;
        a.hist_shift = hm_zoom_shift(w, HM_HIST_BINS);
        a.sample_stride = stride;
        HM_HIP(hipMemsetAsync(e->d_hist, 0, sizeof(uint32_t) * HM_DIGIT_BINS, s));
        HM_HIP(hm_launch_scan(e, HM_MODE_HIST, a, grid, s));
        HM_HIP(hipMemcpyAsync(e->h->hist, e->d_hist, sizeof(uint32_t) * HM_HIST_BINS, hipMemcpyDeviceToHost, s));
        HM_HIP(hipStreamSynchronize(s));
        e->tm.count_pass();
        const ZoomDecision z = hm_zoom_decide(e->h->hist, HM_HIST_BINS, stride, w, target, e->ent_cap, a.n, a.row_begin, a.row_end);
        if (z.kind != ZoomDecision::ZOOM) {
            *cut_bits = z.cut_bits;
            *tie_imax = z.tie_imax;
            return HM_OK;
        }
        w = z.window;
    }
    return HM_OK;
}

// One prefilter form of the search: the passes CutSearch (hm_cut_plan.h) asks for, until it is done or gives up.
// res->total: the exact number of candidates, or -1 when want_count is false and at least k exist (not counted)
static int hm_topk_core_form(hm_engine* e, float c, float thr, int64_t k, int64_t row_begin, int64_t row_end, bool list_all,
                             bool want_count, int64_t n_limit, TopkResult* res, hipStream_t s)
{
    *res = TopkResult{nullptr, 0u, 0, 0};
    e->tm.begin_search();
    const Bounds b = hm_bounds(thr, c);
    ScanArgs a; dim3 grid;
    if (b.none || e->n < 2 || !hm_prepare_scan(e, b, row_begin, row_end, a, grid, n_limit)) return HM_OK;
    const float sqrt_c = sqrtf(c);
    a.count_sure = (want_count || list_all) ? 1 : 0;
    CutSearchInput in = {k, list_all, a.count_sure != 0, e->ent_cap, a.row_begin, a.row_end, false, 0u};
    if (!list_all && k != 0) {
        const SearchState::Cut& cut = e->st.cut();
        in.have_cut = a.row_begin == 0 && a.row_end == e->n - 1 && cut.have && cut.k >= k && cut.c == c && cut.bits > HM_CUT_ONE;
        if (in.have_cut) in.cut_bits = e->st.consume_debug_cut() ? cut.bits : cut.bits + hm_tie_slack(cut.bits);
    }
    CutSearch plan(in);
    PassOutcome o = {};
    for (;;) {
        const CutAction act = plan.next();
        if (act.kind == CutAction::FAIL) return hm_fail(e, act.status, act.message);
        if (act.kind == CutAction::DONE) break;
        if (act.kind == CutAction::ESTIMATE) {
            uint32_t cut_bits; int tie_imax;
            const int rc = hm_estimate_cut(e, a, grid, act.target, &cut_bits, &tie_imax, s);
            if (rc) return rc;
            plan.estimated(cut_bits, tie_imax);
            continue;
        }
        a.cut_bits = act.cut_bits;
        a.tie_imax = act.tie_imax;
        HM_HIP(hipMemsetAsync(e->d_ctr, 0, sizeof(uint32_t) * 8, s));
        HM_HIP(hipMemsetAsync(e->d_ctr64, 0, sizeof(unsigned long long) * 4, s));
        HM_HIP(hm_launch_scan(e, HM_MODE_TOPK, a, grid, s, e->tm.own().ev0, e->tm.own().ev1));
        hipLaunchKernelGGL(hm_post_distance_kernel, dim3(1024), dim3(256), 0, s, e->ent, e->d_ctr64, e->ent_cap, e->img, e->RS, e->d,
                           e->sign_mode, sqrt_c, thr, a.cut_bits, a.tie_imax, e->d_ctr + HM_CTR_POST_FIRST);
        HM_HIP(hipGetLastError());
        HM_HIP(hipMemcpyAsync(e->h->ctr, e->d_ctr, sizeof(uint32_t) * 8, hipMemcpyDeviceToHost, s));
        HM_HIP(hipMemcpyAsync(e->h->ctr64, e->d_ctr64, sizeof(unsigned long long) * 4, hipMemcpyDeviceToHost, s));
        HM_HIP(hipStreamSynchronize(s));
        o.emitted = e->h->ctr64[HM_CTR64_EMITTED];
        o.valid = e->h->ctr[HM_CTR_VALID];
        o.borderline = e->h->ctr[HM_CTR_BORDERLINE];
        o.sure = (int64_t)e->h->ctr64[HM_CTR64_SURE];
        o.complete = e->h->ctr[HM_CTR_COMPLETE];
        o.margin_violations = e->h->ctr[HM_CTR_MARGIN_BAD];
        e->tm.add_pass(hm_pairs_in_range(a.n, a.row_begin, a.row_end), (int64_t)o.emitted);
        plan.scanned(o);
    }
    *res = TopkResult{e->ent, (uint32_t)o.emitted, plan.next().valid, plan.next().total};      // (done: the last pass fitted the buffer)
    return HM_OK;
}

// The bf16 prefilter's margin (delta ~ 0.004 * max||x_s||^2 in u) makes a shell of undecided pairs around the
// threshold; every one of them has to be emitted to be decided exactly.  With a threshold inside the bulk of the
// distance distribution that shell alone can exceed the emission buffer: the search then runs again with the fp32
// prefilter, whose shell is ~100x thinner.
int hm_topk_core(hm_engine* e, float c, float thr, int64_t k, int64_t row_begin, int64_t row_end, bool list_all, bool want_count,
                 int64_t n_limit, TopkResult* res, hipStream_t s)
{
    const bool had_bf16 = hm_use_bf16(e);
    int rc = HM_E_CAPACITY;
    const bool exact_known = !list_all && (e->force_exact || e->st.straight_to_exact(thr));      // (remembered per table, like the fp32 fallback)
    if (!exact_known && !(had_bf16 && e->st.straight_to_f32(thr)))
        rc = hm_topk_core_form(e, c, thr, k, row_begin, row_end, list_all, want_count, n_limit, res, s);
    if (!exact_known && rc == HM_E_CAPACITY && had_bf16 && !e->force_f32) {
        {
            const HmScopedSet<bool> f32(e->force_f32, true);
            rc = hm_topk_core_form(e, c, thr, k, row_begin, row_end, list_all, want_count, n_limit, res, s);
        }
        if (rc == HM_OK) e->st.remember_f32(thr);
    }
    if (rc == HM_E_CAPACITY && !list_all) {
        // No emission cut fits the buffer in either prefilter form (a table whose distances sit within a few hundred ulps of
        // u = 1): every pair evaluated exactly, selection by counting (hm_exact.hip).  Slow, and always an answer.
        rc = hm_topk_exact(e, c, thr, k, row_begin, row_end, n_limit, res, s);
        if (rc == HM_OK) e->st.remember_exact(thr);
    }
    return rc;
}

// ------------------------------------------------------------------------------------------------
// C ABI: searches
// ------------------------------------------------------------------------------------------------
static const MergeFuse kNoMerge = {nullptr, 0, 0, 0.f, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0u};

extern "C" int hm_pairwise_argmin_dev(hm_engine* e, float c, float thr, int64_t row_begin, int64_t row_end, uint32_t* rec_dev,
                                      void* stream)
{
    if (!e) return hm_fail(nullptr, HM_E_ARG, "hm_pairwise_argmin_dev: engine is NULL");
    if (!rec_dev) return hm_fail(e, HM_E_ARG, "hm_pairwise_argmin_dev: NULL record pointer");
    if (!(c > 0.0f)) return hm_fail(e, HM_E_ARG, "hm_pairwise_argmin_dev: curvature must be > 0");
    hipStream_t s = (hipStream_t)stream;
    HM_HIP(hipSetDevice(e->device));
    e->tm.flush_pending();
    const Bounds b = hm_bounds(thr, c);
    ScanArgs a; dim3 grid;
    const int64_t req_rb = std::max<int64_t>(row_begin, 0), req_re = (row_end < 0 || row_end >= e->n) ? -1 : row_end;
    const bool skip_init = e->st.take_arm(req_rb, req_re);
    if (b.none || e->n < 2 || !hm_prepare_scan(e, b, row_begin, row_end, a, grid, -1, 0, HM_MODE_ARGMIN)) {
        HM_HIP(hipMemsetAsync(rec_dev, 0, sizeof(ArgminRec), s));        // found = 0
        return HM_OK;
    }
    if (!skip_init) {
        int rc0 = hm_launch_seed_init(e, a, s);
        if (rc0) return rc0;
    }
    MergeFuse mf = kNoMerge;
    if (e->shard_loop) {                          // inside hm_shard_loop_begin .. _end: a stopped loop skips its searches
        a.stop = &e->d_loop->stop;
        mf.loop = e->d_loop;
    }
    // (inside a sharded loop only the batch's first search carries the engine's own timing events: reading them back at the
    // next call is a host wait, and the point of the loop is that the host runs ahead of the device; the in-library loop in
    // its measurement mode opens every step's own pair -- ScanTiming::open_step, read after the batch)
    const HmEvPair step = e->tm.step_pair();
    const bool timed = !step.ev0 && (!e->shard_loop || e->n == e->shard_n0);
    const HmEvPair ev = timed ? e->tm.own() : step;
    HM_HIP(hm_launch_scan(e, HM_MODE_ARGMIN, a, grid, s, ev.ev0, ev.ev1));
    int rc = hm_launch_argmin_tail(e, a, sqrtf(c), thr, reinterpret_cast<ArgminRec*>(rec_dev), true, (int)req_rb,
                                   req_re < 0 ? 0x7fffffff : (int)std::min<int64_t>(req_re, 0x7fffffff), true, mf, s);
    if (rc) return rc;
    // Armed optimistically: the host does not see this record.  Should the search have overflowed (found = 2, the
    // kernel then arms nothing), the next search of this range starts on the stale counters, reports found = 2 as
    // well, and its caller takes the bounded host path -- slower, never wrong.
    e->st.arm(req_rb, req_re);
    if (timed) e->tm.note_pending(hm_pairs_in_range(e->n, a.row_begin, a.row_end));
    return HM_OK;
}

extern "C" int hm_pairwise_argmin(hm_engine* e, float c, float thr, int64_t row_begin, int64_t row_end, float* d, int32_t* i,
                                  int32_t* j, int32_t* found, void* stream)
{
    if (!e) return hm_fail(nullptr, HM_E_ARG, "hm_pairwise_argmin: engine is NULL");
    if (!d || !i || !j || !found) return hm_fail(e, HM_E_ARG, "hm_pairwise_argmin: NULL output pointer");
    if (!(c > 0.0f)) return hm_fail(e, HM_E_ARG, "hm_pairwise_argmin: curvature must be > 0");
    hipStream_t s = (hipStream_t)stream;
    HM_HIP(hipSetDevice(e->device));
    *found = 0; *d = 0.f; *i = -1; *j = -1;
    e->tm.begin_search();
    const Bounds b = hm_bounds(thr, c);
    ScanArgs a; dim3 grid;
    // the range as asked, "to the end" normalised (the table grows between searches): what "same range" means
    const int64_t req_rb = std::max<int64_t>(row_begin, 0), req_re = (row_end < 0 || row_end >= e->n) ? -1 : row_end;
    const bool skip_init = e->st.take_arm(req_rb, req_re);
    if (b.none || e->n < 2 || !hm_prepare_scan(e, b, row_begin, row_end, a, grid, -1, e->argmin_col_begin, HM_MODE_ARGMIN)) return HM_OK;
    if (e->force_exact || e->st.straight_to_exact(thr)) {
        // this table's searches are known to end in the prefilter-free path (hm_exact.hip): no scan attempts first
        float d1 = 0.f; int32_t i1 = -1, j1 = -1; int64_t n1 = 0, cnt1 = 0;
        const int rc2 = hm_pairwise_topk_nocount(e, c, thr, 1, row_begin, row_end, &d1, &i1, &j1, &n1, &cnt1, stream);
        if (rc2) return rc2;
        if (n1 > 0) { *found = 1; *d = d1; *i = i1; *j = j1; }
        return HM_OK;
    }
    const float sqrt_c = sqrtf(c);
    const int arm_re = req_re < 0 ? 0x7fffffff : (int)std::min<int64_t>(req_re, 0x7fffffff);
    for (int pass = 0; pass < 2; ++pass) {
        // pass 1 (after an overflow) keeps the final running key of pass 0: every wave then starts
        // with the tight bound and only the band around the minimum is emitted
        if (pass == 0) {
            if (!skip_init) {           // else: the previous search of this range left counters and key armed
                int rc0 = hm_launch_seed_init(e, a, s);
                if (rc0) return rc0;
            }
        } else {
            HM_HIP(hipMemsetAsync(e->d_ctr64 + 2, 0, sizeof(unsigned long long), s));     // emitted = 0, running key kept
        }
        HM_HIP(hm_launch_scan(e, HM_MODE_ARGMIN, a, grid, s, e->tm.own().ev0, e->tm.own().ev1));
        int rc = hm_launch_argmin_tail(e, a, sqrt_c, thr, e->d_rec, true, (int)req_rb, arm_re, true, kNoMerge, s);
        if (rc) return rc;
        // record + emitted count (the slot behind the record) in one copy
        HM_HIP(hipMemcpyAsync(e->h->rec2, e->d_rec, 2 * sizeof(ArgminRec), hipMemcpyDeviceToHost, s));
        HM_HIP(hipStreamSynchronize(s));
        e->h->rec = e->h->rec2[0];
        const uint64_t emitted = (uint64_t)e->h->rec2[1].found | ((uint64_t)e->h->rec2[1].dbits << 32);
        e->tm.add_pass(hm_pairs_in_range(e->n, a.row_begin, a.row_end), (int64_t)emitted);
        if (emitted <= e->ent_cap) break;
        // overflow: the running key is the exact minimum over all published waves; rerun bounded by it
        if (pass == 1) {
            if (a.bf16 && !e->force_f32) {      // the bf16 margin's shell around the bound is too populated: fp32 prefilter
                const HmScopedSet<bool> f32(e->force_f32, true);
                return hm_pairwise_argmin(e, c, thr, row_begin, row_end, d, i, j, found, stream);
            }
            // Still too many pairs inside the running key's slack band (a very dense table: the band is 1024 ulps of
            // u, which near u = 1 spans every distance below ~0.016): take the first entry of an exact top-1 search,
            // whose emission cut is found by histogram zooming instead.
            float d1 = 0.f; int32_t i1 = -1, j1 = -1; int64_t n1 = 0, cnt1 = 0;
            const int rc2 = hm_pairwise_topk(e, c, thr, 1, row_begin, row_end, &d1, &i1, &j1, &n1, &cnt1, stream);
            if (rc2) return rc2;
            if (n1 > 0) { *found = 1; *d = d1; *i = i1; *j = j1; }
            return HM_OK;
        }
    }
    if (e->h->rec.found == 1u) {
        union { uint32_t u; float f; } cv; cv.u = e->h->rec.dbits;
        *found = 1; *d = cv.f; *i = (int32_t)e->h->rec.i; *j = (int32_t)e->h->rec.j;
    }
    if (e->h->rec.found != 2u) e->st.arm(req_rb, req_re);
    return HM_OK;
}

// Incremental refresh (rows are only ever appended).  The ordered list S[:k] of the previous
// whole-table search is still the k smallest of the pairs among the rows it saw; the k smallest of the grown table
// are therefore the k smallest of S[:k] + the pairs that involve a NEW row (j >= prev_n).  Only the last column
// tile(s) are scanned (cut = largest u' of S[:k], so every new pair that could enter is emitted) and the two lists
// are merged by the exact selection.  Preconditions checked by the callers (below); the exact total is not produced here.
static bool hm_topk_incremental_ok(const hm_engine* e, float c, float thr, int64_t k)
{
    return e->incremental_topk && e->st.incremental_ok(e->n, c, thr, k);
}

// entries the device-side sort takes: the pairs of a few hundred new rows under the previous list's cut are often several
// ten thousand; 64 chunks keep the rank merge around 0.1 ms, beyond that the full search's radix narrowing is used
static uint32_t hm_topk_incremental_limit(const hm_engine* e) { return std::min<uint32_t>(e->ent_cap, 64u * HM_SORT_CHUNK); }

// everything of the incremental refresh up to the read-back, enqueued; no host wait
static int hm_topk_incremental_enqueue(hm_engine* e, float c, float thr, int64_t k, hipStream_t s)
{
    e->tm.begin_search();
    const Bounds b = hm_bounds(thr, c);
    const uint32_t lim = hm_topk_incremental_limit(e);
    if ((uint64_t)k + 1 > lim) return HM_E_CAPACITY;
    HM_HIP(hipMemsetAsync(e->d_ctr, 0, sizeof(uint32_t) * 8, s));
    HM_HIP(hipMemsetAsync(e->d_ctr64, 0, sizeof(unsigned long long) * 4, s));
    if (e->n > e->st.prev().n) {
        ScanArgs a; dim3 grid;
        if (!hm_prepare_scan(e, b, 0, -1, a, grid, -1, e->st.prev().n)) return hm_fail(e, HM_E_STATE, "incremental refresh: empty scan");
        a.count_sure = 0;
        a.cut_bits = e->st.cut().bits + hm_tie_slack(e->st.cut().bits);
        a.tie_imax = 0x7fffffff;
        HM_HIP(hm_launch_scan(e, HM_MODE_TOPK, a, grid, s));
        hipLaunchKernelGGL(hm_post_distance_kernel, dim3(256), dim3(256), 0, s, e->ent, e->d_ctr64, e->ent_cap, e->img, e->RS, e->d,
                           e->sign_mode, sqrtf(c), thr, a.cut_bits, a.tie_imax, e->d_ctr + HM_CTR_POST_FIRST);
        HM_HIP(hipGetLastError());
        e->tm.count_pass();
    }
    // union with the previous list (appended behind the new entries; invalid new entries carry all-ones keys), sorted
    // outright: the count of new entries stays on the device
    const unsigned long long* m_dev = e->d_ctr64 + HM_CTR64_EMITTED;
    const uint32_t room = lim - (uint32_t)k;                                       // new entries the sort can take
    hipLaunchKernelGGL(hm_append_prev_kernel, dim3(64), dim3(256), 0, s, e->ent, m_dev, lim, e->d_prev, (uint32_t)k);
    const uint32_t max_chunks = (lim + HM_SORT_CHUNK - 1) / HM_SORT_CHUNK;
    hipLaunchKernelGGL(hm_chunk_sort_dev_kernel, dim3(max_chunks), dim3(1024), 0, s, e->ent, m_dev, room, (uint32_t)k, e->ent2);
    hipLaunchKernelGGL(hm_rank_merge_dev_kernel, dim3(max_chunks * (HM_SORT_CHUNK / 256)), dim3(256), 0, s, e->ent2, m_dev, room, (uint32_t)k,
                       e->sorted, (uint32_t)k);
    HM_HIP(hipGetLastError());
    HM_HIP(hipMemcpyAsync(e->h->ctr64, e->d_ctr64, sizeof(unsigned long long) * 4, hipMemcpyDeviceToHost, s));
    HM_HIP(hipMemcpyAsync(e->h_sorted, e->sorted, sizeof(uint4) * (size_t)k, hipMemcpyDeviceToHost, s));
    return HM_OK;
}

// the one synchronisation; HM_E_CAPACITY: too many new entries for the device-side sort (the caller runs the full search)
static int hm_topk_incremental_finish(hm_engine* e, int64_t k, hipStream_t s, uint32_t* kk_out)
{
    *kk_out = 0;
    HM_HIP(hipStreamSynchronize(s));
    const unsigned long long emitted = e->h->ctr64[HM_CTR64_EMITTED];          // (the read-back of this chain itself)
    e->tm.set_emitted((int64_t)emitted);
    if (emitted > (unsigned long long)(hm_topk_incremental_limit(e) - (uint32_t)k)) return HM_E_CAPACITY;
    *kk_out = (uint32_t)k;
    return HM_OK;
}

// entries {distance bits, i, j, .} -> the triples of the ABI
void hm_unpack_entries(const uint4* ent, int64_t n, float* d_out, int32_t* i_out, int32_t* j_out)
{
    for (int64_t t = 0; t < n; ++t) {
        union { uint32_t u; float f; } cv; cv.u = ent[t].x;
        d_out[t] = cv.f; i_out[t] = (int32_t)ent[t].y; j_out[t] = (int32_t)ent[t].z;
    }
}

// host side of a finished top-k search whose ordered list sits in e->h_sorted: outputs and the state the next refresh uses
static void hm_topk_publish(hm_engine* e, uint32_t kk, int64_t k, float c, float thr, bool keep, float* d_out, int32_t* i_out, int32_t* j_out,
                            int64_t* n_out)
{
    hm_unpack_entries(e->h_sorted, kk, d_out, i_out, j_out);
    uint32_t mx = 0;
    for (uint32_t t = 0; t < kk; ++t) mx = std::max(mx, e->h_sorted[t].w);     // entries are ordered by distance, not by u': the max u' bits of the selection
    *n_out = kk;
    // remember the largest u' of the selection: while rows are only appended, the k-th smallest key can
    // only move down, so this cut (+ tie slack) is a guaranteed superset for the next refresh
    e->st.publish(keep, mx, k, c, e->n, thr);
}

// common body of hm_pairwise_topk / hm_pairwise_topk_nocount
static int hm_topk_impl(hm_engine* e, float c, float thr, int64_t k, int64_t row_begin, int64_t row_end, bool want_count,
                        float* d_out, int32_t* i_out, int32_t* j_out, int64_t* n_out, int64_t* count, void* stream)
{
    if (!e) return hm_fail(nullptr, HM_E_ARG, "hm_pairwise_topk: engine is NULL");
    e->st.disarm();                                // (before the argument checks: a refused top-k disarms too)
    if (!n_out || !count || k < 0 || (k > 0 && (!d_out || !i_out || !j_out)))
        return hm_fail(e, HM_E_ARG, "hm_pairwise_topk: bad output pointers / k");
    if (!(c > 0.0f)) return hm_fail(e, HM_E_ARG, "hm_pairwise_topk: curvature must be > 0");
    if (k > (int64_t)e->sorted_cap) return hm_fail(e, HM_E_CAPACITY, "hm_pairwise_topk: k > 65536");
    hipStream_t s = (hipStream_t)stream;
    HM_HIP(hipSetDevice(e->device));
    *n_out = 0; *count = 0;
    const bool whole = row_begin <= 0 && (row_end < 0 || row_end >= e->n - 1);
    uint32_t kk = 0;
    bool done = false;
    if (!want_count && whole && hm_topk_incremental_ok(e, c, thr, k)) {
        int rc = hm_topk_incremental_enqueue(e, c, thr, k, s);
        if (rc == HM_OK) rc = hm_topk_incremental_finish(e, k, s, &kk);
        if (rc == HM_OK) { done = true; *count = -1; }
        else if (rc != HM_E_CAPACITY) return rc;
    }
    if (!done) {
        TopkResult res;
        int rc = hm_topk_core(e, c, thr, k, row_begin, row_end, false, want_count || k == 0, -1, &res, s);
        if (rc) return rc;
        // the uncounted form answers -1 once k candidates exist (include/hypmerge.h), also where a small table's search
        // emitted every candidate and so knows their number
        *count = (!want_count && k > 0 && res.total >= k) ? -1 : res.total;
        kk = (uint32_t)std::min<int64_t>(k, res.valid);
        if (kk == 0 || !res.ent) { e->st.drop_prev(); return HM_OK; }
        rc = hm_select_sorted(e, res.ent, e->ent2, res.m, kk, s);
        if (rc) return rc;
    }
    const bool keep = (kk == k && whole);
    if (keep) HM_HIP(hipMemcpyAsync(e->d_prev, e->sorted, sizeof(uint4) * kk, hipMemcpyDeviceToDevice, s));    // (stream-ordered: no wait needed for it)
    if (!done) {                                   // (the incremental refresh has read its list back already)
        HM_HIP(hipMemcpyAsync(e->h_sorted, e->sorted, sizeof(uint4) * kk, hipMemcpyDeviceToHost, s));
        HM_HIP(hipStreamSynchronize(s));
    }
    hm_topk_publish(e, kk, k, c, thr, keep, d_out, i_out, j_out, n_out);
    return HM_OK;
}

extern "C" int hm_pairwise_topk(hm_engine* e, float c, float thr, int64_t k, int64_t row_begin, int64_t row_end, float* d_out,
                                int32_t* i_out, int32_t* j_out, int64_t* n_out, int64_t* count, void* stream)
{
    return hm_topk_impl(e, c, thr, k, row_begin, row_end, true, d_out, i_out, j_out, n_out, count, stream);
}

extern "C" int hm_pairwise_topk_nocount(hm_engine* e, float c, float thr, int64_t k, int64_t row_begin, int64_t row_end,
                                        float* d_out, int32_t* i_out, int32_t* j_out, int64_t* n_out, int64_t* count, void* stream)
{
    return hm_topk_impl(e, c, thr, k, row_begin, row_end, false, d_out, i_out, j_out, n_out, count, stream);
}

// The refresh of a table whose rows were only appended since the last whole-table top-k search, in two halves: begin
// enqueues the whole chain and returns; end waits and delivers.  Between the two the engine must not be used.
extern "C" int hm_topk_refresh_begin(hm_engine* e, float c, float thr, int64_t k, void* stream)
{
    if (!e) return hm_fail(nullptr, HM_E_ARG, "hm_topk_refresh_begin: engine is NULL");
    if (e->st.refresh().pending) return hm_fail(e, HM_E_STATE, "hm_topk_refresh_begin: a refresh is already pending");
    if (!(c > 0.0f) || k <= 0 || k > (int64_t)e->sorted_cap) return hm_fail(e, HM_E_ARG, "hm_topk_refresh_begin: bad arguments");
    if (!hm_topk_incremental_ok(e, c, thr, k)) return HM_E_NA;                     // (no message: "not applicable" is an ordinary answer)
    HM_HIP(hipSetDevice(e->device));
    e->st.disarm();
    const int rc = hm_topk_incremental_enqueue(e, c, thr, k, (hipStream_t)stream);
    if (rc) return rc;
    e->st.refresh_begin(k, c, thr, stream);
    return HM_OK;
}

extern "C" int hm_topk_refresh_end(hm_engine* e, float* d_out, int32_t* i_out, int32_t* j_out, int64_t* n_out)
{
    if (!e) return hm_fail(nullptr, HM_E_ARG, "hm_topk_refresh_end: engine is NULL");
    if (!e->st.refresh().pending) return hm_fail(e, HM_E_STATE, "hm_topk_refresh_end: no refresh pending");
    if (!d_out || !i_out || !j_out || !n_out) return hm_fail(e, HM_E_ARG, "hm_topk_refresh_end: NULL output pointer");
    HM_HIP(hipSetDevice(e->device));
    e->st.refresh_end();                                                           // (first: an HM_E_CAPACITY answer ends it too)
    const SearchState::Refresh& r = e->st.refresh();
    hipStream_t s = (hipStream_t)r.stream;
    *n_out = 0;
    uint32_t kk = 0;
    const int rc = hm_topk_incremental_finish(e, r.k, s, &kk);
    if (rc) return rc;                                                             // HM_E_CAPACITY: run hm_pairwise_topk_nocount instead
    HM_HIP(hipMemcpyAsync(e->d_prev, e->sorted, sizeof(uint4) * kk, hipMemcpyDeviceToDevice, s));
    hm_topk_publish(e, kk, r.k, r.c, r.thr, true, d_out, i_out, j_out, n_out);
    return HM_OK;
}

extern "C" int hm_pairwise_count(hm_engine* e, float c, float thr, int64_t n_limit, int64_t* count, void* stream)
{
    if (!e) return hm_fail(nullptr, HM_E_ARG, "hm_pairwise_count: engine is NULL");
    if (!count || !(c > 0.0f)) return hm_fail(e, HM_E_ARG, "hm_pairwise_count: bad arguments");
    e->st.disarm();
    HM_HIP(hipSetDevice(e->device));
    *count = 0;
    TopkResult res;
    const SearchState::Cut cut = e->st.suspend_cut();     // a count does not disturb the cut prediction of the refreshes
    int rc = hm_topk_core(e, c, thr, 0, 0, -1, false, true, n_limit, &res, (hipStream_t)stream);
    e->st.restore_cut(cut);
    if (rc) return rc;
    *count = res.total;
    return HM_OK;
}

// valid entries of a listing -> host triples out[0, min(valid, room))
static int hm_copy_valid(hm_engine* e, const TopkResult& res, int64_t room, int32_t* i_out, int32_t* j_out, float* d_out,
                         int64_t* ncopy, hipStream_t s)
{
    HM_HIP(hipMemsetAsync(e->d_ctr + HM_CTR_COMPACTED, 0, sizeof(uint32_t), s));
    hipLaunchKernelGGL(hm_compact_valid_kernel, dim3(1024), dim3(256), 0, s, res.ent, res.m, e->ent2, e->d_ctr + HM_CTR_COMPACTED, e->ent_cap);
    HM_HIP(hipGetLastError());
    *ncopy = std::min<int64_t>(res.valid, room);
    std::vector<uint4> host((size_t)*ncopy);
    HM_HIP(hipMemcpyAsync(host.data(), e->ent2, sizeof(uint4) * (size_t)*ncopy, hipMemcpyDeviceToHost, s));
    HM_HIP(hipStreamSynchronize(s));
    hm_unpack_entries(host.data(), *ncopy, d_out, i_out, j_out);
    return HM_OK;
}

// More candidates in the range than the emission buffer holds (a tie flood: up to C(131 072, 2) > 2^32 pairs at distance 0):
// the exact number from a pure count, and min(cap, count) candidates listed slab of rows by slab of rows in row order.  A
// slab of at most ent_cap pairs cannot overflow the buffer; one row (< max_rows pairs) always fits it.
static int hm_candidates_by_rows(hm_engine* e, float c, float thr, int64_t row_begin, int64_t row_end, int64_t cap,
                                 int32_t* i_out, int32_t* j_out, float* d_out, int64_t* total, hipStream_t s)
{
    const int64_t n = e->n;
    const int64_t r0 = std::max<int64_t>(row_begin, 0), r1 = (row_end < 0 || row_end > n - 1) ? n - 1 : row_end;
    TopkResult res;
    int rc = hm_topk_core(e, c, thr, 0, r0, r1, false, true, -1, &res, s);
    if (rc) return rc;
    *total = res.total;
    const int64_t want = std::min<int64_t>(cap, res.total);
    int64_t got = 0;
    for (int64_t lo = r0; lo < r1 && got < want;) {
        int64_t hi = lo + 1, step = 1;
        while (step > 0) {                                   // largest hi <= r1 with at most ent_cap pairs in [lo, hi)
            if (hi + step <= r1 && hm_pairs_in_range(n, lo, hi + step) <= (int64_t)e->ent_cap) { hi += step; step *= 2; }
            else step /= 2;
        }
        rc = hm_topk_core(e, c, thr, 0, lo, hi, true, true, -1, &res, s);
        if (rc) return rc;
        if (res.ent && res.valid > 0) {
            int64_t ncopy = 0;
            rc = hm_copy_valid(e, res, want - got, i_out + got, j_out + got, d_out + got, &ncopy, s);
            if (rc) return rc;
            got += ncopy;
        }
        lo = hi;
    }
    if (got != want) return hm_fail(e, HM_E_STATE, "candidate listing: the row slabs disagree with the count");
    return HM_OK;
}

extern "C" int hm_pairwise_candidates(hm_engine* e, float c, float thr, int64_t row_begin, int64_t row_end, int64_t cap,
                                      int32_t* i_out, int32_t* j_out, float* d_out, int64_t* total, void* stream)
{
    if (!e) return hm_fail(nullptr, HM_E_ARG, "hm_pairwise_candidates: engine is NULL");
    e->st.disarm();
    if (!total || cap < 0 || (cap > 0 && (!i_out || !j_out || !d_out)))
        return hm_fail(e, HM_E_ARG, "hm_pairwise_candidates: bad output pointers");
    if (!(c > 0.0f)) return hm_fail(e, HM_E_ARG, "hm_pairwise_candidates: curvature must be > 0");
    hipStream_t s = (hipStream_t)stream;
    HM_HIP(hipSetDevice(e->device));
    *total = 0;
    TopkResult res;
    int rc = hm_topk_core(e, c, thr, 0, row_begin, row_end, true, true, -1, &res, s);
    if (rc == HM_E_CAPACITY) return hm_candidates_by_rows(e, c, thr, row_begin, row_end, cap, i_out, j_out, d_out, total, s);
    if (rc) return rc;
    *total = res.total;
    if (!res.ent || res.valid == 0 || cap == 0) return HM_OK;
    int64_t ncopy = 0;
    return hm_copy_valid(e, res, cap, i_out, j_out, d_out, &ncopy, s);
}

extern "C" int hm_row_argmin(hm_engine* e, int64_t row, int64_t n_partners, float c, float thr, float* d, int32_t* i, int32_t* j,
                             int32_t* found, void* stream)
{
    if (!e) return hm_fail(nullptr, HM_E_ARG, "hm_row_argmin: engine is NULL");
    e->st.disarm();
    if (!d || !i || !j || !found) return hm_fail(e, HM_E_ARG, "hm_row_argmin: NULL output pointer");
    if (row < 0 || row >= e->n || n_partners < 0 || n_partners > e->n || !(c > 0.0f))
        return hm_fail(e, HM_E_ARG, "hm_row_argmin: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    HM_HIP(hipSetDevice(e->device));
    *found = 0; *d = 0.f; *i = -1; *j = -1;
    if (!(thr > 0.0f) || n_partners == 0) return HM_OK;
    // row tiles (hm_newrow_key_kernel, the pipelined loop's row pass): one 64-bit key folded by atomicMin
    unsigned long long* key = e->d_rowkey + 2;
    HM_HIP(hipMemsetAsync(key, 0xff, sizeof(unsigned long long), s));
    int rc = hm_launch_row_key(e, row, n_partners, sqrtf(c), thr, key, s);
    if (rc) return rc;
    HM_HIP(hipMemcpyAsync(&e->h->ctr64[HM_CTR64_ROW_KEY], key, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HM_HIP(hipStreamSynchronize(s));
    const unsigned long long k64 = e->h->ctr64[HM_CTR64_ROW_KEY];
    if (k64 != ~0ull) {
        union { uint32_t u; float f; } cv; cv.u = (uint32_t)(k64 >> 32);
        const int64_t p = (int64_t)(uint32_t)k64;
        *found = 1; *d = cv.f; *i = (int32_t)(p < row ? p : row); *j = (int32_t)(p < row ? row : p);
    }
    return HM_OK;
}
