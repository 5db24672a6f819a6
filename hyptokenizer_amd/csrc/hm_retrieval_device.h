// hm_retrieval_device.h -- the rank walk of hm_retrieval.hip and hm_recon.hip: "count the rows of a table that are nearer to
// my owner row than my pivot is".  A block of 256 threads owns 64 rows, thread (r = lane, q = wave) compares owner row r with
// rows 16 q .. 16 q + 15 of every 64-row tile of the table.  Here: the comparison of a pair with the pivot (hm_rk_pivot,
// hm_rk_cmp; proof: header of hm_retrieval.hip), the two tile layouts (hm_rk_layout), the tile loop (hm_rk_walk), the sum of the
// four waves' counts (hm_rk_reduce) and the host's choice of the layout with its launch (hm_rk_launch).
#pragma once
#include <type_traits>

#include "hm_grad_device.h"

#pragma clang fp contract(off)

#define HM_RT_BAND_LO 0.9990234375f          // 1 - 2^-10
#define HM_RT_BAND_HI 1.0009765625f          // 1 + 2^-10

// a pivot: its clamped u, its distance at c = 1 and the band outside which u decides
struct hm_rk_pivot_t {
    float u, d, lo, hi;
};

__device__ __forceinline__ hm_rk_pivot_t hm_rk_pivot(float uc)
{
    return {uc, hm::dist_from_u(uc, 1.0f), uc * HM_RT_BAND_LO, uc * HM_RT_BAND_HI};
}

// one pair with clamped u `uc` against the pivot: 1 = less, 2 = equal, 0 = greater
__device__ __forceinline__ int hm_rk_cmp(const hm_rk_pivot_t p, float uc)
{
    const bool pnan = p.u != p.u;
    if (uc != uc) return pnan ? 2 : 0;                         // NaN is never less; it equals a NaN pivot
    if (pnan) return 1;                                        // every number is less than NaN
    if (uc == p.u) return 2;
    if (uc < p.lo) return 1;
    if (uc > p.hi) return 0;
    const float dj = hm::dist_from_u(uc, 1.0f);
    return dj < p.d ? 1 : (dj == p.d ? 2 : 0);
}

// The register layout: thread (r, q) keeps its owner row in MAXN + 1 registers for the whole kernel; only the table's tile
// lives in LDS, one row per MAXN + 4 floats: spatial column s at offset s (so that eight consecutive terms are two aligned
// float4), the time column at offset MAXN.  A whole wave reads the same tile row: every ds_read_b128 is a broadcast.  One
// instantiation per column class (MAXN = 32, 64, 128).  hm_rt_u_reg is hm::torch_order_sum unrolled to the class's length with
// wave-uniform guards in place of the run-time loop bounds: every accumulator receives the same terms in the same order, so u
// has the same bits (tests/test_gpu_retrieval.py runs both layouts against the oracle).  n = d1 - 1 >= 8; narrower rows take
// the LDS layout.
template <int MAXN>
__device__ __forceinline__ float hm_rt_u_reg(const float (&a)[MAXN], float a0, const float* __restrict__ b, int n, int sign_mode)
{
    constexpr int NV = MAXN / 8;
    const int vec_size = n >> 3, main_end = (vec_size >> 2) << 2;
    float ps[4][8];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int l = 0; l < 8; ++l) ps[k][l] = 0.0f;
    float acc = 0.0f;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        if (v <= vec_size) {
            const float4 b0 = *reinterpret_cast<const float4*>(b + 8 * v);
            const float4 b1 = *reinterpret_cast<const float4*>(b + 8 * v + 4);
            const float bb[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
            if (v < main_end) {                                 // the 4-way interleaved part: vector v feeds accumulator v & 3
#pragma unroll
                for (int l = 0; l < 8; ++l) ps[v & 3][l] = ps[v & 3][l] + a[8 * v + l] * bb[l];
            } else if (v < vec_size) {                          // the remaining whole vectors feed accumulator 0
#pragma unroll
                for (int l = 0; l < 8; ++l) ps[0][l] = ps[0][l] + a[8 * v + l] * bb[l];
            } else {                                            // the scalar tail, added up from 0 before the vector sums
#pragma unroll
                for (int l = 0; l < 8; ++l)
                    if (8 * v + l < n) acc = acc + a[8 * v + l] * bb[l];
            }
        }
    }
#pragma unroll
    for (int k = 1; k < 4; ++k)
#pragma unroll
        for (int l = 0; l < 8; ++l) ps[0][l] = ps[0][l] + ps[k][l];
#pragma unroll
    for (int l = 0; l < 8; ++l) acc = acc + ps[0][l];
    const float t = a0 * b[MAXN];
    const float m = t - acc;
    return sign_mode ? m : -m;
}

// Where the 64 owner rows and a 64-row tile live.  MAXN = 0: both in LDS at the odd stride d1 | 1 (the layout of
// hm_grad_device.h; every width), u by hm_g_u.  MAXN = 32 / 64 / 128: the register layout above, u by hm_rt_u_reg.  `idx` maps
// row rr of a tile to a row of M[n, ld]; a row outside [0, n) is a row of zeros and is not read: r0 + rr and a gathered list
// with -1 for its dead entries are the same loop.  Construct it in the kernel body; every member is inlined there.
template <int MAXN>
struct hm_rk_layout {
    static constexpr bool REG = MAXN > 0;
    float a[REG ? MAXN : 1], a0;                               // REG: the owner row of this thread
    float *As, *Bs;                                            // As: the owner rows (LDS layout only); Bs: the tile
    int d1, sign_mode, stride;

    __device__ __forceinline__ hm_rk_layout(float* lds, int d1_, int sign_mode_)
        : As(lds), d1(d1_), sign_mode(sign_mode_), stride(REG ? MAXN + 4 : hm_pt_stride(d1_))
    {
        Bs = REG ? lds : lds + HM_PT * stride;
    }

    static size_t lds_bytes(int d1) { return sizeof(float) * (REG ? (size_t)HM_PT * (MAXN + 4) : hm_pt_lds_floats(d1, false)); }

    template <class IDX>
    __device__ __forceinline__ void stage_into(float* tile, const float* __restrict__ M, int64_t n, int64_t ld, IDX idx) const
    {
        for (int e = threadIdx.x; e < HM_PT * d1; e += HM_PT_THREADS) {
            const int rr = e / d1, k = e - rr * d1;
            const int64_t row = idx(rr);
            tile[rr * stride + (REG ? (k == 0 ? MAXN : k - 1) : k)] = (uint64_t)row < (uint64_t)n ? M[row * ld + k] : 0.0f;
        }
    }

    template <class IDX>
    __device__ __forceinline__ void stage(const float* __restrict__ M, int64_t n, int64_t ld, IDX idx) const
    {
        stage_into(Bs, M, n, ld, idx);
    }

    // the owner rows: collectively into As, or each thread its own into registers (a barrier before the first u)
    template <class IDX>
    __device__ __forceinline__ void load_owner(const float* __restrict__ M, int64_t n, int64_t ld, IDX idx)
    {
        if constexpr (REG) {
            const int64_t row = idx((int)(threadIdx.x & 63));
            const bool live = (uint64_t)row < (uint64_t)n;
            const float* arow = M + (live ? row : 0) * ld;
#pragma unroll
            for (int s = 0; s < MAXN; ++s) a[s] = (s < d1 - 1 && live) ? arow[1 + s] : 0.0f;
            a0 = live ? arow[0] : 0.0f;
        } else {
            stage_into(As, M, n, ld, idx);
        }
    }

    // the canonical u of owner row r (this thread's lane) against row jl of the tile
    __device__ __forceinline__ float u(int r, int jl) const
    {
        if constexpr (REG) return hm_rt_u_reg<MAXN>(a, a0, Bs + jl * stride, d1 - 1, sign_mode);
        else return hm_g_u(As + r * stride, Bs + jl * stride, d1, sign_mode);
    }
};

// B[nb, ldb] in ascending tiles of 64 rows; pair(j, clamped u of owner row r against B[j]) for this thread's 16 rows of each.
// The register layouts would otherwise unroll the 16 pairs over MAXN registers.
template <class LAYOUT, class PAIR>
__device__ __forceinline__ void hm_rk_walk(const LAYOUT& lay, const float* __restrict__ B, int64_t nb, int64_t ldb, PAIR pair)
{
    const int r = threadIdx.x & 63, q = threadIdx.x >> 6;
    for (int64_t j0 = 0; j0 < nb; j0 += HM_PT) {
        lay.stage(B, nb, ldb, [&](int rr) -> int64_t { return j0 + rr; });
        __syncthreads();
#pragma unroll 1
        for (int jj = 0; jj < HM_PT_JPT; ++jj) {
            const int jl = q * HM_PT_JPT + jj;
            const int64_t j = j0 + jl;
            if (j >= nb) break;                                // wave-uniform
            pair(j, hm::clamp_min_one(lay.u(r, jl)));
        }
        __syncthreads();
    }
}

// the four waves' partial counts of owner row r in a fixed order, all lt, then all eq: no atomics.  The sums are wave 0's.
__device__ __forceinline__ void hm_rk_reduce(int& lt, int& eq)
{
    __shared__ int part_lt[4][HM_PT], part_eq[4][HM_PT];
    const int r = threadIdx.x & 63, q = threadIdx.x >> 6;
    part_lt[q][r] = lt;
    part_eq[q][r] = eq;
    __syncthreads();
    if (q == 0) {
        lt = eq = 0;
        for (int w = 0; w < 4; ++w) lt += part_lt[w][r];
        for (int w = 0; w < 4; ++w) eq += part_eq[w][r];
    }
}

// Host: one block per 64 of the n owner rows.  layout 2 keeps the owner row in registers (MAXN = 32 / 64 / 128 for
// d1 <= 33 / 65 / 129); layout 1, and every row narrower than 9 columns, takes the LDS layout.  kernel_of(constant MAXN)
// returns that instantiation of the caller's kernel.
template <int MAXN, class KERNEL_OF, class... ARGS>
static int hm_rk_launch_as(KERNEL_OF kernel_of, int64_t n, int d1, hipStream_t s, ARGS... args)
{
    auto kernel = kernel_of(std::integral_constant<int, MAXN>{});
    const size_t lds = hm_rk_layout<MAXN>::lds_bytes(d1);
    HM_HIP0(hm_pt_allow_lds(kernel, lds));
    hipLaunchKernelGGL(kernel, dim3((unsigned)((n + HM_PT - 1) / HM_PT)), dim3(HM_PT_THREADS), lds, s, args...);
    return HM_OK;
}

template <class KERNEL_OF, class... ARGS>
static int hm_rk_launch(KERNEL_OF kernel_of, int layout, int64_t n, int d1, hipStream_t s, ARGS... args)
{
    if (layout != 2 || d1 < 9) return hm_rk_launch_as<0>(kernel_of, n, d1, s, args...);
    if (d1 <= 33) return hm_rk_launch_as<32>(kernel_of, n, d1, s, args...);
    if (d1 <= 65) return hm_rk_launch_as<64>(kernel_of, n, d1, s, args...);
    return hm_rk_launch_as<128>(kernel_of, n, d1, s, args...);
}
