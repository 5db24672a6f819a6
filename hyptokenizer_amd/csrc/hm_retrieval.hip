// hm_retrieval.hip -- fused hyperbolic retrieval: the rank of every matched pair (recall@K) and the exact k nearest keys of
// every query, without the B x B distance matrix.
//
// Replaces compute_recall_at_k of the reference (scripts/train_retrieval.py:176-229: B^2 calls of distance(...).item() into a
// matrix, then torch.topk per row and per column) and the per-query search of its FAISS branch (index.search(q, k),
// tokenizer/hyperbolic_merge.py:217, tokenizer/fast_hyperbolic_merge.py:302-304).
//
// Both are the pair-tile walk of hm_grad_device.h with a forward-only fold: a block of 256 threads owns 64 rows of A, walks B
// in ascending tiles of 64 rows, thread (r = lane, q = wave) evaluates the canonical u (hm_g_u: torch's reduction order, plain
// fp32, the bits of batch_distance) of row r against rows 16 q .. 16 q + 15 of the tile.
//
// Comparisons are defined on the canonical DISTANCE, not on u (acosh maps several u to one fp32 distance, and a computed acosh
// need not be monotone to the last bit).  The kernels decide in the u domain only where that is provably the same decision:
//   * equal clamped u  =>  equal distance (the same operations on the same value);
//   * with eps = 2^-10 and a pivot x >= 1 the code uses lo = fl(x (1 - eps)) and hi = fl(x (1 + eps)) (each within 6e-8
//     relative of the exact product).  acosh is concave with acosh'(t) = 1 / sqrt(t^2 - 1) > 1 / t, hence
//       y < lo:  acosh(x) - acosh(y) >= (x - y) acosh'(x) > (x - y) / x >= eps (1 - 1e-4)             > 9.7e-4
//       y > hi:  acosh(y) - acosh(x) >= (y - x) acosh'(y) > (y - x) / y >= eps / (1 + eps) (1 - 1e-4) > 9.7e-4
//     so the true distances times sqrt(c) differ by more than 9.7e-4 in absolute terms on either side, while they are at
//     most acosh(FLT_MAX) = 89.4, where one fp32 ulp is 7.6e-6.  hm::acosh_c follows glibc's acoshf (a few ulp) and the
//     correctly rounded division by sqrt(c) is monotone, so the computed distances are ordered the same way, strictly.
//   Every pair with lo <= y <= hi gets its distance evaluated and compared as such.
// NaN orders as torch.sort orders it in the ranks (greater than every number, equal to NaN) and is never selected by the k-NN.
#include "hm_retrieval_device.h"

#pragma clang fp contract(off)

#define HM_KNN_MAX_K 128
#define HM_RT_MAX_ROWS ((int64_t)1 << 20)

// ------------------------------------------------------------------------------------------------
// ranks: rank[i] = #{ j : D[i, j] < D[i, i] } + #{ j < i : D[i, j] == D[i, i] },  D[i, j] = distance(A[i], B[j]), c = 1
// ------------------------------------------------------------------------------------------------
// The column direction is the same kernel with A and B exchanged (u is symmetric bit for bit): the owning index is then the
// column and "j" the row, which is exactly the tie rule of the column ranks.  The walk, its two tile layouts (MAXN = 0: A and
// B rows in LDS; 32 / 64 / 128: the A row in registers, the step DESIGN.md 5.11 left open) and the fixed-order sum of the four
// waves' counts live in hm_retrieval_device.h, shared with hm_recon.hip: identical results on every run.
template <int MAXN>
__global__ __launch_bounds__(HM_PT_THREADS) void hm_retrieval_rank_kernel(const float* __restrict__ A, const float* __restrict__ B, int64_t n,
                                                                           int64_t lda, int64_t ldb, int d1, int sign_mode,
                                                                           int32_t* __restrict__ rank)
{
    extern __shared__ float hm_pt_lds[];
    const int r = threadIdx.x & 63;
    const int64_t i0 = (int64_t)blockIdx.x * HM_PT, i = i0 + r;
    const auto own = [&](int rr) -> int64_t { return i0 + rr; };
    hm_rk_layout<MAXN> lay(hm_pt_lds, d1, sign_mode);
    lay.load_owner(A, n, lda, own);
    // the diagonal D[i, i]: the B rows of the block's own indices, through the same code path as every other pair
    lay.stage(B, n, ldb, own);
    __syncthreads();
    const hm_rk_pivot_t piv = hm_rk_pivot(hm::clamp_min_one(lay.u(r, r)));
    __syncthreads();
    int lt = 0, eq = 0;
    hm_rk_walk(lay, B, n, ldb, [&](int64_t j, float uc) {
        const int c = hm_rk_cmp(piv, uc);
        lt += c & 1;
        eq += (c >> 1) & (j < i);
    });
    hm_rk_reduce(lt, eq);
    if (threadIdx.x < HM_PT && i < n) rank[i] = lt + eq;
}

#define HM_RT_LAYOUT_DEFAULT 2                  // faster up to B = 16 384, 8 % slower at 65 536
static int g_rt_layout = 0;

static int hm_rank_launch(const float* A, const float* B, int64_t n, int64_t lda, int64_t ldb, int d1, int sign_mode, int32_t* rank,
                          hipStream_t s)
{
    return hm_rk_launch([](auto maxn) { return hm_retrieval_rank_kernel<decltype(maxn)::value>; },
                        g_rt_layout ? g_rt_layout : HM_RT_LAYOUT_DEFAULT, n, d1, s, A, B, n, lda, ldb, d1, sign_mode, rank);
}

extern "C" int hm_retrieval_ranks(const float* zt_dev, const float* zi_dev, int64_t n, int64_t ld_t, int64_t ld_i, int d1, int sign_mode,
                                  int32_t* rank_t2i_dev, int32_t* rank_i2t_dev, void* stream)
{
    if (n < 1 || n > 65536 || d1 < 2 || d1 > 129 || ld_t < d1 || ld_i < d1 || (sign_mode != 0 && sign_mode != 1))
        return hm_fail(nullptr, HM_E_ARG, "hm_retrieval_ranks: bad arguments");
    if (!zt_dev || !zi_dev || (!rank_t2i_dev && !rank_i2t_dev)) return hm_fail(nullptr, HM_E_ARG, "hm_retrieval_ranks: NULL pointer");
    hipStream_t s = (hipStream_t)stream;
    if (rank_t2i_dev)
        if (int rc = hm_rank_launch(zt_dev, zi_dev, n, ld_t, ld_i, d1, sign_mode, rank_t2i_dev, s)) return rc;
    if (rank_i2t_dev)
        if (int rc = hm_rank_launch(zi_dev, zt_dev, n, ld_i, ld_t, d1, sign_mode, rank_i2t_dev, s)) return rc;
    HM_HIP0(hipGetLastError());
    return HM_OK;
}

// ------------------------------------------------------------------------------------------------
// k-NN: per query row the k smallest (distance, key index), NaN never selected
// ------------------------------------------------------------------------------------------------
// Per A row the block keeps an UNSORTED list of up to k (distance bits, index) in LDS (row stride k | 1: lane r walking its row
// hits 64 different banks), the position of its largest entry ("the k-th") and an admission bound in the u domain,
// ub = u_kth (1 + 2^-10): a pair with clamped u above ub is strictly farther than the k-th (header of this file) and is dropped
// without an acosh.  The u of every listed entry is parked in the row's slice of the distance OUTPUT until the final write,
// so the call needs no scratch at all.
// A tile in three steps: (1) every thread writes the clamped u of its 16 pairs to the 64 x 64 tile Ws and a 16-bit mask of the
// pairs that pass the bound; (2) after the barrier lane r of wave 0 visits the flagged pairs of row r in ascending key
// index, re-checks the (possibly tightened) bound, evaluates the distance and, if (distance, index) is below the k-th, overwrites
// the k-th and rescans the list for the new one (k reads; after the first tiles admissions are rare: about k ln(N / k) per row);
// (3) the next tile is staged.  Keys arrive in ascending index, so an equal distance with a larger index never displaces.
// At the end thread (r, q) ranks entries q, q + 4, .. of row r among the row's entries (keys are distinct: indices are) and
// writes each to its place; missing places are padded with (+inf, -1).  Nothing depends on the tile size or the grid.
// One block per 64 queries: below 64 x 256 = 16 384 queries the chip is not full and the call is latency-bound (5.12).
__host__ __device__ __forceinline__ int hm_knn_stride(int k) { return k | 1; }
static size_t hm_knn_lds_bytes(int d1, int k)
{
    return sizeof(float) * ((size_t)2 * HM_PT * hm_pt_stride(d1) + (size_t)HM_PT * HM_PT_WS + (size_t)2 * HM_PT * hm_knn_stride(k));
}

__global__ __launch_bounds__(HM_PT_THREADS) void hm_knn_kernel(const float* __restrict__ A, int64_t na, const float* __restrict__ B, int64_t nb,
                                                                int64_t lda, int64_t ldb, int d1, float sqrt_c, int sign_mode, int k,
                                                                int exclude_self, float* __restrict__ d_out, int32_t* __restrict__ i_out)
{
    extern __shared__ float hm_pt_lds[];
    __shared__ float ubound[HM_PT];
    __shared__ uint32_t masks[4][HM_PT];
    const int SA = hm_pt_stride(d1), KS = hm_knn_stride(k);
    float* As = hm_pt_lds;
    float* Bs = As + HM_PT * SA;
    float* Ws = Bs + HM_PT * SA;
    float* Ld = Ws + HM_PT * HM_PT_WS;
    int32_t* Li = reinterpret_cast<int32_t*>(Ld + HM_PT * KS);
    const int r = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int64_t i0 = (int64_t)blockIdx.x * HM_PT, i = i0 + r;
    hm_pt_stage(A, na, lda, d1, i0, As);
    if (q == 0) ubound[r] = INFINITY;
    // state of the list of row r, kept by lane r of wave 0
    int cnt = 0, kp = 0, ki = 0;
    float kd = 0.0f;
    float* ld_row = Ld + r * KS;
    int32_t* li_row = Li + r * KS;
    float* u_row = d_out + (i < na ? i : 0) * (int64_t)k;      // parked u of the listed entries (only touched where i < na)
    __syncthreads();
    for (int64_t j0 = 0; j0 < nb; j0 += HM_PT) {
        hm_pt_stage(B, nb, ldb, d1, j0, Bs);
        __syncthreads();
        const float ub = ubound[r];
        uint32_t mask = 0;
        for (int jj = 0; jj < HM_PT_JPT; ++jj) {
            const int jl = q * HM_PT_JPT + jj;
            const int64_t j = j0 + jl;
            float uc = INFINITY;
            if (i < na && j < nb && !(exclude_self && j == i)) {
                uc = hm::clamp_min_one(hm_g_u(As + r * SA, Bs + jl * SA, d1, sign_mode));
                if (uc <= ub) mask |= 1u << jj;                // false for NaN
            }
            Ws[r * HM_PT_WS + jl] = uc;
        }
        masks[q][r] = mask;
        __syncthreads();
        if (q == 0 && i < na) {
            for (int w = 0; w < 4; ++w) {
                uint32_t m = masks[w][r];
                while (m) {
                    const int jj = __builtin_ctz(m);
                    m &= m - 1;
                    const int jl = w * HM_PT_JPT + jj;
                    const float uc = Ws[r * HM_PT_WS + jl];
                    if (!(uc <= ubound[r])) continue;
                    const float dj = hm::dist_from_u(uc, sqrt_c);
                    const int j = (int)(j0 + jl);
                    bool rescan = false;
                    if (cnt < k) {
                        ld_row[cnt] = dj; li_row[cnt] = j; u_row[cnt] = uc;
                        cnt += 1;
                        rescan = cnt == k;
                    } else if (dj < kd || (dj == kd && j < ki)) {
                        ld_row[kp] = dj; li_row[kp] = j; u_row[kp] = uc;
                        rescan = true;
                    }
                    if (rescan) {
                        kp = 0; kd = ld_row[0]; ki = li_row[0];
                        for (int e = 1; e < k; ++e) {
                            const float de = ld_row[e];
                            if (de > kd || (de == kd && li_row[e] > ki)) { kp = e; kd = de; ki = li_row[e]; }
                        }
                        ubound[r] = u_row[kp] * HM_RT_BAND_HI;
                    }
                }
            }
        }
        // the barrier after the next staging orders these list / bound updates before the next tile's reads of them
    }
    __shared__ int cnts[HM_PT];
    if (q == 0) cnts[r] = cnt;
    __syncthreads();
    if (i < na) {
        const int c = cnts[r];
        float* dr = d_out + i * (int64_t)k;
        int32_t* ir = i_out + i * (int64_t)k;
        for (int e = q; e < k; e += 4) {
            if (e >= c) continue;
            const float de = ld_row[e];
            const int ie = li_row[e];
            int pos = 0;
            for (int f = 0; f < c; ++f) {
                const float df = ld_row[f];
                if (df < de || (df == de && li_row[f] < ie)) pos += 1;
            }
            dr[pos] = de; ir[pos] = ie;
        }
        for (int e = c + q; e < k; e += 4) { dr[e] = INFINITY; ir[e] = -1; }
    }
}

extern "C" int hm_knn(const float* q_dev, int64_t nq, const float* k_dev, int64_t nk, int64_t ld_q, int64_t ld_k, int d1, float c,
                      int sign_mode, int k, int exclude_self, float* d_out_dev, int32_t* i_out_dev, void* stream)
{
    if (nq < 1 || nk < 1 || nq > HM_RT_MAX_ROWS || nk > HM_RT_MAX_ROWS || d1 < 2 || d1 > 129 || ld_q < d1 || ld_k < d1 || !(c > 0.0f) ||
        (sign_mode != 0 && sign_mode != 1) || k < 1 || k > HM_KNN_MAX_K || k > nk)
        return hm_fail(nullptr, HM_E_ARG, "hm_knn: bad arguments");
    if (!q_dev || !k_dev || !d_out_dev || !i_out_dev) return hm_fail(nullptr, HM_E_ARG, "hm_knn: NULL pointer");
    const size_t lds = hm_knn_lds_bytes(d1, k);
    HM_HIP0(hm_pt_allow_lds(hm_knn_kernel, lds));
    hipLaunchKernelGGL(hm_knn_kernel, dim3((unsigned)((nq + HM_PT - 1) / HM_PT)), dim3(HM_PT_THREADS), lds, (hipStream_t)stream, q_dev, nq,
                       k_dev, nk, ld_q, ld_k, d1, sqrtf(c), sign_mode, k, exclude_self ? 1 : 0, d_out_dev, i_out_dev);
    HM_HIP0(hipGetLastError());
    return HM_OK;
}

extern "C" int hm_debug_retrieval_layout(int layout)
{
    if (layout < 0 || layout > 2) return hm_fail(nullptr, HM_E_ARG, "hm_debug_retrieval_layout: layout must be 0, 1 or 2");
    g_rt_layout = layout;
    return HM_OK;
}
