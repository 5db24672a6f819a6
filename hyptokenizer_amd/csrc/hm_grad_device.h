// hm_grad_device.h -- device helpers shared by the Lorentz row kernels and the backward kernels (hm_lorentz.hip, hm_contrastive.hip).
//
// Derivative conventions: what is differentiated is the reference's torch expression as torch
// differentiates it, not the ideal function.
//   u          = s0 * x0 * y0 + s1 * sum_k x_k y_k, (s0, s1) = (-1, +1) under "reference", (+1, -1) under "lorentz";
//                evaluated in torch's reduction order (hm::torch_order_sum), i.e. with the bits of the forward kernels
//   clamp      : torch.clamp(u, min = 1 + 1e-8) passes the gradient where u >= 1.0f and gives exactly 0 below
//   acosh      : grad * 1 / sqrt(a * a - 1) on the clamped a; at a == 1 that is +-inf (0 * inf = NaN), as in torch
#pragma once
#include "hm_common.h"
#include "hm_device_math.h"

#pragma clang fp contract(off)

// canonical u of two rows in reference column order (column 0 = time); any pointer kind (global or LDS)
__device__ __forceinline__ float hm_g_u(const float* x, const float* y, int d1, int sign_mode)
{
    const float S = hm::torch_order_sum([&](int s) { return x[1 + s] * y[1 + s]; }, d1 - 1);
    const float t = x[0] * y[0];
    const float m = t - S;
    return sign_mode ? m : -m;
}

// d distance / d u for upstream gradient g of the distance: acosh backward, then the clamp's mask
__device__ __forceinline__ float hm_g_dist_du(float g, float u, float sqrt_c)
{
    if (!(u >= 1.0f)) return 0.0f;                            // clamped (or NaN u: the mask u >= min is false)
    const float gd = g / sqrt_c;
    return gd * (1.0f / __builtin_sqrtf(u * u - 1.0f));
}

// factors of du/dx0 and du/dx_k
__device__ __forceinline__ float hm_g_s0(int sign_mode) { return sign_mode ? 1.0f : -1.0f; }
__device__ __forceinline__ float hm_g_s1(int sign_mode) { return sign_mode ? -1.0f : 1.0f; }

// ------------------------------------------------------------------------------------------------
// pair tiles: one block of 256 threads owns HM_PT rows of A and walks B in tiles of HM_PT rows
// ------------------------------------------------------------------------------------------------
// Both tiles are staged in LDS in reference column order at the odd row stride SA = d1 | 1, so that lane r reading row r
// hits 64 different banks and a row of B read by a whole wave is a broadcast.  Thread (r = lane, q = wave) evaluates the
// canonical u (hm_g_u: torch's reduction order, the bits of hm_rows_distance) of row r of A against rows 16 q .. 16 q + 15
// of the B tile.  Every pair counts here and u - 1 carries the answer for close points, so no reduced-precision or
// re-associated product is used.
#define HM_PT 64
#define HM_PT_THREADS 256
#define HM_PT_JPT (HM_PT / 4)        // pairs per thread and tile
#define HM_PT_WS (HM_PT + 1)         // row stride of the coefficient tile
#define HM_PT_SLACK 136              // the product phase reads up to 4 * NM <= 132 columns of a B row

__host__ __device__ __forceinline__ int hm_pt_stride(int d1) { return d1 | 1; }
__host__ __device__ __forceinline__ size_t hm_pt_lds_floats(int d1, bool with_coef)
{
    return (size_t)2 * HM_PT * hm_pt_stride(d1) + HM_PT_SLACK + (with_coef ? (size_t)HM_PT * HM_PT_WS : 0);
}

// rows [r0, r0 + HM_PT) of M[n, ld] into tile (zero rows past n)
__device__ __forceinline__ void hm_pt_stage(const float* __restrict__ M, int64_t n, int64_t ld, int d1, int64_t r0, float* tile)
{
    const int SA = hm_pt_stride(d1);
    for (int idx = threadIdx.x; idx < HM_PT * d1; idx += HM_PT_THREADS) {
        const int r = idx / d1, k = idx - r * d1;
        tile[r * SA + k] = r0 + r < n ? M[(r0 + r) * ld + k] : 0.0f;
    }
}

// gA[i, :] = sum_j coef(i, j, u_ij) * (s0 B[j, 0], s1 B[j, 1:]) over all rows j of B, j ascending: a fixed order, no
// atomics.  NM = ceil(d1 / 4): thread (r, q) accumulates columns q + 4 m, m < NM, of row r.
template <int NM, class COEF>
__device__ __forceinline__ void hm_pt_grad(const float* __restrict__ A, int64_t na, int64_t lda, const float* __restrict__ B, int64_t nb,
                                           int64_t ldb, int d1, int sign_mode, float* __restrict__ gA, int64_t ldo, COEF coef, float* lds)
{
    const int SA = hm_pt_stride(d1);
    float* As = lds;
    float* Bs = As + HM_PT * SA;
    float* Ws = Bs + HM_PT * SA + HM_PT_SLACK;
    const int r = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int64_t i0 = (int64_t)blockIdx.x * HM_PT, i = i0 + r;
    hm_pt_stage(A, na, lda, d1, i0, As);
    float acc[NM];
#pragma unroll
    for (int m = 0; m < NM; ++m) acc[m] = 0.0f;
    for (int64_t j0 = 0; j0 < nb; j0 += HM_PT) {
        hm_pt_stage(B, nb, ldb, d1, j0, Bs);
        __syncthreads();
        for (int jj = 0; jj < HM_PT_JPT; ++jj) {
            const int jl = q * HM_PT_JPT + jj;
            const int64_t j = j0 + jl;
            float w = 0.0f;
            if (i < na && j < nb) w = coef(i, j, hm_g_u(As + r * SA, Bs + jl * SA, d1, sign_mode));
            Ws[r * HM_PT_WS + jl] = w;
        }
        __syncthreads();
        for (int jl = 0; jl < HM_PT; ++jl) {
            const float w = Ws[r * HM_PT_WS + jl];
            const float* br = Bs + jl * SA + q;
#pragma unroll
            for (int m = 0; m < NM; ++m) acc[m] = __builtin_fmaf(w, br[4 * m], acc[m]);
        }
        __syncthreads();
    }
    if (i < na) {
        const float s0 = hm_g_s0(sign_mode), s1 = hm_g_s1(sign_mode);
#pragma unroll
        for (int m = 0; m < NM; ++m) {
            const int k = q + 4 * m;
            if (k < d1) gA[i * ldo + k] = (k == 0 ? s0 : s1) * acc[m];
        }
    }
}

// host side: dynamic LDS above 64 KB has to be granted per kernel
template <class K>
static inline hipError_t hm_pt_allow_lds(K kernel, size_t bytes)
{
    if (bytes <= 48 * 1024) return hipSuccess;
    return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}
