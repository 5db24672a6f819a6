// hm_contrastive.hip -- fused hyperbolic InfoNCE and triplet loss (multimodal/contrastive_loss.py of the reference),
// forward and backward, without the B x B matrix.
//
// S[i, j] = -distance(z_text[i], z_img[j], c = 1) / temp.  The reference fills S row by row in a Python loop of B
// `distance` calls (:36-46), then takes cross_entropy over rows and over columns (:52-58).  Here S exists only as
// 64 x 64 tiles in registers / LDS (pair tiles of hm_grad_device.h):
//   hm_infonce_lse_kernel  one pass per direction: the block owning 64 rows of A folds every tile into a running
//                          (max, sum-exp) per row; the column direction is the same kernel with A and B exchanged (u is
//                          symmetric bit for bit), so no partial column state crosses blocks and the order is fixed
//   hm_infonce_finish      per-sample losses and their fixed-order sum
//   hm_infonce_bwd_kernel  recomputes the tiles, forms dL/dS from the saved log-sum-exps, chains through -1/temp, acosh'
//                          and the clamp mask, and accumulates the gradient rows as coefficient-tile x B-tile products;
//                          again once per direction
//   hm_triplet_kernel      row-wise relu(d(a, p) - d(a, n) + margin) and its gradients
#include "hm_grad_device.h"

#pragma clang fp contract(off)

__device__ __forceinline__ float hm_nce_logit(float u, float temp) { return -hm::dist_from_u(u, 1.0f) / temp; }

__global__ __launch_bounds__(HM_PT_THREADS) void hm_infonce_lse_kernel(const float* __restrict__ A, const float* __restrict__ B, int64_t n,
                                                                        int64_t lda, int64_t ldb, int d1, float temp, int sign_mode,
                                                                        float* __restrict__ lse, float* __restrict__ diag)
{
    extern __shared__ float hm_pt_lds[];
    __shared__ float part_m[4][HM_PT], part_s[4][HM_PT];
    const int SA = hm_pt_stride(d1);
    float* As = hm_pt_lds;
    float* Bs = As + HM_PT * SA;
    const int r = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int64_t i0 = (int64_t)blockIdx.x * HM_PT, i = i0 + r;
    hm_pt_stage(A, n, lda, d1, i0, As);
    float run_m = -INFINITY, run_s = 0.0f;
    for (int64_t j0 = 0; j0 < n; j0 += HM_PT) {
        hm_pt_stage(B, n, ldb, d1, j0, Bs);
        __syncthreads();
        float sv[HM_PT_JPT];
        float tile_m = -INFINITY;
#pragma unroll
        for (int jj = 0; jj < HM_PT_JPT; ++jj) {
            const int jl = q * HM_PT_JPT + jj;
            const int64_t j = j0 + jl;
            sv[jj] = -INFINITY;
            if (i < n && j < n) {
                sv[jj] = hm_nce_logit(hm_g_u(As + r * SA, Bs + jl * SA, d1, sign_mode), temp);
                if (diag != nullptr && i == j) diag[i] = sv[jj];
            }
            tile_m = fmaxf(tile_m, sv[jj]);
        }
        if (tile_m > -INFINITY) {
            const float new_m = fmaxf(run_m, tile_m);
            float acc = run_s * expf(run_m - new_m);          // exp(-inf) = 0 on the first tile
#pragma unroll
            for (int jj = 0; jj < HM_PT_JPT; ++jj) acc = acc + expf(sv[jj] - new_m);
            run_m = new_m; run_s = acc;
        }
        __syncthreads();
    }
    part_m[q][r] = run_m; part_s[q][r] = run_s;
    __syncthreads();
    if (q == 0 && i < n) {
        float m = part_m[0][r];
        for (int w = 1; w < 4; ++w) m = fmaxf(m, part_m[w][r]);
        float s = 0.0f;
        for (int w = 0; w < 4; ++w) if (part_m[w][r] > -INFINITY) s = s + part_s[w][r] * expf(part_m[w][r] - m);
        lse[i] = m + logf(s);
    }
}

// losses[i] = ((lse_row[i] - S_ii) + (lse_col[i] - S_ii)) / 2; *total = their sum in a fixed order (one block)
__global__ __launch_bounds__(1024) void hm_infonce_finish_kernel(const float* __restrict__ lse_row, const float* __restrict__ lse_col,
                                                                  const float* __restrict__ diag, int64_t n, float* __restrict__ losses,
                                                                  float* __restrict__ total)
{
    __shared__ float part[1024];
    float acc = 0.0f;
    for (int64_t i = threadIdx.x; i < n; i += 1024) {
        const float l = ((lse_row[i] - diag[i]) + (lse_col[i] - diag[i])) / 2.0f;
        losses[i] = l;
        acc = acc + l;
    }
    part[threadIdx.x] = acc;
    __syncthreads();
    for (int step = 512; step > 0; step >>= 1) {
        if ((int)threadIdx.x < step) part[threadIdx.x] = part[threadIdx.x] + part[threadIdx.x + step];
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = part[0];
}

// dL/du for the pair (row i of A, row j of B): i indexes lse_a / the owning side, j the other one; w is the upstream weight
// of the per-sample losses (the same vector on both sides)
struct NceCoef {
    const float* lse_a; const float* lse_b; const float* w; float temp;
    __device__ __forceinline__ float operator()(int64_t i, int64_t j, float u) const
    {
        const float s = hm_nce_logit(u, temp);
        const float delta = i == j ? 1.0f : 0.0f;
        const float gs = (w[i] / 2.0f) * (expf(s - lse_a[i]) - delta) + (w[j] / 2.0f) * (expf(s - lse_b[j]) - delta);
        return hm_g_dist_du(-(gs / temp), u, 1.0f);
    }
};

template <int NM>
__global__ __launch_bounds__(HM_PT_THREADS) void hm_infonce_bwd_kernel(const float* __restrict__ A, const float* __restrict__ B, int64_t n,
                                                                        int64_t lda, int64_t ldb, int d1, int sign_mode,
                                                                        float* __restrict__ gA, int64_t ldo, NceCoef coef)
{
    extern __shared__ float hm_pt_lds[];
    hm_pt_grad<NM>(A, n, lda, B, n, ldb, d1, sign_mode, gA, ldo, coef, hm_pt_lds);
}

template <int NM>
static int hm_infonce_bwd_launch(const float* A, const float* B, int64_t n, int64_t lda, int64_t ldb, int d1, int sign_mode, float* gA,
                                 int64_t ldo, NceCoef coef, hipStream_t s)
{
    const size_t lds = sizeof(float) * hm_pt_lds_floats(d1, true);
    HM_HIP0(hm_pt_allow_lds(hm_infonce_bwd_kernel<NM>, lds));
    hipLaunchKernelGGL(hm_infonce_bwd_kernel<NM>, dim3((unsigned)((n + HM_PT - 1) / HM_PT)), dim3(HM_PT_THREADS), lds, s, A, B, n, lda, ldb,
                       d1, sign_mode, gA, ldo, coef);
    HM_HIP0(hipGetLastError());
    return HM_OK;
}

static bool hm_nce_args_ok(int64_t n, int64_t ld_t, int64_t ld_i, int d1, float temp, int sign_mode)
{
    return n >= 0 && n <= 65536 && d1 >= 2 && d1 <= 129 && ld_t >= d1 && ld_i >= d1 && temp > 0.0f && (sign_mode == 0 || sign_mode == 1);
}

extern "C" int hm_infonce_fwd(const float* zt_dev, const float* zi_dev, int64_t n, int64_t ld_t, int64_t ld_i, int d1, float temp,
                              int sign_mode, float* lse_row_dev, float* lse_col_dev, float* diag_dev, float* losses_dev,
                              float* total_dev, void* stream)
{
    if (!hm_nce_args_ok(n, ld_t, ld_i, d1, temp, sign_mode)) return hm_fail(nullptr, HM_E_ARG, "hm_infonce_fwd: bad arguments");
    if (!total_dev || (n > 0 && (!zt_dev || !zi_dev || !lse_row_dev || !lse_col_dev || !diag_dev || !losses_dev)))
        return hm_fail(nullptr, HM_E_ARG, "hm_infonce_fwd: NULL pointer");
    hipStream_t s = (hipStream_t)stream;
    if (n > 0) {
        const size_t lds = sizeof(float) * hm_pt_lds_floats(d1, false);
        HM_HIP0(hm_pt_allow_lds(hm_infonce_lse_kernel, lds));
        const dim3 grid((unsigned)((n + HM_PT - 1) / HM_PT));
        hipLaunchKernelGGL(hm_infonce_lse_kernel, grid, dim3(HM_PT_THREADS), lds, s, zt_dev, zi_dev, n, ld_t, ld_i, d1, temp, sign_mode,
                           lse_row_dev, diag_dev);
        hipLaunchKernelGGL(hm_infonce_lse_kernel, grid, dim3(HM_PT_THREADS), lds, s, zi_dev, zt_dev, n, ld_i, ld_t, d1, temp, sign_mode,
                           lse_col_dev, (float*)nullptr);
    }
    hipLaunchKernelGGL(hm_infonce_finish_kernel, dim3(1), dim3(1024), 0, s, lse_row_dev, lse_col_dev, diag_dev, n, losses_dev, total_dev);
    HM_HIP0(hipGetLastError());
    return HM_OK;
}

extern "C" int hm_infonce_bwd(const float* zt_dev, const float* zi_dev, int64_t n, int64_t ld_t, int64_t ld_i, int d1, float temp,
                              int sign_mode, const float* lse_row_dev, const float* lse_col_dev, const float* w_dev, float* g_text_dev,
                              float* g_img_dev, int64_t ld_out, void* stream)
{
    if (!hm_nce_args_ok(n, ld_t, ld_i, d1, temp, sign_mode) || ld_out < d1) return hm_fail(nullptr, HM_E_ARG, "hm_infonce_bwd: bad arguments");
    if (n == 0) return HM_OK;
    if (!zt_dev || !zi_dev || !lse_row_dev || !lse_col_dev || !w_dev || (!g_text_dev && !g_img_dev))
        return hm_fail(nullptr, HM_E_ARG, "hm_infonce_bwd: NULL pointer");
    hipStream_t s = (hipStream_t)stream;
    for (int pass = 0; pass < 2; ++pass) {
        float* out = pass ? g_img_dev : g_text_dev;
        if (!out) continue;
        const float* A = pass ? zi_dev : zt_dev;
        const float* B = pass ? zt_dev : zi_dev;
        const int64_t lda = pass ? ld_i : ld_t, ldb = pass ? ld_t : ld_i;
        const NceCoef coef{pass ? lse_col_dev : lse_row_dev, pass ? lse_row_dev : lse_col_dev, w_dev, temp};
        int st;
        if (d1 <= 36) st = hm_infonce_bwd_launch<9>(A, B, n, lda, ldb, d1, sign_mode, out, ld_out, coef, s);
        else if (d1 <= 68) st = hm_infonce_bwd_launch<17>(A, B, n, lda, ldb, d1, sign_mode, out, ld_out, coef, s);
        else st = hm_infonce_bwd_launch<33>(A, B, n, lda, ldb, d1, sign_mode, out, ld_out, coef, s);
        if (st != HM_OK) return st;
    }
    return HM_OK;
}

// triplet loss (:64-97): losses[t] = relu(d(a, p) - d(a, n) + margin); with w the gradients of sum_t w[t] * losses[t]
__global__ void hm_triplet_kernel(const float* __restrict__ a, const float* __restrict__ p, const float* __restrict__ n, int64_t b,
                                  int64_t ld, int d1, float margin, int sign_mode, const float* __restrict__ w, float* __restrict__ losses,
                                  float* __restrict__ ga, float* __restrict__ gp, float* __restrict__ gn, int64_t ldo)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= b) return;
    const float* ar = a + t * ld;
    const float* pr = p + t * ld;
    const float* nr = n + t * ld;
    const float up = hm_g_u(ar, pr, d1, sign_mode), un = hm_g_u(ar, nr, d1, sign_mode);
    const float z = (hm::dist_from_u(up, 1.0f) - hm::dist_from_u(un, 1.0f)) + margin;
    if (losses != nullptr) losses[t] = z > 0.0f ? z : (z != z ? z : 0.0f);
    if (w == nullptr) return;
    const float gz = z > 0.0f ? w[t] : 0.0f;                  // relu' at exactly 0 is 0
    const float gup = hm_g_dist_du(gz, up, 1.0f), gun = hm_g_dist_du(-gz, un, 1.0f);
    const float s0 = hm_g_s0(sign_mode), s1 = hm_g_s1(sign_mode);
    for (int k = 0; k < d1; ++k) {
        const float s = k == 0 ? s0 : s1;
        ga[t * ldo + k] = s * (gup * pr[k]) + s * (gun * nr[k]);
        gp[t * ldo + k] = s * (gup * ar[k]);
        gn[t * ldo + k] = s * (gun * ar[k]);
    }
}

extern "C" int hm_triplet_fwd_bwd(const float* a_dev, const float* p_dev, const float* n_dev, int64_t b, int64_t ld, int d1, float margin,
                                  int sign_mode, const float* w_dev, float* losses_dev, float* ga_dev, float* gp_dev, float* gn_dev,
                                  int64_t ld_out, void* stream)
{
    if (b < 0 || d1 < 2 || ld < d1 || (w_dev && ld_out < d1)) return hm_fail(nullptr, HM_E_ARG, "hm_triplet_fwd_bwd: bad arguments");
    if (b == 0) return HM_OK;
    if (!a_dev || !p_dev || !n_dev || (!w_dev && !losses_dev) || (w_dev && (!ga_dev || !gp_dev || !gn_dev)))
        return hm_fail(nullptr, HM_E_ARG, "hm_triplet_fwd_bwd: NULL pointer");
    hipLaunchKernelGGL(hm_triplet_kernel, dim3((unsigned)((b + 127) / 128)), dim3(128), 0, (hipStream_t)stream, a_dev, p_dev, n_dev, b, ld,
                       d1, margin, sign_mode, w_dev, losses_dev, ga_dev, gp_dev, gn_dev, ld_out);
    HM_HIP0(hipGetLastError());
    return HM_OK;
}
