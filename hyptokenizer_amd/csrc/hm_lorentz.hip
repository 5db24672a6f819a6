// hm_lorentz.hip -- the row-wise Lorentz primitives of the reference's embedding/lorentz_model.py on row-major arrays,
// forward and backward, engine-independent: batch_distance, minkowski_dot, distance, log_map, exp_map,
// project_to_hyperboloid and their vector-Jacobian products.
//
// Forward and backward share every scalar: the canonical u (hm_g_u) and the log_map coefficient, exp_map norm and project
// time coordinate of hm_device_math.h, so the backward kernels carry the forward kernels' bits by construction
// (DESIGN.md 5.11).  Each backward kernel walks the reference's torch expression backwards operation by operation (clamp
// masks, the mask * a + (1 - mask) * b arithmetic of log_map / exp_map, acosh' = 1 / sqrt(a^2 - 1) with its infinities).
// log_map, exp_map, project and the backward kernels take one thread per row; the two distance kernels a half-wave per
// row pair.
#include "hm_grad_device.h"

#pragma clang fp contract(off)

// launch geometry of the one-thread-per-row kernels
#define HM_ROW_GRID(b) dim3((unsigned)(((b) + 127) / 128)), dim3(128), 0, (hipStream_t)stream

// ------------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------------
// half-wave per row pair (coalesced)
__device__ __forceinline__ float hm_rm_u_halfwave(const float* x, const float* y, int d1, int sign_mode, int lane)
{
    const float S = hm_halfwave_sum(d1 - 1, lane, [&](int e) { return x[1 + e] * y[1 + e]; });
    const float t = x[0] * y[0];
    const float m = t - S;
    return sign_mode ? m : -m;
}

// one half-wave per 32 consecutive outputs (row-major enumeration of out[i, j])
__global__ __launch_bounds__(256) void hm_dense_kernel(const float* __restrict__ X, int64_t n1, const float* __restrict__ Y, int64_t n2,
                                                       int64_t ldx, int64_t ldy, int d1, float sqrt_c, int sign_mode,
                                                       float* __restrict__ out)
{
    const int lane = threadIdx.x & 63, t = lane & 31;
    const int64_t total = n1 * n2;
    const int64_t nhw = ((int64_t)gridDim.x * blockDim.x) >> 5;
    const int64_t hw = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 5;
    for (int64_t base = (hw & ~(int64_t)1) * HM_GATHER; base < total; base += nhw * HM_GATHER) {
        const int64_t mybase = base + (hw & 1) * HM_GATHER;
        const float u = hm_halfwave_gather(lane, [&](int k) {
            const int64_t o = mybase + k < total ? mybase + k : total - 1;
            const int64_t i = o / n2, j = o - i * n2;
            return hm_rm_u_halfwave(X + i * ldx, Y + j * ldy, d1, sign_mode, lane);
        });
        if (t < HM_GATHER && mybase + t < total) out[mybase + t] = hm::dist_from_u(u, sqrt_c);
    }
}

__global__ void hm_rows_minkowski_kernel(const float* __restrict__ x, const float* __restrict__ y, int64_t b, int64_t ld, int d1,
                                         int sign_mode, float* __restrict__ out)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= b) return;
    // minkowski_dot under the active convention = -u
    out[t] = -hm_g_u(x + t * ld, y + t * ld, d1, sign_mode);
}

__global__ __launch_bounds__(256) void hm_rows_distance_kernel(const float* __restrict__ x, const float* __restrict__ y, int64_t b, int64_t ld,
                                                               int d1, float sqrt_c, int sign_mode, float* __restrict__ out)
{
    const int lane = threadIdx.x & 63, t = lane & 31;
    const int64_t nhw = ((int64_t)gridDim.x * blockDim.x) >> 5;
    const int64_t hw = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 5;
    for (int64_t base = (hw & ~(int64_t)1) * HM_GATHER; base < b; base += nhw * HM_GATHER) {
        const int64_t mybase = base + (hw & 1) * HM_GATHER;
        const float u = hm_halfwave_gather(lane, [&](int k) {
            const int64_t r = mybase + k < b ? mybase + k : b - 1;
            return hm_rm_u_halfwave(x + r * ld, y + r * ld, d1, sign_mode, lane);
        });
        if (t < HM_GATHER && mybase + t < b) out[mybase + t] = hm::dist_from_u(u, sqrt_c);
    }
}

__global__ void hm_rows_log_map_kernel(const float* __restrict__ x, const float* __restrict__ y, int64_t b, int64_t ld, int d1,
                                       int sign_mode, float* __restrict__ out, int64_t ldo)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= b) return;
    const float* xr = x + t * ld;
    const float* yr = y + t * ld;
    const float u = hm_g_u(xr, yr, d1, sign_mode);
    const float m = -u;
    const float coef = hm::log_map_coef(u).coef;
    for (int k = 0; k < d1; ++k) out[t * ldo + k] = coef * (yr[k] + m * xr[k]);
}

__global__ void hm_rows_exp_map_kernel(const float* __restrict__ x, const float* __restrict__ v, int64_t b, int64_t ld, int d1,
                                       float* __restrict__ out, int64_t ldo)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= b) return;
    const float* xr = x + t * ld;
    const float* vr = v + t * ld;
    const float nn = hm::exp_map_norm(hm::torch_order_sum([&](int s) { return vr[1 + s] * vr[1 + s]; }, d1 - 1));
    const float ch = hm::cosh_c(nn), sh = hm::sinh_c(nn);
    for (int k = 0; k < d1; ++k) out[t * ldo + k] = ch * xr[k] + sh * (vr[k] / nn);
}

__global__ void hm_rows_project_kernel(const float* __restrict__ x, int64_t b, int64_t ld, int d1, float c, float* __restrict__ out,
                                       int64_t ldo)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= b) return;
    const float* xr = x + t * ld;
    float r2 = 0.0f;
    for (int k = 1; k < d1; ++k) r2 = __builtin_fmaf(xr[k], xr[k], r2);
    const float x0 = hm::project_x0(r2, c);
    for (int k = 1; k < d1; ++k) out[t * ldo + k] = xr[k];
    out[t * ldo] = x0;
}

// ------------------------------------------------------------------------------------------------
// backward
// ------------------------------------------------------------------------------------------------
// distance (:122-138) and minkowski_dot (:14-25): both are functions of u alone; gu = d out / d u * g
__global__ void hm_rows_u_bwd_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ g, int64_t b,
                                     int64_t ld, int d1, float sqrt_c, int sign_mode, int is_distance, float* __restrict__ gx,
                                     float* __restrict__ gy, int64_t ldo)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= b) return;
    const float* xr = x + t * ld;
    const float* yr = y + t * ld;
    float gu;
    if (is_distance) gu = hm_g_dist_du(g[t], hm_g_u(xr, yr, d1, sign_mode), sqrt_c);
    else gu = -g[t];                                          // minkowski_dot = -u
    const float s0 = hm_g_s0(sign_mode), s1 = hm_g_s1(sign_mode);
    for (int k = 0; k < d1; ++k) {
        const float s = k == 0 ? s0 : s1;
        gx[t * ldo + k] = s * (gu * yr[k]);
        gy[t * ldo + k] = s * (gu * xr[k]);
    }
}

// log_map (:96-119)
__global__ void hm_rows_log_map_bwd_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ g,
                                           int64_t ldg, int64_t b, int64_t ld, int d1, int sign_mode, float* __restrict__ gx,
                                           float* __restrict__ gy, int64_t ldo)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= b) return;
    const float* xr = x + t * ld;
    const float* yr = y + t * ld;
    const float* gr = g + t * ldg;
    // forward, as hm_rows_log_map_kernel
    const float u = hm_g_u(xr, yr, d1, sign_mode);
    const float m = -u;                                       // minkowski_dot(x, y) under the active convention
    const hm::LogMapCoef lc = hm::log_map_coef(u);
    const float a = lc.a, A = lc.A, Q = lc.Q, coef0 = lc.coef0, coef1 = lc.coef;
    const float mask = (coef1 != coef1 || coef1 > HM_LOG_COEF_MAX) ? 1.0f : 0.0f;
    const float coef = mask * 1.0f + (1.0f - mask) * coef1;
    // out = coef * w, w = y + m * x
    const float gcoef = hm::torch_order_sum([&](int k) { return gr[k] * (yr[k] + m * xr[k]); }, d1);
    const float gm_w = hm::torch_order_sum([&](int k) { return (gr[k] * coef) * xr[k]; }, d1);
    const float gcoef1 = gcoef * (1.0f - mask);
    const float gcoef0 = (coef0 <= HM_LOG_COEF_MAX) ? gcoef1 : 0.0f;   // clamp(max = 1e4): where(self <= max, grad, 0)
    const float gA = gcoef0 / Q;
    const float gQ = (-gcoef0 * A) / (Q * Q);
    float ga = gA * (1.0f / Q);                               // acosh: 1 / sqrt(a * a - 1)
    const float grad_rad = gQ / (2.0f * Q);                   // sqrt
    ga = ga + (grad_rad * a + grad_rad * a);                  // a * a
    const float gu = (u >= 1.0f) ? ga : 0.0f;                 // clamp(min = 1)
    const float gm = gm_w - gu;                               // both uses of minkowski_dot(x, y)
    const float s0 = hm_g_s0(sign_mode), s1 = hm_g_s1(sign_mode);
    for (int k = 0; k < d1; ++k) {
        const float s = k == 0 ? -s0 : -s1;                   // minkowski_dot = -u
        const float gw = gr[k] * coef;
        gx[t * ldo + k] = gw * m + s * (gm * yr[k]);
        gy[t * ldo + k] = gw + s * (gm * xr[k]);
    }
}

// exp_map (:73-93)
__global__ void hm_rows_exp_map_bwd_kernel(const float* __restrict__ x, const float* __restrict__ v, const float* __restrict__ g,
                                           int64_t ldg, int64_t b, int64_t ld, int d1, float* __restrict__ gx, float* __restrict__ gv,
                                           int64_t ldo)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= b) return;
    const float* xr = x + t * ld;
    const float* vr = v + t * ld;
    const float* gr = g + t * ldg;
    const float s = hm::torch_order_sum([&](int e) { return vr[1 + e] * vr[1 + e]; }, d1 - 1);
    const float nn = hm::exp_map_norm(s);
    const float mask = (nn < 1.0e-6f) ? 1.0f : 0.0f;          // never 1 after the clamp; kept as the reference has it
    const float den = nn + mask;
    const float ch = hm::cosh_c(nn), sh = hm::sinh_c(nn);
    const float keep = 1.0f - mask;
    // out = ch * x + sh * dir, dir = keep * (v / den)
    const float g_ch = hm::torch_order_sum([&](int k) { return gr[k] * xr[k]; }, d1);
    const float g_sh = hm::torch_order_sum([&](int k) { return gr[k] * (keep * (vr[k] / den)); }, d1);
    const float g_den = hm::torch_order_sum([&](int k) { return ((-(gr[k] * sh) * keep) * vr[k]) / (den * den); }, d1);
    const float g_nn = g_ch * sh + g_sh * ch + g_den;         // cosh' = sinh, sinh' = cosh
    const float g_n2 = g_nn / (2.0f * nn);                    // sqrt
    const float g_s = (s >= HM_EXP_N2_MIN) ? g_n2 : 0.0f;           // clamp(min = 1e-8)
    for (int k = 0; k < d1; ++k) {
        gx[t * ldo + k] = gr[k] * ch;
        float o = ((gr[k] * sh) * keep) / den;
        if (k > 0) o = o + (g_s * vr[k] + g_s * vr[k]);
        gv[t * ldo + k] = o;
    }
}

// project_to_hyperboloid (:41-56): x0 is not an input of the result
__global__ void hm_rows_project_bwd_kernel(const float* __restrict__ x, const float* __restrict__ g, int64_t ldg, int64_t b, int64_t ld,
                                           int d1, float c, float* __restrict__ gx, int64_t ldo)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= b) return;
    const float* xr = x + t * ld;
    const float* gr = g + t * ldg;
    float r2 = 0.0f;
    for (int k = 1; k < d1; ++k) r2 = __builtin_fmaf(xr[k], xr[k], r2);
    const float rr = __builtin_sqrtf(r2);
    const float x0 = hm::project_x0(r2, c);
    const float g_sq = gr[0] / (2.0f * x0);                   // sqrt
    const float g_rr = g_sq * (c * rr) + (g_sq * rr) * c;     // (c * n) * n
    const float scale = g_rr / rr;                            // norm: x * (grad / norm), 0 where the norm is 0
    gx[t * ldo] = 0.0f;
    for (int k = 1; k < d1; ++k) gx[t * ldo + k] = gr[k] + (rr == 0.0f ? 0.0f : xr[k] * scale);
}

// batch_distance (:141-210): gX = sum over the rows of Y, gY = sum over the rows of X, on pair tiles
struct BdistCoef {
    const float* G; int64_t ldg; float sqrt_c; int transposed;
    __device__ __forceinline__ float operator()(int64_t i, int64_t j, float u) const
    {
        return hm_g_dist_du(transposed ? G[j * ldg + i] : G[i * ldg + j], u, sqrt_c);
    }
};

template <int NM>
__global__ __launch_bounds__(HM_PT_THREADS) void hm_batch_distance_bwd_kernel(const float* __restrict__ A, int64_t na, int64_t lda,
                                                                              const float* __restrict__ B, int64_t nb, int64_t ldb, int d1,
                                                                              int sign_mode, float* __restrict__ gA, int64_t ldo, BdistCoef coef)
{
    extern __shared__ float hm_pt_lds[];
    hm_pt_grad<NM>(A, na, lda, B, nb, ldb, d1, sign_mode, gA, ldo, coef, hm_pt_lds);
}

template <int NM>
static int hm_bdist_bwd_launch(const float* A, int64_t na, int64_t lda, const float* B, int64_t nb, int64_t ldb, int d1, int sign_mode,
                               float* gA, int64_t ldo, BdistCoef coef, hipStream_t s)
{
    const size_t lds = sizeof(float) * hm_pt_lds_floats(d1, true);
    HM_HIP0(hm_pt_allow_lds(hm_batch_distance_bwd_kernel<NM>, lds));
    hipLaunchKernelGGL(hm_batch_distance_bwd_kernel<NM>, dim3((unsigned)((na + HM_PT - 1) / HM_PT)), dim3(HM_PT_THREADS), lds, s, A, na,
                       lda, B, nb, ldb, d1, sign_mode, gA, ldo, coef);
    HM_HIP0(hipGetLastError());
    return HM_OK;
}

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
extern "C" int hm_batch_distance(const float* X_dev, int64_t n1, const float* Y_dev, int64_t n2, int64_t ld_x, int64_t ld_y, int d1,
                                 float c, int sign_mode, float* out_dev, void* stream)
{
    if (n1 < 0 || n2 < 0 || d1 < 2 || ld_x < d1 || ld_y < d1 || !(c > 0.0f)) return hm_fail(nullptr, HM_E_ARG, "hm_batch_distance: bad arguments");
    if (n1 == 0 || n2 == 0) return HM_OK;
    if (!X_dev || !Y_dev || !out_dev) return hm_fail(nullptr, HM_E_ARG, "hm_batch_distance: NULL pointer");
    const int64_t total = n1 * n2;
    const unsigned blocks = (unsigned)std::min<int64_t>((total + 8 * HM_GATHER - 1) / (8 * HM_GATHER), 8192);
    hipLaunchKernelGGL(hm_dense_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, X_dev, n1, Y_dev, n2, ld_x, ld_y, d1,
                       sqrtf(c), sign_mode, out_dev);
    HM_HIP0(hipGetLastError());
    return HM_OK;
}

extern "C" int hm_rows_minkowski(const float* x_dev, const float* y_dev, int64_t b, int64_t ld, int d1, int sign_mode, float* out_dev,
                                 void* stream)
{
    if (b < 0 || d1 < 2 || ld < d1) return hm_fail(nullptr, HM_E_ARG, "hm_rows_minkowski: bad arguments");
    if (b == 0) return HM_OK;
    hipLaunchKernelGGL(hm_rows_minkowski_kernel, HM_ROW_GRID(b), x_dev, y_dev, b,
                       ld, d1, sign_mode, out_dev);
    HM_HIP0(hipGetLastError());
    return HM_OK;
}

extern "C" int hm_rows_distance(const float* x_dev, const float* y_dev, int64_t b, int64_t ld, int d1, float c, int sign_mode,
                                float* out_dev, void* stream)
{
    if (b < 0 || d1 < 2 || ld < d1 || !(c > 0.0f)) return hm_fail(nullptr, HM_E_ARG, "hm_rows_distance: bad arguments");
    if (b == 0) return HM_OK;
    hipLaunchKernelGGL(hm_rows_distance_kernel, dim3((unsigned)std::min<int64_t>((b + 8 * HM_GATHER - 1) / (8 * HM_GATHER), 8192)), dim3(256), 0, (hipStream_t)stream, x_dev, y_dev, b,
                       ld, d1, sqrtf(c), sign_mode, out_dev);
    HM_HIP0(hipGetLastError());
    return HM_OK;
}

extern "C" int hm_rows_log_map(const float* x_dev, const float* y_dev, int64_t b, int64_t ld, int d1, int sign_mode, float* out_dev,
                               int64_t ld_out, void* stream)
{
    if (b < 0 || d1 < 2 || ld < d1 || ld_out < d1) return hm_fail(nullptr, HM_E_ARG, "hm_rows_log_map: bad arguments");
    if (b == 0) return HM_OK;
    hipLaunchKernelGGL(hm_rows_log_map_kernel, HM_ROW_GRID(b), x_dev, y_dev, b,
                       ld, d1, sign_mode, out_dev, ld_out);
    HM_HIP0(hipGetLastError());
    return HM_OK;
}

extern "C" int hm_rows_exp_map(const float* x_dev, const float* v_dev, int64_t b, int64_t ld, int d1, float* out_dev, int64_t ld_out,
                               void* stream)
{
    if (b < 0 || d1 < 2 || ld < d1 || ld_out < d1) return hm_fail(nullptr, HM_E_ARG, "hm_rows_exp_map: bad arguments");
    if (b == 0) return HM_OK;
    hipLaunchKernelGGL(hm_rows_exp_map_kernel, HM_ROW_GRID(b), x_dev, v_dev, b,
                       ld, d1, out_dev, ld_out);
    HM_HIP0(hipGetLastError());
    return HM_OK;
}

extern "C" int hm_rows_project(const float* x_dev, int64_t b, int64_t ld, int d1, float c, float* out_dev, int64_t ld_out,
                               void* stream)
{
    if (b < 0 || d1 < 2 || ld < d1 || ld_out < d1) return hm_fail(nullptr, HM_E_ARG, "hm_rows_project: bad arguments");
    if (b == 0) return HM_OK;
    hipLaunchKernelGGL(hm_rows_project_kernel, HM_ROW_GRID(b), x_dev, b, ld, d1,
                       c, out_dev, ld_out);
    HM_HIP0(hipGetLastError());
    return HM_OK;
}

extern "C" int hm_batch_distance_bwd(const float* X_dev, int64_t n1, const float* Y_dev, int64_t n2, int64_t ld_x, int64_t ld_y, int d1,
                                     float c, int sign_mode, const float* G_dev, int64_t ld_g, float* gX_dev, float* gY_dev,
                                     int64_t ld_out, void* stream)
{
    if (n1 < 0 || n2 < 0 || d1 < 2 || d1 > 129 || ld_x < d1 || ld_y < d1 || ld_out < d1 || ld_g < n2 || !(c > 0.0f))
        return hm_fail(nullptr, HM_E_ARG, "hm_batch_distance_bwd: bad arguments");
    if (n1 == 0 && n2 == 0) return HM_OK;
    if ((n1 > 0 && n2 > 0 && (!X_dev || !Y_dev || !G_dev)) || (!gX_dev && !gY_dev))
        return hm_fail(nullptr, HM_E_ARG, "hm_batch_distance_bwd: NULL pointer");
    hipStream_t s = (hipStream_t)stream;
    for (int pass = 0; pass < 2; ++pass) {
        float* out = pass ? gY_dev : gX_dev;
        const int64_t na = pass ? n2 : n1, nb = pass ? n1 : n2;
        if (!out || na == 0) continue;
        const BdistCoef coef{G_dev, ld_g, sqrtf(c), pass};
        const float* A = pass ? Y_dev : X_dev;
        const float* B = pass ? X_dev : Y_dev;
        const int64_t lda = pass ? ld_y : ld_x, ldb = pass ? ld_x : ld_y;
        int st;
        if (d1 <= 36) st = hm_bdist_bwd_launch<9>(A, na, lda, B, nb, ldb, d1, sign_mode, out, ld_out, coef, s);
        else if (d1 <= 68) st = hm_bdist_bwd_launch<17>(A, na, lda, B, nb, ldb, d1, sign_mode, out, ld_out, coef, s);
        else st = hm_bdist_bwd_launch<33>(A, na, lda, B, nb, ldb, d1, sign_mode, out, ld_out, coef, s);
        if (st != HM_OK) return st;
    }
    return HM_OK;
}

extern "C" int hm_rows_distance_bwd(const float* x_dev, const float* y_dev, const float* g_dev, int64_t b, int64_t ld, int d1, float c,
                                    int sign_mode, float* gx_dev, float* gy_dev, int64_t ld_out, void* stream)
{
    if (b < 0 || d1 < 2 || ld < d1 || ld_out < d1 || !(c > 0.0f)) return hm_fail(nullptr, HM_E_ARG, "hm_rows_distance_bwd: bad arguments");
    if (b == 0) return HM_OK;
    if (!x_dev || !y_dev || !g_dev || !gx_dev || !gy_dev) return hm_fail(nullptr, HM_E_ARG, "hm_rows_distance_bwd: NULL pointer");
    hipLaunchKernelGGL(hm_rows_u_bwd_kernel, HM_ROW_GRID(b), x_dev, y_dev, g_dev, b, ld, d1, sqrtf(c), sign_mode, 1, gx_dev, gy_dev,
                       ld_out);
    HM_HIP0(hipGetLastError());
    return HM_OK;
}

extern "C" int hm_rows_minkowski_bwd(const float* x_dev, const float* y_dev, const float* g_dev, int64_t b, int64_t ld, int d1,
                                     int sign_mode, float* gx_dev, float* gy_dev, int64_t ld_out, void* stream)
{
    if (b < 0 || d1 < 2 || ld < d1 || ld_out < d1) return hm_fail(nullptr, HM_E_ARG, "hm_rows_minkowski_bwd: bad arguments");
    if (b == 0) return HM_OK;
    if (!x_dev || !y_dev || !g_dev || !gx_dev || !gy_dev) return hm_fail(nullptr, HM_E_ARG, "hm_rows_minkowski_bwd: NULL pointer");
    hipLaunchKernelGGL(hm_rows_u_bwd_kernel, HM_ROW_GRID(b), x_dev, y_dev, g_dev, b, ld, d1, 1.0f, sign_mode, 0, gx_dev, gy_dev,
                       ld_out);
    HM_HIP0(hipGetLastError());
    return HM_OK;
}

extern "C" int hm_rows_log_map_bwd(const float* x_dev, const float* y_dev, const float* g_dev, int64_t ld_g, int64_t b, int64_t ld, int d1,
                                   int sign_mode, float* gx_dev, float* gy_dev, int64_t ld_out, void* stream)
{
    if (b < 0 || d1 < 2 || ld < d1 || ld_g < d1 || ld_out < d1) return hm_fail(nullptr, HM_E_ARG, "hm_rows_log_map_bwd: bad arguments");
    if (b == 0) return HM_OK;
    if (!x_dev || !y_dev || !g_dev || !gx_dev || !gy_dev) return hm_fail(nullptr, HM_E_ARG, "hm_rows_log_map_bwd: NULL pointer");
    hipLaunchKernelGGL(hm_rows_log_map_bwd_kernel, HM_ROW_GRID(b), x_dev, y_dev, g_dev, ld_g, b, ld, d1, sign_mode, gx_dev, gy_dev,
                       ld_out);
    HM_HIP0(hipGetLastError());
    return HM_OK;
}

extern "C" int hm_rows_exp_map_bwd(const float* x_dev, const float* v_dev, const float* g_dev, int64_t ld_g, int64_t b, int64_t ld, int d1,
                                   float* gx_dev, float* gv_dev, int64_t ld_out, void* stream)
{
    if (b < 0 || d1 < 2 || ld < d1 || ld_g < d1 || ld_out < d1) return hm_fail(nullptr, HM_E_ARG, "hm_rows_exp_map_bwd: bad arguments");
    if (b == 0) return HM_OK;
    if (!x_dev || !v_dev || !g_dev || !gx_dev || !gv_dev) return hm_fail(nullptr, HM_E_ARG, "hm_rows_exp_map_bwd: NULL pointer");
    hipLaunchKernelGGL(hm_rows_exp_map_bwd_kernel, HM_ROW_GRID(b), x_dev, v_dev, g_dev, ld_g, b, ld, d1, gx_dev, gv_dev, ld_out);
    HM_HIP0(hipGetLastError());
    return HM_OK;
}

extern "C" int hm_rows_project_bwd(const float* x_dev, const float* g_dev, int64_t ld_g, int64_t b, int64_t ld, int d1, float c,
                                   float* gx_dev, int64_t ld_out, void* stream)
{
    if (b < 0 || d1 < 2 || ld < d1 || ld_g < d1 || ld_out < d1) return hm_fail(nullptr, HM_E_ARG, "hm_rows_project_bwd: bad arguments");
    if (b == 0) return HM_OK;
    if (!x_dev || !g_dev || !gx_dev) return hm_fail(nullptr, HM_E_ARG, "hm_rows_project_bwd: NULL pointer");
    hipLaunchKernelGGL(hm_rows_project_bwd_kernel, HM_ROW_GRID(b), x_dev, g_dev, ld_g, b, ld, d1, c, gx_dev, ld_out);
    HM_HIP0(hipGetLastError());
    return HM_OK;
}
