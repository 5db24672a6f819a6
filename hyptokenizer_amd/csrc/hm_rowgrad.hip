// hm_rowgrad.hip -- vector-Jacobian products of the row-wise Lorentz primitives (embedding/lorentz_model.py of the
// reference), engine-independent like the hm_rows_* forward kernels of hm_rows.hip.
//
// Each kernel walks the reference's torch expression backwards operation by operation (clamp masks, the
// mask * a + (1 - mask) * b arithmetic of log_map / exp_map, acosh' = 1 / sqrt(a^2 - 1) with its infinities), and
// recomputes the forward intermediates with the canonical helpers of hm_device_math.h, so they carry the forward
// kernels' bits.  One thread per row, as the forward log_map / exp_map / project kernels.
#include "hm_grad_device.h"

#pragma clang fp contract(off)

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
    const float a = hm::clamp_min_one(u);
    const float A = hm::acosh_c(a);
    const float rad = a * a - 1.0f;
    const float Q = __builtin_sqrtf(rad);
    const float coef0 = A / Q;
    float coef1 = coef0;
    if (coef1 == coef1 && coef1 > 1.0e4f) coef1 = 1.0e4f;
    const float mask = (coef1 != coef1 || coef1 > 1.0e4f) ? 1.0f : 0.0f;
    const float coef = mask * 1.0f + (1.0f - mask) * coef1;
    // out = coef * w, w = y + m * x
    const float gcoef = hm::torch_order_sum([&](int k) { return gr[k] * (yr[k] + m * xr[k]); }, d1);
    const float gm_w = hm::torch_order_sum([&](int k) { return (gr[k] * coef) * xr[k]; }, d1);
    const float gcoef1 = gcoef * (1.0f - mask);
    const float gcoef0 = (coef0 <= 1.0e4f) ? gcoef1 : 0.0f;   // clamp(max = 1e4): where(self <= max, grad, 0)
    const float gA = gcoef0 / Q;
    const float gQ = (-gcoef0 * A) / (Q * Q);
    float ga = gA * (1.0f / __builtin_sqrtf(a * a - 1.0f));   // acosh
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
    float n2 = s;
    if (n2 == n2 && n2 < 1.0e-8f) n2 = 1.0e-8f;
    const float nn = __builtin_sqrtf(n2);
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
    const float g_s = (s >= 1.0e-8f) ? g_n2 : 0.0f;           // clamp(min = 1e-8)
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
    const float x0 = __builtin_sqrtf(1.0f + (c * rr) * rr);
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

#define HM_ROWGRAD_GRID(b) dim3((unsigned)(((b) + 127) / 128)), dim3(128), 0, (hipStream_t)stream

extern "C" int hm_rows_distance_bwd(const float* x_dev, const float* y_dev, const float* g_dev, int64_t b, int64_t ld, int d1, float c,
                                    int sign_mode, float* gx_dev, float* gy_dev, int64_t ld_out, void* stream)
{
    if (b < 0 || d1 < 2 || ld < d1 || ld_out < d1 || !(c > 0.0f)) return hm_fail(nullptr, HM_E_ARG, "hm_rows_distance_bwd: bad arguments");
    if (b == 0) return HM_OK;
    if (!x_dev || !y_dev || !g_dev || !gx_dev || !gy_dev) return hm_fail(nullptr, HM_E_ARG, "hm_rows_distance_bwd: NULL pointer");
    hipLaunchKernelGGL(hm_rows_u_bwd_kernel, HM_ROWGRAD_GRID(b), x_dev, y_dev, g_dev, b, ld, d1, sqrtf(c), sign_mode, 1, gx_dev, gy_dev,
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
    hipLaunchKernelGGL(hm_rows_u_bwd_kernel, HM_ROWGRAD_GRID(b), x_dev, y_dev, g_dev, b, ld, d1, 1.0f, sign_mode, 0, gx_dev, gy_dev,
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
    hipLaunchKernelGGL(hm_rows_log_map_bwd_kernel, HM_ROWGRAD_GRID(b), x_dev, y_dev, g_dev, ld_g, b, ld, d1, sign_mode, gx_dev, gy_dev,
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
    hipLaunchKernelGGL(hm_rows_exp_map_bwd_kernel, HM_ROWGRAD_GRID(b), x_dev, v_dev, g_dev, ld_g, b, ld, d1, gx_dev, gv_dev, ld_out);
    HM_HIP0(hipGetLastError());
    return HM_OK;
}

extern "C" int hm_rows_project_bwd(const float* x_dev, const float* g_dev, int64_t ld_g, int64_t b, int64_t ld, int d1, float c,
                                   float* gx_dev, int64_t ld_out, void* stream)
{
    if (b < 0 || d1 < 2 || ld < d1 || ld_g < d1 || ld_out < d1) return hm_fail(nullptr, HM_E_ARG, "hm_rows_project_bwd: bad arguments");
    if (b == 0) return HM_OK;
    if (!x_dev || !g_dev || !gx_dev) return hm_fail(nullptr, HM_E_ARG, "hm_rows_project_bwd: NULL pointer");
    hipLaunchKernelGGL(hm_rows_project_bwd_kernel, HM_ROWGRAD_GRID(b), x_dev, g_dev, ld_g, b, ld, d1, c, gx_dev, ld_out);
    HM_HIP0(hipGetLastError());
    return HM_OK;
}
