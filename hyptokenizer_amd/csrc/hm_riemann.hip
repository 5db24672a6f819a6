// hm_riemann.hip -- one fused, in-place Riemannian optimiser step (RSGD, Riemannian Adam) for rows on the unit
// hyperboloid <x, x> = -1, <a, b> = -a0 b0 + sum_k ak bk; engine-independent like the hm_rows_* kernels.
//
// Layout: the Lorentz rows of hm_rowgroup.h, a lane group per row of d1 <= 129 columns.  Every operand row
// is read once and every result row written once, in place; a group lives inside one wave, whose loads of a row all precede
// its stores in program order.  No atomics, no LDS, no workspace.
//
// The step (formulas fixed by DESIGN.md 5.16, not by lorentz_model.exp_map / parallel_transport / riemannian_gradient):
//   u  = h + <x, h> x, h = (-g0, g1, ...)                               Riemannian gradient
//   RSGD:  m+ = mu m + (1 - dampening) u, dir = m+ or u + mu m+ (Nesterov); without momentum dir = u
//   RAdam: m+ = b1 m + (1 - b1) u, v+ = b2 v + (1 - b2) <u, u>, dir = (m+ / bc1) / (sqrt(v+ / bc2) + eps)
//   s  = -lr dir, n = sqrt(max(<s, s>, 0)), y_s = cosh(n) x_s + (sinh(n) / n) s_s (factor 1 at n = 0),
//   y0 = sqrt(1 + |y_s|^2)                                              retraction, time coordinate recomputed
//   w  = m+ + <y, m+> / (1 - <x, y>) (x + y), m' = w + <y, w> y         transport and re-projection
#include "hm_rowgroup.h"

#pragma clang fp contract(off)

#define HM_RO_SGD 0                                           // RSGD without momentum: no state
#define HM_RO_SGD_MOM 1
#define HM_RO_ADAM 2

struct RoArgs {
    float* x;
    const float* g;
    float* m;
    float* v;
    const int64_t* rows;
    int64_t ld_x, ld_g, ld_m, n, table_rows;
    int d, lsh, nesterov;
    float lr, k_m, k_u;                                       // m+ = k_m m + k_u u: (mu, 1 - dampening) or (b1, 1 - b1)
    float b2, omb2, eps, bc1, bc2;
};

// <a, b> = -a0 b0 + sum_k ak bk
__device__ __forceinline__ float ro_ldot(const RgMap& m, const RgRow& a, const RgRow& b) { return rg_dot(m, a.s, b.s) - a.t * b.t; }

template <int OPT>
__global__ __launch_bounds__(HM_RG_THREADS) void hm_ro_step_kernel(const RoArgs a)
{
    // group t steps gradient row t; its x, m and v rows are row t of the table, or row rows[t] when indexed.  An index
    // outside the table is not live: it never writes
    RgMap q = rg_map(a.lsh, 0, a.n);
    const int64_t t = q.row;
    int64_t row = t;
    if (q.live && a.rows) {
        row = a.rows[t];
        q.live = rg_in(row, a.table_rows);
    }
    const int d = a.d;
    float* xr = a.x + row * a.ld_x;
    float* mr = a.m + row * a.ld_m;
    const RgRow x = rg_lrow_load(xr, d, q, 1.0f);             // dead rows keep the origin
    const RgRow g = rg_lrow_load(a.g + t * a.ld_g, d, q, 0.0f);
    RgRow m = {0.0f, {0.0f, 0.0f, 0.0f, 0.0f}}, h = g, u, s, y, w;
    float vv = 0.0f;
    if (OPT != HM_RO_SGD) m = rg_lrow_load(mr, d, q, 0.0f);
    if (OPT == HM_RO_ADAM && q.live) vv = a.v[row];

    // Riemannian gradient: h = (-g0, g_s), u = h + <x, h> x
    h.t = -g.t;
    const float xh = ro_ldot(q, x, h);
    u.t = h.t + xh * x.t;
#pragma unroll
    for (int j = 0; j < 4; ++j) u.s[j] = h.s[j] + xh * x.s[j];

    // moments and direction; s = -lr dir
    if (OPT == HM_RO_SGD) {
        m = u;
        s.t = -a.lr * u.t;
#pragma unroll
        for (int j = 0; j < 4; ++j) s.s[j] = -a.lr * u.s[j];
    } else if (OPT == HM_RO_SGD_MOM) {
        m.t = a.k_m * m.t + a.k_u * u.t;
#pragma unroll
        for (int j = 0; j < 4; ++j) m.s[j] = a.k_m * m.s[j] + a.k_u * u.s[j];
        if (a.nesterov) {
            s.t = -a.lr * (u.t + a.k_m * m.t);
#pragma unroll
            for (int j = 0; j < 4; ++j) s.s[j] = -a.lr * (u.s[j] + a.k_m * m.s[j]);
        } else {
            s.t = -a.lr * m.t;
#pragma unroll
            for (int j = 0; j < 4; ++j) s.s[j] = -a.lr * m.s[j];
        }
    } else {
        m.t = a.k_m * m.t + a.k_u * u.t;
#pragma unroll
        for (int j = 0; j < 4; ++j) m.s[j] = a.k_m * m.s[j] + a.k_u * u.s[j];
        const float uu = ro_ldot(q, u, u);                    // the row's squared Riemannian norm
        vv = a.b2 * vv + a.omb2 * uu;
        const float den = __builtin_sqrtf(vv / a.bc2) + a.eps;
        s.t = -a.lr * ((m.t / a.bc1) / den);
#pragma unroll
        for (int j = 0; j < 4; ++j) s.s[j] = -a.lr * ((m.s[j] / a.bc1) / den);
    }

    // retraction: Exp_x(s), then the time coordinate from the spatial part
    const float n2 = ro_ldot(q, s, s);
    const float nn = __builtin_sqrtf((n2 < 0.0f) ? 0.0f : n2);   // NaN propagates
    float ch, sh;
    hm::cosh_sinh_c(nn, ch, sh);
    const float coef = (nn > 0.0f) ? sh / nn : 1.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) y.s[j] = ch * x.s[j] + coef * s.s[j];
    y.t = __builtin_sqrtf(1.0f + rg_dot(q, y.s, y.s));
    rg_lrow_store(xr, d, q, y);
    if (OPT == HM_RO_SGD) return;

    // transport of m+ from x to y, re-projected onto the tangent space at y
    const float ym = ro_ldot(q, y, m);
    const float xy = ro_ldot(q, x, y);
    const float f = ym / (1.0f - xy);
    w.t = m.t + f * (x.t + y.t);
#pragma unroll
    for (int j = 0; j < 4; ++j) w.s[j] = m.s[j] + f * (x.s[j] + y.s[j]);
    const float yw = ro_ldot(q, y, w);
    w.t = w.t + yw * y.t;
#pragma unroll
    for (int j = 0; j < 4; ++j) w.s[j] = w.s[j] + yw * y.s[j];
    rg_lrow_store(mr, d, q, w);
    if (OPT == HM_RO_ADAM && q.live && q.sub == 0) a.v[row] = vv;
}

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
static inline bool ro_unit(float b) { return b >= 0.0f && b < 1.0f; }            // false for NaN
static inline bool ro_bad_common(int64_t ld_x, int64_t ld_g, int64_t n, int64_t table_rows, int d1, float lr, bool dense)
{
    if (rg_bad_lrow(d1, ld_x) || ld_g < d1) return true;
    if (n < 0 || n > ((int64_t)1 << 31) || table_rows < 0 || (dense && n != table_rows)) return true;
    return !(lr >= 0.0f) || !(lr < INFINITY);
}

template <int OPT>
static int ro_launch(const RoArgs& a, void* stream)
{
    hipLaunchKernelGGL(hm_ro_step_kernel<OPT>, rg_grid(a.n, a.lsh), dim3(HM_RG_THREADS), 0, (hipStream_t)stream, a);
    HM_HIP0(hipGetLastError());
    return HM_OK;
}

extern "C" int hm_rsgd_step(float* x_dev, int64_t ld_x, const float* g_dev, int64_t ld_g, float* m_dev, int64_t ld_m,
                            const int64_t* rows_dev, int64_t n, int64_t table_rows, int d1, float lr, float momentum, float dampening,
                            int nesterov, void* stream)
{
    if (ro_bad_common(ld_x, ld_g, n, table_rows, d1, lr, rows_dev == nullptr) || !ro_unit(momentum) || !ro_unit(dampening) ||
        (nesterov != 0 && nesterov != 1))
        return hm_fail(nullptr, HM_E_ARG, "hm_rsgd_step: bad arguments");
    if (!x_dev || !g_dev) return hm_fail(nullptr, HM_E_ARG, "hm_rsgd_step: NULL pointer");
    const bool mom = momentum != 0.0f;
    if (mom != (m_dev != nullptr)) return hm_fail(nullptr, HM_E_ARG, "hm_rsgd_step: the momentum buffer is given exactly when momentum != 0");
    if (mom && ld_m < d1) return hm_fail(nullptr, HM_E_ARG, "hm_rsgd_step: bad arguments");
    if (n == 0) return HM_OK;
    RoArgs a = {};
    a.x = x_dev; a.g = g_dev; a.m = m_dev; a.rows = rows_dev;
    a.ld_x = ld_x; a.ld_g = ld_g; a.ld_m = ld_m; a.n = n; a.table_rows = table_rows;
    a.d = d1 - 1; a.lsh = rg_lsh(a.d); a.nesterov = nesterov;
    a.lr = lr; a.k_m = momentum; a.k_u = (float)(1.0 - (double)dampening);
    return mom ? ro_launch<HM_RO_SGD_MOM>(a, stream) : ro_launch<HM_RO_SGD>(a, stream);
}

extern "C" int hm_radam_step(float* x_dev, int64_t ld_x, const float* g_dev, int64_t ld_g, float* m_dev, int64_t ld_m, float* v_dev,
                             const int64_t* rows_dev, int64_t n, int64_t table_rows, int d1, float lr, float beta1, float beta2,
                             float eps, float bc1, float bc2, void* stream)
{
    if (ro_bad_common(ld_x, ld_g, n, table_rows, d1, lr, rows_dev == nullptr) || ld_m < d1 || !ro_unit(beta1) || !ro_unit(beta2) ||
        !(bc1 > 0.0f) || !(bc1 < INFINITY) || !(bc2 > 0.0f) || !(bc2 < INFINITY) || !(eps >= 0.0f) || !(eps < INFINITY))
        return hm_fail(nullptr, HM_E_ARG, "hm_radam_step: bad arguments");
    if (!x_dev || !g_dev || !m_dev || !v_dev) return hm_fail(nullptr, HM_E_ARG, "hm_radam_step: NULL pointer");
    if (n == 0) return HM_OK;
    RoArgs a = {};
    a.x = x_dev; a.g = g_dev; a.m = m_dev; a.v = v_dev; a.rows = rows_dev;
    a.ld_x = ld_x; a.ld_g = ld_g; a.ld_m = ld_m; a.n = n; a.table_rows = table_rows;
    a.d = d1 - 1; a.lsh = rg_lsh(a.d);
    a.lr = lr; a.k_m = beta1; a.k_u = (float)(1.0 - (double)beta1);
    a.b2 = beta2; a.omb2 = (float)(1.0 - (double)beta2); a.eps = eps; a.bc1 = bc1; a.bc2 = bc2;
    return ro_launch<HM_RO_ADAM>(a, stream);
}
