// hm_poincare.hip -- the Poincare-ball primitives of the reference's embedding/poincare_ball.py and their
// vector-Jacobian products, engine-independent like the Lorentz row primitives of hm_lorentz.hip.
//
// Layout: the lane groups of hm_rowgroup.h, a group per row of width d <= 128.  The vector form is taken
// when every operand allows it; the two conversions move Lorentz rows (RgRow).  Every operand row is read once and every
// result row written once; the backward kernels recompute the row scalars from the inputs.
//
// The derivative is that of the reference's torch expression as torch differentiates it (clamp(min = 1e-8) passes the
// gradient where the norm is >= 1e-8f, the (norm == 0) mask arithmetic is walked back term by term, norm' is 0 at the zero
// vector, atanh' = 1 / (1 - z^2) with its infinity at 1 and its finite values beyond).  No gradient with respect to c.
#include "hm_rowgroup.h"

#pragma clang fp contract(off)

#define HM_PB_CLAMP 1.0e-8f

__device__ __forceinline__ float pb_clamp(float n) { return (n < HM_PB_CLAMP) ? HM_PB_CLAMP : n; }      // NaN propagates

// ------------------------------------------------------------------------------------------------
// mobius_addition (:27-46): out = (A x + B y) / D
// ------------------------------------------------------------------------------------------------
struct PbMob { float x2, y2, xy, A, B, D; };

__device__ __forceinline__ PbMob pb_mob(const RgMap& m, const float (&x)[4], const float (&y)[4], float c)
{
    PbMob q;
    q.x2 = rg_dot(m, x, x);
    q.y2 = rg_dot(m, y, y);
    q.xy = rg_dot(m, x, y);
    const float t = 1.0f + (2.0f * c) * q.xy;
    q.A = t + c * q.y2;
    q.B = 1.0f - c * q.x2;
    q.D = t + ((c * c) * q.x2) * q.y2;
    return q;
}

// vjp of (A x + B y) / D for the upstream row g
__device__ __forceinline__ void pb_mob_bwd(const RgMap& m, const PbMob& q, float c, const float (&x)[4], const float (&y)[4],
                                           const float (&g)[4], float (&gx)[4], float (&gy)[4])
{
    const float gdx = rg_dot(m, g, x), gdy = rg_dot(m, g, y);
    const float gA = gdx / q.D, gB = gdy / q.D;
    const float gD = -((q.A * gdx + q.B * gdy) / q.D) / q.D;  // -sum(g * num) / D^2
    const float gxy = (2.0f * c) * (gA + gD);
    const float gy2 = c * gA + ((c * c) * q.x2) * gD;
    const float gx2 = ((c * c) * q.y2) * gD - c * gB;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float gn = g[j] / q.D;
        gx[j] = (gn * q.A + (2.0f * gx2) * x[j]) + gxy * y[j];
        gy[j] = (gn * q.B + (2.0f * gy2) * y[j]) + gxy * x[j];
    }
}

__global__ __launch_bounds__(HM_RG_THREADS) void hm_pb_mobius_add_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                                         int64_t b, int64_t ld, int d, float c, int lsh, int vec,
                                                                         float* __restrict__ out, int64_t ldo)
{
    const RgMap m = rg_map(lsh, vec, b);
    float xv[4], yv[4], o[4];
    rg_load(x + m.row * ld, d, m, xv);
    rg_load(y + m.row * ld, d, m, yv);
    const PbMob q = pb_mob(m, xv, yv, c);
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = (q.A * xv[j] + q.B * yv[j]) / q.D;
    rg_store(out + m.row * ldo, d, m, o);
}

__global__ __launch_bounds__(HM_RG_THREADS) void hm_pb_mobius_add_bwd_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                                             const float* __restrict__ g, int64_t ldg, int64_t b,
                                                                             int64_t ld, int d, float c, int lsh, int vec,
                                                                             float* __restrict__ gx, float* __restrict__ gy, int64_t ldo)
{
    const RgMap m = rg_map(lsh, vec, b);
    float xv[4], yv[4], gv[4], ox[4], oy[4];
    rg_load(x + m.row * ld, d, m, xv);
    rg_load(y + m.row * ld, d, m, yv);
    rg_load(g + m.row * ldg, d, m, gv);
    const PbMob q = pb_mob(m, xv, yv, c);
    pb_mob_bwd(m, q, c, xv, yv, gv, ox, oy);
    rg_store(gx + m.row * ldo, d, m, ox);
    rg_store(gy + m.row * ldo, d, m, oy);
}

// ------------------------------------------------------------------------------------------------
// distance (:106-126): 2 / sqrt(c) * atanh(sqrt(c) * || (-x) (+) y ||), one value per row
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(HM_RG_THREADS) void hm_pb_distance_kernel(const float* __restrict__ x, const float* __restrict__ y, int64_t b,
                                                                       int64_t ld, int d, float c, float sc, int lsh, int vec,
                                                                       float* __restrict__ out)
{
    const RgMap m = rg_map(lsh, vec, b);
    float xn[4], yv[4], mv[4];
    rg_load(x + m.row * ld, d, m, xn);
    rg_load(y + m.row * ld, d, m, yv);
#pragma unroll
    for (int j = 0; j < 4; ++j) xn[j] = -xn[j];
    const PbMob q = pb_mob(m, xn, yv, c);
#pragma unroll
    for (int j = 0; j < 4; ++j) mv[j] = (q.A * xn[j] + q.B * yv[j]) / q.D;
    const float n = __builtin_sqrtf(rg_dot(m, mv, mv));
    if (m.live && m.sub == 0) out[m.row] = (2.0f / sc) * hm::atanh_c(sc * n);
}

__global__ __launch_bounds__(HM_RG_THREADS) void hm_pb_distance_bwd_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                                           const float* __restrict__ g, int64_t b, int64_t ld, int d,
                                                                           float c, float sc, int lsh, int vec, float* __restrict__ gx,
                                                                           float* __restrict__ gy, int64_t ldo)
{
    const RgMap m = rg_map(lsh, vec, b);
    float xn[4], yv[4], mv[4], gm[4], ox[4], oy[4];
    rg_load(x + m.row * ld, d, m, xn);
    rg_load(y + m.row * ld, d, m, yv);
    const float gr = m.live ? g[m.row] : 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) xn[j] = -xn[j];
    const PbMob q = pb_mob(m, xn, yv, c);
#pragma unroll
    for (int j = 0; j < 4; ++j) mv[j] = (q.A * xn[j] + q.B * yv[j]) / q.D;
    const float n = __builtin_sqrtf(rg_dot(m, mv, mv));
    const float z = sc * n;
    const float gz = (gr * (2.0f / sc)) / (1.0f - z * z);     // atanh
    const float gn = gz * sc;
    const float s = gn / n;                                   // norm: x * (grad / norm), 0 where the norm is 0
#pragma unroll
    for (int j = 0; j < 4; ++j) gm[j] = (n == 0.0f) ? 0.0f : mv[j] * s;
    pb_mob_bwd(m, q, c, xn, yv, gm, ox, oy);
#pragma unroll
    for (int j = 0; j < 4; ++j) ox[j] = -ox[j];
    rg_store(gx + m.row * ldo, d, m, ox);
    rg_store(gy + m.row * ldo, d, m, oy);
}

// ------------------------------------------------------------------------------------------------
// mobius_scalar_mul (:49-65): tanh(r * atanh(sqrt(c) * n)) / (sqrt(c) * n) * x, n = clamp(||x||, 1e-8), r one value per row
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(HM_RG_THREADS) void hm_pb_scalar_mul_kernel(const float* __restrict__ r, const float* __restrict__ x, int64_t b,
                                                                         int64_t ld, int d, float sc, int lsh, int vec,
                                                                         float* __restrict__ out, int64_t ldo)
{
    const RgMap m = rg_map(lsh, vec, b);
    float xv[4], o[4];
    rg_load(x + m.row * ld, d, m, xv);
    const float rr = m.live ? r[m.row] : 0.0f;
    const float a = sc * pb_clamp(__builtin_sqrtf(rg_dot(m, xv, xv)));
    const float q = hm::tanh_c(rr * hm::atanh_c(a)) / a;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = q * xv[j];
    rg_store(out + m.row * ldo, d, m, o);
}

__global__ __launch_bounds__(HM_RG_THREADS) void hm_pb_scalar_mul_bwd_kernel(const float* __restrict__ r, const float* __restrict__ x,
                                                                             const float* __restrict__ g, int64_t ldg, int64_t b,
                                                                             int64_t ld, int d, float sc, int lsh, int vec,
                                                                             float* __restrict__ gr, float* __restrict__ gx, int64_t ldo)
{
    const RgMap m = rg_map(lsh, vec, b);
    float xv[4], gv[4], o[4];
    rg_load(x + m.row * ld, d, m, xv);
    rg_load(g + m.row * ldg, d, m, gv);
    const float rr = m.live ? r[m.row] : 0.0f;
    const float n = __builtin_sqrtf(rg_dot(m, xv, xv));
    const float a = sc * pb_clamp(n);
    const float t = hm::atanh_c(a);
    const float th = hm::tanh_c(rr * t);
    const float q = th / a;
    const float gq = rg_dot(m, gv, xv);
    const float gth = gq / a;
    const float gw = gth * (1.0f - th * th);                  // tanh
    const float ga = (-gq * th) / (a * a) + (gw * rr) / (1.0f - a * a);      // the quotient and atanh
    const float gnc = ga * sc;
    const float gn = (n >= HM_PB_CLAMP) ? gnc : 0.0f;         // clamp(min = 1e-8)
    const float s = gn / n;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = gv[j] * q + ((n == 0.0f) ? 0.0f : xv[j] * s);
    rg_store(gx + m.row * ldo, d, m, o);
    if (m.live && m.sub == 0) gr[m.row] = gw * t;
}

// ------------------------------------------------------------------------------------------------
// exp_map_zero (:68-84) and log_map_zero (:87-103): f(a) / a * v * (1 - mask) + mask * v, a = sqrt(c) * clamp(||v||, 1e-8),
// mask = (||v|| == 0), f = tanh / atanh
// ------------------------------------------------------------------------------------------------
template <int IS_LOG>
__global__ __launch_bounds__(HM_RG_THREADS) void hm_pb_zero_map_kernel(const float* __restrict__ v, int64_t b, int64_t ld, int d, float sc,
                                                                       int lsh, int vec, float* __restrict__ out, int64_t ldo)
{
    const RgMap m = rg_map(lsh, vec, b);
    float vv[4], o[4];
    rg_load(v + m.row * ld, d, m, vv);
    const float n = __builtin_sqrtf(rg_dot(m, vv, vv));
    const float mask = (n == 0.0f) ? 1.0f : 0.0f;
    const float a = sc * pb_clamp(n);
    const float q = (IS_LOG ? hm::atanh_c(a) : hm::tanh_c(a)) / a;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = (q * vv[j]) * (1.0f - mask) + mask * vv[j];
    rg_store(out + m.row * ldo, d, m, o);
}

template <int IS_LOG>
__global__ __launch_bounds__(HM_RG_THREADS) void hm_pb_zero_map_bwd_kernel(const float* __restrict__ v, const float* __restrict__ g,
                                                                           int64_t ldg, int64_t b, int64_t ld, int d, float sc, int lsh,
                                                                           int vec, float* __restrict__ gvo, int64_t ldo)
{
    const RgMap m = rg_map(lsh, vec, b);
    float vv[4], gv[4], gk[4], o[4];
    rg_load(v + m.row * ld, d, m, vv);
    rg_load(g + m.row * ldg, d, m, gv);
    const float n = __builtin_sqrtf(rg_dot(m, vv, vv));
    const float mask = (n == 0.0f) ? 1.0f : 0.0f;
    const float a = sc * pb_clamp(n);
    const float f = IS_LOG ? hm::atanh_c(a) : hm::tanh_c(a);
    const float q = f / a;
#pragma unroll
    for (int j = 0; j < 4; ++j) gk[j] = gv[j] * (1.0f - mask);
    const float gq = rg_dot(m, gk, vv);
    const float gf = gq / a;
    const float gfa = IS_LOG ? gf / (1.0f - a * a) : gf * (1.0f - f * f);
    const float ga = (-gq * f) / (a * a) + gfa;
    const float gnc = ga * sc;
    const float gn = (n >= HM_PB_CLAMP) ? gnc : 0.0f;         // clamp(min = 1e-8)
    const float s = gn / n;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = (gk[j] * q + gv[j] * mask) + ((n == 0.0f) ? 0.0f : vv[j] * s);
    rg_store(gvo + m.row * ldo, d, m, o);
}

// ------------------------------------------------------------------------------------------------
// lorentz_to_poincare (:129-140): x[1:] / (x0 + 1 / sqrt(c)); the Lorentz rows have d + 1 columns
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(HM_RG_THREADS) void hm_pb_l2p_kernel(const float* __restrict__ x, int64_t b, int64_t ld, int d, float sc, int lsh,
                                                                  float* __restrict__ out, int64_t ldo)
{
    const RgMap m = rg_map(lsh, 0, b);
    float o[4];
    const RgRow xr = rg_lrow_load(x + m.row * ld, d, m, 1.0f);
    const float den = xr.t + 1.0f / sc;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = xr.s[j] / den;
    rg_store(out + m.row * ldo, d, m, o);
}

__global__ __launch_bounds__(HM_RG_THREADS) void hm_pb_l2p_bwd_kernel(const float* __restrict__ x, const float* __restrict__ g, int64_t ldg,
                                                                      int64_t b, int64_t ld, int d, float sc, int lsh,
                                                                      float* __restrict__ gx, int64_t ldo)
{
    const RgMap m = rg_map(lsh, 0, b);
    float gv[4];
    const RgRow xr = rg_lrow_load(x + m.row * ld, d, m, 1.0f);
    rg_load(g + m.row * ldg, d, m, gv);
    const float den = xr.t + 1.0f / sc;
    const float dd = den * den;
    RgRow o;
    o.t = rg_sum(m, ((-gv[0] * xr.s[0]) / dd + (-gv[1] * xr.s[1]) / dd) + ((-gv[2] * xr.s[2]) / dd + (-gv[3] * xr.s[3]) / dd));
#pragma unroll
    for (int j = 0; j < 4; ++j) o.s[j] = gv[j] / den;
    rg_lrow_store(gx + m.row * ldo, d, m, o);
}

// ------------------------------------------------------------------------------------------------
// poincare_to_lorentz (:143-163): f = 1 / (1 - c |x|^2); x0 = f (1 + c |x|^2) / k0, x_s = ks f x
//   as shipped: k0 = 2 sqrt(c), ks = 1 (lands on x0^2 - |x_s|^2 = 1 / (4 c));  standard: k0 = sqrt(c), ks = 2
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(HM_RG_THREADS) void hm_pb_p2l_kernel(const float* __restrict__ x, int64_t b, int64_t ld, int d, float c, float k0,
                                                                  float ks, int lsh, float* __restrict__ out, int64_t ldo)
{
    const RgMap m = rg_map(lsh, 0, b);
    float xv[4];
    rg_load(x + m.row * ld, d, m, xv);
    const float cx2 = c * rg_dot(m, xv, xv);
    const float f = 1.0f / (1.0f - cx2);
    const float kf = ks * f;
    RgRow o;
    o.t = (f * (1.0f + cx2)) / k0;
#pragma unroll
    for (int j = 0; j < 4; ++j) o.s[j] = kf * xv[j];
    rg_lrow_store(out + m.row * ldo, d, m, o);
}

__global__ __launch_bounds__(HM_RG_THREADS) void hm_pb_p2l_bwd_kernel(const float* __restrict__ x, const float* __restrict__ g, int64_t ldg,
                                                                      int64_t b, int64_t ld, int d, float c, float k0, float ks, int lsh,
                                                                      float* __restrict__ gx, int64_t ldo)
{
    const RgMap m = rg_map(lsh, 0, b);
    float xv[4], o[4];
    rg_load(x + m.row * ld, d, m, xv);
    const RgRow gr = rg_lrow_load(g + m.row * ldg, d, m, 0.0f);
    const float cx2 = c * rg_dot(m, xv, xv);
    const float f = 1.0f / (1.0f - cx2);
    const float kf = ks * f;
    const float gf = (gr.t * (1.0f + cx2)) / k0 + ks * rg_dot(m, gr.s, xv);
    const float gh = (gr.t * f) / k0;                         // towards 1 + c |x|^2
    const float gx2 = c * gh + c * ((gf * f) * f);            // 1 / den: -grad * result^2, den = 1 - c |x|^2
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = gr.s[j] * kf + (2.0f * gx2) * xv[j];
    rg_store(gx + m.row * ldo, d, m, o);
}

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
struct PbDim { int64_t ld; int need; };                       // a leading dimension and the row width it has to hold
struct PbOp { const void* p; int64_t ld; };

// The preamble every entry point shares, in this order: "bad arguments" (shape, curvature, leading dimensions, flags),
// "NULL pointer", then b == 0.  HM_PB_GO when the entry point goes on to its launch, else the status it returns.
#define HM_PB_GO INT_MIN
static int pb_enter(const char* who, int64_t b, int d, float c, std::initializer_list<PbDim> dims, std::initializer_list<const void*> ptrs,
                    bool flags_ok = true)
{
    bool bad = b < 0 || b > ((int64_t)1 << 31) || d < 1 || d > HM_RG_MAX_D || !(c > 0.0f) || !(c < INFINITY) || !flags_ok;
    for (const PbDim& q : dims) bad = bad || q.ld < q.need;
    if (bad) return hm_fail(nullptr, HM_E_ARG, std::string(who) + ": bad arguments");
    for (const void* p : ptrs)
        if (!p) return hm_fail(nullptr, HM_E_ARG, std::string(who) + ": NULL pointer");
    return b == 0 ? HM_OK : HM_PB_GO;
}

// the 16-byte form: d % 4 == 0 and every operand aligned
static int pb_vec(int d, std::initializer_list<PbOp> ops)
{
    bool vec = (d & 3) == 0;
    for (const PbOp& o : ops) vec = vec && rg_al(o.p, o.ld);
    return vec;
}

#define HM_PB_ENTER(...) \
    if (const int st_ = pb_enter(__VA_ARGS__); st_ != HM_PB_GO) return st_

#define HM_PB_LAUNCH(kernel, ...)                                                                       \
    do {                                                                                                \
        hipLaunchKernelGGL(kernel, rg_grid(b, rg_lsh(d)), dim3(HM_RG_THREADS), 0, (hipStream_t)stream, __VA_ARGS__); \
        HM_HIP0(hipGetLastError());                                                                     \
        return HM_OK;                                                                                   \
    } while (0)

extern "C" int hm_rows_mobius_add(const float* x_dev, const float* y_dev, int64_t b, int64_t ld, int d, float c, float* out_dev,
                                  int64_t ld_out, void* stream)
{
    HM_PB_ENTER("hm_rows_mobius_add", b, d, c, {{ld, d}, {ld_out, d}}, {x_dev, y_dev, out_dev});
    const int vec = pb_vec(d, {{x_dev, ld}, {y_dev, ld}, {out_dev, ld_out}});
    HM_PB_LAUNCH(hm_pb_mobius_add_kernel, x_dev, y_dev, b, ld, d, c, rg_lsh(d), vec, out_dev, ld_out);
}

extern "C" int hm_rows_mobius_add_bwd(const float* x_dev, const float* y_dev, const float* g_dev, int64_t ld_g, int64_t b, int64_t ld,
                                      int d, float c, float* gx_dev, float* gy_dev, int64_t ld_out, void* stream)
{
    HM_PB_ENTER("hm_rows_mobius_add_bwd", b, d, c, {{ld, d}, {ld_g, d}, {ld_out, d}}, {x_dev, y_dev, g_dev, gx_dev, gy_dev});
    const int vec = pb_vec(d, {{x_dev, ld}, {y_dev, ld}, {g_dev, ld_g}, {gx_dev, ld_out}, {gy_dev, ld_out}});
    HM_PB_LAUNCH(hm_pb_mobius_add_bwd_kernel, x_dev, y_dev, g_dev, ld_g, b, ld, d, c, rg_lsh(d), vec, gx_dev, gy_dev, ld_out);
}

extern "C" int hm_rows_poincare_distance(const float* x_dev, const float* y_dev, int64_t b, int64_t ld, int d, float c, float* out_dev,
                                         void* stream)
{
    HM_PB_ENTER("hm_rows_poincare_distance", b, d, c, {{ld, d}}, {x_dev, y_dev, out_dev});
    const int vec = pb_vec(d, {{x_dev, ld}, {y_dev, ld}});
    HM_PB_LAUNCH(hm_pb_distance_kernel, x_dev, y_dev, b, ld, d, c, sqrtf(c), rg_lsh(d), vec, out_dev);
}

extern "C" int hm_rows_poincare_distance_bwd(const float* x_dev, const float* y_dev, const float* g_dev, int64_t b, int64_t ld, int d,
                                             float c, float* gx_dev, float* gy_dev, int64_t ld_out, void* stream)
{
    HM_PB_ENTER("hm_rows_poincare_distance_bwd", b, d, c, {{ld, d}, {ld_out, d}}, {x_dev, y_dev, g_dev, gx_dev, gy_dev});
    const int vec = pb_vec(d, {{x_dev, ld}, {y_dev, ld}, {gx_dev, ld_out}, {gy_dev, ld_out}});
    HM_PB_LAUNCH(hm_pb_distance_bwd_kernel, x_dev, y_dev, g_dev, b, ld, d, c, sqrtf(c), rg_lsh(d), vec, gx_dev, gy_dev, ld_out);
}

extern "C" int hm_rows_mobius_scalar_mul(const float* r_dev, const float* x_dev, int64_t b, int64_t ld, int d, float c, float* out_dev,
                                         int64_t ld_out, void* stream)
{
    HM_PB_ENTER("hm_rows_mobius_scalar_mul", b, d, c, {{ld, d}, {ld_out, d}}, {r_dev, x_dev, out_dev});
    const int vec = pb_vec(d, {{x_dev, ld}, {out_dev, ld_out}});
    HM_PB_LAUNCH(hm_pb_scalar_mul_kernel, r_dev, x_dev, b, ld, d, sqrtf(c), rg_lsh(d), vec, out_dev, ld_out);
}

extern "C" int hm_rows_mobius_scalar_mul_bwd(const float* r_dev, const float* x_dev, const float* g_dev, int64_t ld_g, int64_t b, int64_t ld,
                                             int d, float c, float* gr_dev, float* gx_dev, int64_t ld_out, void* stream)
{
    HM_PB_ENTER("hm_rows_mobius_scalar_mul_bwd", b, d, c, {{ld, d}, {ld_g, d}, {ld_out, d}}, {r_dev, x_dev, g_dev, gr_dev, gx_dev});
    const int vec = pb_vec(d, {{x_dev, ld}, {g_dev, ld_g}, {gx_dev, ld_out}});
    HM_PB_LAUNCH(hm_pb_scalar_mul_bwd_kernel, r_dev, x_dev, g_dev, ld_g, b, ld, d, sqrtf(c), rg_lsh(d), vec, gr_dev, gx_dev, ld_out);
}

static int pb_zero_map(const char* who, int is_log, const float* v_dev, int64_t b, int64_t ld, int d, float c, float* out_dev,
                       int64_t ld_out, void* stream)
{
    HM_PB_ENTER(who, b, d, c, {{ld, d}, {ld_out, d}}, {v_dev, out_dev});
    const int vec = pb_vec(d, {{v_dev, ld}, {out_dev, ld_out}});
    if (is_log) HM_PB_LAUNCH(hm_pb_zero_map_kernel<1>, v_dev, b, ld, d, sqrtf(c), rg_lsh(d), vec, out_dev, ld_out);
    HM_PB_LAUNCH(hm_pb_zero_map_kernel<0>, v_dev, b, ld, d, sqrtf(c), rg_lsh(d), vec, out_dev, ld_out);
}

static int pb_zero_map_bwd(const char* who, int is_log, const float* v_dev, const float* g_dev, int64_t ld_g, int64_t b, int64_t ld, int d,
                           float c, float* gv_dev, int64_t ld_out, void* stream)
{
    HM_PB_ENTER(who, b, d, c, {{ld, d}, {ld_g, d}, {ld_out, d}}, {v_dev, g_dev, gv_dev});
    const int vec = pb_vec(d, {{v_dev, ld}, {g_dev, ld_g}, {gv_dev, ld_out}});
    if (is_log) HM_PB_LAUNCH(hm_pb_zero_map_bwd_kernel<1>, v_dev, g_dev, ld_g, b, ld, d, sqrtf(c), rg_lsh(d), vec, gv_dev, ld_out);
    HM_PB_LAUNCH(hm_pb_zero_map_bwd_kernel<0>, v_dev, g_dev, ld_g, b, ld, d, sqrtf(c), rg_lsh(d), vec, gv_dev, ld_out);
}

extern "C" int hm_rows_exp_map_zero(const float* v_dev, int64_t b, int64_t ld, int d, float c, float* out_dev, int64_t ld_out, void* stream)
{
    return pb_zero_map("hm_rows_exp_map_zero", 0, v_dev, b, ld, d, c, out_dev, ld_out, stream);
}

extern "C" int hm_rows_exp_map_zero_bwd(const float* v_dev, const float* g_dev, int64_t ld_g, int64_t b, int64_t ld, int d, float c,
                                        float* gv_dev, int64_t ld_out, void* stream)
{
    return pb_zero_map_bwd("hm_rows_exp_map_zero_bwd", 0, v_dev, g_dev, ld_g, b, ld, d, c, gv_dev, ld_out, stream);
}

extern "C" int hm_rows_log_map_zero(const float* x_dev, int64_t b, int64_t ld, int d, float c, float* out_dev, int64_t ld_out, void* stream)
{
    return pb_zero_map("hm_rows_log_map_zero", 1, x_dev, b, ld, d, c, out_dev, ld_out, stream);
}

extern "C" int hm_rows_log_map_zero_bwd(const float* x_dev, const float* g_dev, int64_t ld_g, int64_t b, int64_t ld, int d, float c,
                                        float* gx_dev, int64_t ld_out, void* stream)
{
    return pb_zero_map_bwd("hm_rows_log_map_zero_bwd", 1, x_dev, g_dev, ld_g, b, ld, d, c, gx_dev, ld_out, stream);
}

// the two conversions take the scalar form: their Lorentz side starts one column in
extern "C" int hm_rows_lorentz_to_poincare(const float* x_dev, int64_t b, int64_t ld, int d, float c, float* out_dev, int64_t ld_out,
                                           void* stream)
{
    HM_PB_ENTER("hm_rows_lorentz_to_poincare", b, d, c, {{ld, d + 1}, {ld_out, d}}, {x_dev, out_dev});
    HM_PB_LAUNCH(hm_pb_l2p_kernel, x_dev, b, ld, d, sqrtf(c), rg_lsh(d), out_dev, ld_out);
}

extern "C" int hm_rows_lorentz_to_poincare_bwd(const float* x_dev, const float* g_dev, int64_t ld_g, int64_t b, int64_t ld, int d, float c,
                                               float* gx_dev, int64_t ld_out, void* stream)
{
    HM_PB_ENTER("hm_rows_lorentz_to_poincare_bwd", b, d, c, {{ld, d + 1}, {ld_g, d}, {ld_out, d + 1}}, {x_dev, g_dev, gx_dev});
    HM_PB_LAUNCH(hm_pb_l2p_bwd_kernel, x_dev, g_dev, ld_g, b, ld, d, sqrtf(c), rg_lsh(d), gx_dev, ld_out);
}

extern "C" int hm_rows_poincare_to_lorentz(const float* x_dev, int64_t b, int64_t ld, int d, float c, int standard, float* out_dev,
                                           int64_t ld_out, void* stream)
{
    HM_PB_ENTER("hm_rows_poincare_to_lorentz", b, d, c, {{ld, d}, {ld_out, d + 1}}, {x_dev, out_dev}, standard == 0 || standard == 1);
    const float sc = sqrtf(c);
    HM_PB_LAUNCH(hm_pb_p2l_kernel, x_dev, b, ld, d, c, standard ? sc : 2.0f * sc, standard ? 2.0f : 1.0f, rg_lsh(d), out_dev, ld_out);
}

extern "C" int hm_rows_poincare_to_lorentz_bwd(const float* x_dev, const float* g_dev, int64_t ld_g, int64_t b, int64_t ld, int d, float c,
                                               int standard, float* gx_dev, int64_t ld_out, void* stream)
{
    HM_PB_ENTER("hm_rows_poincare_to_lorentz_bwd", b, d, c, {{ld, d}, {ld_g, d + 1}, {ld_out, d}}, {x_dev, g_dev, gx_dev}, standard == 0 || standard == 1);
    const float sc = sqrtf(c);
    HM_PB_LAUNCH(hm_pb_p2l_bwd_kernel, x_dev, g_dev, ld_g, b, ld, d, c, standard ? sc : 2.0f * sc, standard ? 2.0f : 1.0f, rg_lsh(d), gx_dev,
                 ld_out);
}
