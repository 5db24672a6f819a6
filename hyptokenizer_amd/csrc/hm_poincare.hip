// hm_poincare.hip -- the Poincare-ball primitives of the reference's embedding/poincare_ball.py and their
// vector-Jacobian products, engine-independent like the hm_rows_* kernels of hm_rows.hip / hm_rowgrad.hip.
//
// Layout.  A row of width d <= 128 is owned by a group of 16 (d <= 64) or 32 lanes of one wave; a wave
// therefore carries 4 or 2 rows and a load instruction of the wave always covers whole rows.  A lane holds four slots of
// its row:
//   vector form (d % 4 == 0, every leading dimension % 4 == 0, every base 16-byte aligned): slots 4 sub .. 4 sub + 3, one
//     16-byte load / store per operand;
//   scalar form (everything else, and the two conversions, whose Lorentz side is shifted by one column): slots
//     sub + lanes * j, coalesced 4-byte accesses.
// Norms and dots are butterfly sums over the group (__shfl_xor), so every lane ends with the row scalars.  Every operand
// row is read once and every result row written once; the backward kernels recompute the row scalars from the inputs.
//
// The derivative is that of the reference's torch expression as torch differentiates it (clamp(min = 1e-8) passes the
// gradient where the norm is >= 1e-8f, the (norm == 0) mask arithmetic is walked back term by term, norm' is 0 at the zero
// vector, atanh' = 1 / (1 - z^2) with its infinity at 1 and its finite values beyond).  No gradient with respect to c.
#include "hm_common.h"

#pragma clang fp contract(off)

#define HM_PB_MAX_D 128
#define HM_PB_THREADS 256
#define HM_PB_CLAMP 1.0e-8f

struct PbMap {
    int sub, lsh, vec;
    int64_t row;
    bool live;
};

__device__ __forceinline__ PbMap pb_map(int lsh, int vec, int64_t b)
{
    PbMap m;
    const int64_t gl = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    m.lsh = lsh;
    m.vec = vec;
    m.sub = (int)(threadIdx.x & ((1u << lsh) - 1u));
    m.row = gl >> lsh;
    m.live = m.row < b;                                       // dead rows keep zeros and take part in the butterflies only
    return m;
}

__device__ __forceinline__ int pb_idx(const PbMap& m, int j) { return m.vec ? 4 * m.sub + j : m.sub + (j << m.lsh); }

// row m.row of p[., ld] (columns shift .. shift + d - 1) into the lane's slots; slots past d are 0
__device__ __forceinline__ void pb_load(const float* __restrict__ p, int64_t ld, int d, const PbMap& m, float (&v)[4], int shift = 0)
{
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = 0.0f;
    if (!m.live) return;
    const float* r = p + m.row * ld + shift;
    if (m.vec) {
        if (4 * m.sub < d) {
            const float4 t = *reinterpret_cast<const float4*>(r + 4 * m.sub);
            v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = pb_idx(m, j);
            if (k < d) v[j] = r[k];
        }
    }
}

__device__ __forceinline__ void pb_store(float* __restrict__ p, int64_t ld, int d, const PbMap& m, const float (&v)[4], int shift = 0)
{
    if (!m.live) return;
    float* r = p + m.row * ld + shift;
    if (m.vec) {
        if (4 * m.sub < d) *reinterpret_cast<float4*>(r + 4 * m.sub) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = pb_idx(m, j);
            if (k < d) r[k] = v[j];
        }
    }
}

__device__ __forceinline__ float pb_sum(const PbMap& m, float a)
{
    for (int off = (1 << m.lsh) >> 1; off > 0; off >>= 1) a = a + __shfl_xor(a, off, 64);
    return a;
}

__device__ __forceinline__ float pb_dot(const PbMap& m, const float (&a)[4], const float (&b)[4])
{
    return pb_sum(m, (a[0] * b[0] + a[1] * b[1]) + (a[2] * b[2] + a[3] * b[3]));
}

__device__ __forceinline__ float pb_clamp(float n) { return (n < HM_PB_CLAMP) ? HM_PB_CLAMP : n; }      // NaN propagates

// ------------------------------------------------------------------------------------------------
// mobius_addition (:27-46): out = (A x + B y) / D
// ------------------------------------------------------------------------------------------------
struct PbMob { float x2, y2, xy, A, B, D; };

__device__ __forceinline__ PbMob pb_mob(const PbMap& m, const float (&x)[4], const float (&y)[4], float c)
{
    PbMob q;
    q.x2 = pb_dot(m, x, x);
    q.y2 = pb_dot(m, y, y);
    q.xy = pb_dot(m, x, y);
    const float t = 1.0f + (2.0f * c) * q.xy;
    q.A = t + c * q.y2;
    q.B = 1.0f - c * q.x2;
    q.D = t + ((c * c) * q.x2) * q.y2;
    return q;
}

// vjp of (A x + B y) / D for the upstream row g
__device__ __forceinline__ void pb_mob_bwd(const PbMap& m, const PbMob& q, float c, const float (&x)[4], const float (&y)[4],
                                           const float (&g)[4], float (&gx)[4], float (&gy)[4])
{
    const float gdx = pb_dot(m, g, x), gdy = pb_dot(m, g, y);
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

__global__ __launch_bounds__(HM_PB_THREADS) void hm_pb_mobius_add_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                                         int64_t b, int64_t ld, int d, float c, int lsh, int vec,
                                                                         float* __restrict__ out, int64_t ldo)
{
    const PbMap m = pb_map(lsh, vec, b);
    float xv[4], yv[4], o[4];
    pb_load(x, ld, d, m, xv);
    pb_load(y, ld, d, m, yv);
    const PbMob q = pb_mob(m, xv, yv, c);
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = (q.A * xv[j] + q.B * yv[j]) / q.D;
    pb_store(out, ldo, d, m, o);
}

__global__ __launch_bounds__(HM_PB_THREADS) void hm_pb_mobius_add_bwd_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                                             const float* __restrict__ g, int64_t ldg, int64_t b,
                                                                             int64_t ld, int d, float c, int lsh, int vec,
                                                                             float* __restrict__ gx, float* __restrict__ gy, int64_t ldo)
{
    const PbMap m = pb_map(lsh, vec, b);
    float xv[4], yv[4], gv[4], ox[4], oy[4];
    pb_load(x, ld, d, m, xv);
    pb_load(y, ld, d, m, yv);
    pb_load(g, ldg, d, m, gv);
    const PbMob q = pb_mob(m, xv, yv, c);
    pb_mob_bwd(m, q, c, xv, yv, gv, ox, oy);
    pb_store(gx, ldo, d, m, ox);
    pb_store(gy, ldo, d, m, oy);
}

// ------------------------------------------------------------------------------------------------
// distance (:106-126): 2 / sqrt(c) * atanh(sqrt(c) * || (-x) (+) y ||), one value per row
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(HM_PB_THREADS) void hm_pb_distance_kernel(const float* __restrict__ x, const float* __restrict__ y, int64_t b,
                                                                       int64_t ld, int d, float c, float sc, int lsh, int vec,
                                                                       float* __restrict__ out)
{
    const PbMap m = pb_map(lsh, vec, b);
    float xn[4], yv[4], mv[4];
    pb_load(x, ld, d, m, xn);
    pb_load(y, ld, d, m, yv);
#pragma unroll
    for (int j = 0; j < 4; ++j) xn[j] = -xn[j];
    const PbMob q = pb_mob(m, xn, yv, c);
#pragma unroll
    for (int j = 0; j < 4; ++j) mv[j] = (q.A * xn[j] + q.B * yv[j]) / q.D;
    const float n = __builtin_sqrtf(pb_dot(m, mv, mv));
    if (m.live && m.sub == 0) out[m.row] = (2.0f / sc) * hm::atanh_c(sc * n);
}

__global__ __launch_bounds__(HM_PB_THREADS) void hm_pb_distance_bwd_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                                           const float* __restrict__ g, int64_t b, int64_t ld, int d,
                                                                           float c, float sc, int lsh, int vec, float* __restrict__ gx,
                                                                           float* __restrict__ gy, int64_t ldo)
{
    const PbMap m = pb_map(lsh, vec, b);
    float xn[4], yv[4], mv[4], gm[4], ox[4], oy[4];
    pb_load(x, ld, d, m, xn);
    pb_load(y, ld, d, m, yv);
    const float gr = m.live ? g[m.row] : 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) xn[j] = -xn[j];
    const PbMob q = pb_mob(m, xn, yv, c);
#pragma unroll
    for (int j = 0; j < 4; ++j) mv[j] = (q.A * xn[j] + q.B * yv[j]) / q.D;
    const float n = __builtin_sqrtf(pb_dot(m, mv, mv));
    const float z = sc * n;
    const float gz = (gr * (2.0f / sc)) / (1.0f - z * z);     // atanh
    const float gn = gz * sc;
    const float s = gn / n;                                   // norm: x * (grad / norm), 0 where the norm is 0
#pragma unroll
    for (int j = 0; j < 4; ++j) gm[j] = (n == 0.0f) ? 0.0f : mv[j] * s;
    pb_mob_bwd(m, q, c, xn, yv, gm, ox, oy);
#pragma unroll
    for (int j = 0; j < 4; ++j) ox[j] = -ox[j];
    pb_store(gx, ldo, d, m, ox);
    pb_store(gy, ldo, d, m, oy);
}

// ------------------------------------------------------------------------------------------------
// mobius_scalar_mul (:49-65): tanh(r * atanh(sqrt(c) * n)) / (sqrt(c) * n) * x, n = clamp(||x||, 1e-8), r one value per row
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(HM_PB_THREADS) void hm_pb_scalar_mul_kernel(const float* __restrict__ r, const float* __restrict__ x, int64_t b,
                                                                         int64_t ld, int d, float sc, int lsh, int vec,
                                                                         float* __restrict__ out, int64_t ldo)
{
    const PbMap m = pb_map(lsh, vec, b);
    float xv[4], o[4];
    pb_load(x, ld, d, m, xv);
    const float rr = m.live ? r[m.row] : 0.0f;
    const float a = sc * pb_clamp(__builtin_sqrtf(pb_dot(m, xv, xv)));
    const float q = hm::tanh_c(rr * hm::atanh_c(a)) / a;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = q * xv[j];
    pb_store(out, ldo, d, m, o);
}

__global__ __launch_bounds__(HM_PB_THREADS) void hm_pb_scalar_mul_bwd_kernel(const float* __restrict__ r, const float* __restrict__ x,
                                                                             const float* __restrict__ g, int64_t ldg, int64_t b,
                                                                             int64_t ld, int d, float sc, int lsh, int vec,
                                                                             float* __restrict__ gr, float* __restrict__ gx, int64_t ldo)
{
    const PbMap m = pb_map(lsh, vec, b);
    float xv[4], gv[4], o[4];
    pb_load(x, ld, d, m, xv);
    pb_load(g, ldg, d, m, gv);
    const float rr = m.live ? r[m.row] : 0.0f;
    const float n = __builtin_sqrtf(pb_dot(m, xv, xv));
    const float a = sc * pb_clamp(n);
    const float t = hm::atanh_c(a);
    const float th = hm::tanh_c(rr * t);
    const float q = th / a;
    const float gq = pb_dot(m, gv, xv);
    const float gth = gq / a;
    const float gw = gth * (1.0f - th * th);                  // tanh
    const float ga = (-gq * th) / (a * a) + (gw * rr) / (1.0f - a * a);      // the quotient and atanh
    const float gnc = ga * sc;
    const float gn = (n >= HM_PB_CLAMP) ? gnc : 0.0f;         // clamp(min = 1e-8)
    const float s = gn / n;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = gv[j] * q + ((n == 0.0f) ? 0.0f : xv[j] * s);
    pb_store(gx, ldo, d, m, o);
    if (m.live && m.sub == 0) gr[m.row] = gw * t;
}

// ------------------------------------------------------------------------------------------------
// exp_map_zero (:68-84) and log_map_zero (:87-103): f(a) / a * v * (1 - mask) + mask * v, a = sqrt(c) * clamp(||v||, 1e-8),
// mask = (||v|| == 0), f = tanh / atanh
// ------------------------------------------------------------------------------------------------
template <int IS_LOG>
__global__ __launch_bounds__(HM_PB_THREADS) void hm_pb_zero_map_kernel(const float* __restrict__ v, int64_t b, int64_t ld, int d, float sc,
                                                                       int lsh, int vec, float* __restrict__ out, int64_t ldo)
{
    const PbMap m = pb_map(lsh, vec, b);
    float vv[4], o[4];
    pb_load(v, ld, d, m, vv);
    const float n = __builtin_sqrtf(pb_dot(m, vv, vv));
    const float mask = (n == 0.0f) ? 1.0f : 0.0f;
    const float a = sc * pb_clamp(n);
    const float q = (IS_LOG ? hm::atanh_c(a) : hm::tanh_c(a)) / a;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = (q * vv[j]) * (1.0f - mask) + mask * vv[j];
    pb_store(out, ldo, d, m, o);
}

template <int IS_LOG>
__global__ __launch_bounds__(HM_PB_THREADS) void hm_pb_zero_map_bwd_kernel(const float* __restrict__ v, const float* __restrict__ g,
                                                                           int64_t ldg, int64_t b, int64_t ld, int d, float sc, int lsh,
                                                                           int vec, float* __restrict__ gvo, int64_t ldo)
{
    const PbMap m = pb_map(lsh, vec, b);
    float vv[4], gv[4], gk[4], o[4];
    pb_load(v, ld, d, m, vv);
    pb_load(g, ldg, d, m, gv);
    const float n = __builtin_sqrtf(pb_dot(m, vv, vv));
    const float mask = (n == 0.0f) ? 1.0f : 0.0f;
    const float a = sc * pb_clamp(n);
    const float f = IS_LOG ? hm::atanh_c(a) : hm::tanh_c(a);
    const float q = f / a;
#pragma unroll
    for (int j = 0; j < 4; ++j) gk[j] = gv[j] * (1.0f - mask);
    const float gq = pb_dot(m, gk, vv);
    const float gf = gq / a;
    const float gfa = IS_LOG ? gf / (1.0f - a * a) : gf * (1.0f - f * f);
    const float ga = (-gq * f) / (a * a) + gfa;
    const float gnc = ga * sc;
    const float gn = (n >= HM_PB_CLAMP) ? gnc : 0.0f;         // clamp(min = 1e-8)
    const float s = gn / n;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = (gk[j] * q + gv[j] * mask) + ((n == 0.0f) ? 0.0f : vv[j] * s);
    pb_store(gvo, ldo, d, m, o);
}

// ------------------------------------------------------------------------------------------------
// lorentz_to_poincare (:129-140): x[1:] / (x0 + 1 / sqrt(c)); the Lorentz rows have d + 1 columns
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(HM_PB_THREADS) void hm_pb_l2p_kernel(const float* __restrict__ x, int64_t b, int64_t ld, int d, float sc, int lsh,
                                                                  float* __restrict__ out, int64_t ldo)
{
    const PbMap m = pb_map(lsh, 0, b);
    float xs[4], o[4];
    pb_load(x, ld, d, m, xs, 1);
    const float den = (m.live ? x[m.row * ld] : 1.0f) + 1.0f / sc;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = xs[j] / den;
    pb_store(out, ldo, d, m, o);
}

__global__ __launch_bounds__(HM_PB_THREADS) void hm_pb_l2p_bwd_kernel(const float* __restrict__ x, const float* __restrict__ g, int64_t ldg,
                                                                      int64_t b, int64_t ld, int d, float sc, int lsh,
                                                                      float* __restrict__ gx, int64_t ldo)
{
    const PbMap m = pb_map(lsh, 0, b);
    float xs[4], gv[4], o[4];
    pb_load(x, ld, d, m, xs, 1);
    pb_load(g, ldg, d, m, gv);
    const float den = (m.live ? x[m.row * ld] : 1.0f) + 1.0f / sc;
    const float dd = den * den;
    const float g0 = pb_sum(m, ((-gv[0] * xs[0]) / dd + (-gv[1] * xs[1]) / dd) + ((-gv[2] * xs[2]) / dd + (-gv[3] * xs[3]) / dd));
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = gv[j] / den;
    pb_store(gx, ldo, d, m, o, 1);
    if (m.live && m.sub == 0) gx[m.row * ldo] = g0;
}

// ------------------------------------------------------------------------------------------------
// poincare_to_lorentz (:143-163): f = 1 / (1 - c |x|^2); x0 = f (1 + c |x|^2) / k0, x_s = ks f x
//   as shipped: k0 = 2 sqrt(c), ks = 1 (lands on x0^2 - |x_s|^2 = 1 / (4 c));  standard: k0 = sqrt(c), ks = 2
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(HM_PB_THREADS) void hm_pb_p2l_kernel(const float* __restrict__ x, int64_t b, int64_t ld, int d, float c, float k0,
                                                                  float ks, int lsh, float* __restrict__ out, int64_t ldo)
{
    const PbMap m = pb_map(lsh, 0, b);
    float xv[4], o[4];
    pb_load(x, ld, d, m, xv);
    const float cx2 = c * pb_dot(m, xv, xv);
    const float f = 1.0f / (1.0f - cx2);
    const float kf = ks * f;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = kf * xv[j];
    pb_store(out, ldo, d, m, o, 1);
    if (m.live && m.sub == 0) out[m.row * ldo] = (f * (1.0f + cx2)) / k0;
}

__global__ __launch_bounds__(HM_PB_THREADS) void hm_pb_p2l_bwd_kernel(const float* __restrict__ x, const float* __restrict__ g, int64_t ldg,
                                                                      int64_t b, int64_t ld, int d, float c, float k0, float ks, int lsh,
                                                                      float* __restrict__ gx, int64_t ldo)
{
    const PbMap m = pb_map(lsh, 0, b);
    float xv[4], gs[4], o[4];
    pb_load(x, ld, d, m, xv);
    pb_load(g, ldg, d, m, gs, 1);
    const float g0 = m.live ? g[m.row * ldg] : 0.0f;
    const float cx2 = c * pb_dot(m, xv, xv);
    const float f = 1.0f / (1.0f - cx2);
    const float kf = ks * f;
    const float gf = (g0 * (1.0f + cx2)) / k0 + ks * pb_dot(m, gs, xv);
    const float gh = (g0 * f) / k0;                           // towards 1 + c |x|^2
    const float gx2 = c * gh + c * ((gf * f) * f);            // 1 / den: -grad * result^2, den = 1 - c |x|^2
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = gs[j] * kf + (2.0f * gx2) * xv[j];
    pb_store(gx, ldo, d, m, o);
}

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
static inline bool pb_bad_c(float c) { return !(c > 0.0f) || !(c < INFINITY); }
static inline bool pb_bad_shape(int64_t b, int d) { return b < 0 || b > ((int64_t)1 << 31) || d < 1 || d > HM_PB_MAX_D; }
static inline int pb_lsh(int d) { return d <= 64 ? 4 : 5; }      // log2 of the lanes per row: 4 slots each cover d <= 128
static inline bool pb_al(const void* p, int64_t ld) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0 && (ld & 3) == 0; }
static inline dim3 pb_grid(int64_t b, int lsh) { return dim3((unsigned)(((b << lsh) + HM_PB_THREADS - 1) / HM_PB_THREADS)); }

#define HM_PB_LAUNCH(kernel, ...)                                                                       \
    do {                                                                                                \
        hipLaunchKernelGGL(kernel, pb_grid(b, lsh), dim3(HM_PB_THREADS), 0, (hipStream_t)stream, __VA_ARGS__); \
        HM_HIP0(hipGetLastError());                                                                     \
        return HM_OK;                                                                                   \
    } while (0)

extern "C" int hm_rows_mobius_add(const float* x_dev, const float* y_dev, int64_t b, int64_t ld, int d, float c, float* out_dev,
                                  int64_t ld_out, void* stream)
{
    if (pb_bad_shape(b, d) || ld < d || ld_out < d || pb_bad_c(c)) return hm_fail(nullptr, HM_E_ARG, "hm_rows_mobius_add: bad arguments");
    if (!x_dev || !y_dev || !out_dev) return hm_fail(nullptr, HM_E_ARG, "hm_rows_mobius_add: NULL pointer");
    if (b == 0) return HM_OK;
    const int lsh = pb_lsh(d), vec = (d & 3) == 0 && pb_al(x_dev, ld) && pb_al(y_dev, ld) && pb_al(out_dev, ld_out);
    HM_PB_LAUNCH(hm_pb_mobius_add_kernel, x_dev, y_dev, b, ld, d, c, lsh, vec, out_dev, ld_out);
}

extern "C" int hm_rows_mobius_add_bwd(const float* x_dev, const float* y_dev, const float* g_dev, int64_t ld_g, int64_t b, int64_t ld,
                                      int d, float c, float* gx_dev, float* gy_dev, int64_t ld_out, void* stream)
{
    if (pb_bad_shape(b, d) || ld < d || ld_g < d || ld_out < d || pb_bad_c(c))
        return hm_fail(nullptr, HM_E_ARG, "hm_rows_mobius_add_bwd: bad arguments");
    if (!x_dev || !y_dev || !g_dev || !gx_dev || !gy_dev) return hm_fail(nullptr, HM_E_ARG, "hm_rows_mobius_add_bwd: NULL pointer");
    if (b == 0) return HM_OK;
    const int lsh = pb_lsh(d), vec = (d & 3) == 0 && pb_al(x_dev, ld) && pb_al(y_dev, ld) && pb_al(g_dev, ld_g) &&
                                     pb_al(gx_dev, ld_out) && pb_al(gy_dev, ld_out);
    HM_PB_LAUNCH(hm_pb_mobius_add_bwd_kernel, x_dev, y_dev, g_dev, ld_g, b, ld, d, c, lsh, vec, gx_dev, gy_dev, ld_out);
}

extern "C" int hm_rows_poincare_distance(const float* x_dev, const float* y_dev, int64_t b, int64_t ld, int d, float c, float* out_dev,
                                         void* stream)
{
    if (pb_bad_shape(b, d) || ld < d || pb_bad_c(c)) return hm_fail(nullptr, HM_E_ARG, "hm_rows_poincare_distance: bad arguments");
    if (!x_dev || !y_dev || !out_dev) return hm_fail(nullptr, HM_E_ARG, "hm_rows_poincare_distance: NULL pointer");
    if (b == 0) return HM_OK;
    const int lsh = pb_lsh(d), vec = (d & 3) == 0 && pb_al(x_dev, ld) && pb_al(y_dev, ld);
    HM_PB_LAUNCH(hm_pb_distance_kernel, x_dev, y_dev, b, ld, d, c, sqrtf(c), lsh, vec, out_dev);
}

extern "C" int hm_rows_poincare_distance_bwd(const float* x_dev, const float* y_dev, const float* g_dev, int64_t b, int64_t ld, int d,
                                             float c, float* gx_dev, float* gy_dev, int64_t ld_out, void* stream)
{
    if (pb_bad_shape(b, d) || ld < d || ld_out < d || pb_bad_c(c))
        return hm_fail(nullptr, HM_E_ARG, "hm_rows_poincare_distance_bwd: bad arguments");
    if (!x_dev || !y_dev || !g_dev || !gx_dev || !gy_dev) return hm_fail(nullptr, HM_E_ARG, "hm_rows_poincare_distance_bwd: NULL pointer");
    if (b == 0) return HM_OK;
    const int lsh = pb_lsh(d), vec = (d & 3) == 0 && pb_al(x_dev, ld) && pb_al(y_dev, ld) && pb_al(gx_dev, ld_out) && pb_al(gy_dev, ld_out);
    HM_PB_LAUNCH(hm_pb_distance_bwd_kernel, x_dev, y_dev, g_dev, b, ld, d, c, sqrtf(c), lsh, vec, gx_dev, gy_dev, ld_out);
}

extern "C" int hm_rows_mobius_scalar_mul(const float* r_dev, const float* x_dev, int64_t b, int64_t ld, int d, float c, float* out_dev,
                                         int64_t ld_out, void* stream)
{
    if (pb_bad_shape(b, d) || ld < d || ld_out < d || pb_bad_c(c)) return hm_fail(nullptr, HM_E_ARG, "hm_rows_mobius_scalar_mul: bad arguments");
    if (!r_dev || !x_dev || !out_dev) return hm_fail(nullptr, HM_E_ARG, "hm_rows_mobius_scalar_mul: NULL pointer");
    if (b == 0) return HM_OK;
    const int lsh = pb_lsh(d), vec = (d & 3) == 0 && pb_al(x_dev, ld) && pb_al(out_dev, ld_out);
    HM_PB_LAUNCH(hm_pb_scalar_mul_kernel, r_dev, x_dev, b, ld, d, sqrtf(c), lsh, vec, out_dev, ld_out);
}

extern "C" int hm_rows_mobius_scalar_mul_bwd(const float* r_dev, const float* x_dev, const float* g_dev, int64_t ld_g, int64_t b, int64_t ld,
                                             int d, float c, float* gr_dev, float* gx_dev, int64_t ld_out, void* stream)
{
    if (pb_bad_shape(b, d) || ld < d || ld_g < d || ld_out < d || pb_bad_c(c))
        return hm_fail(nullptr, HM_E_ARG, "hm_rows_mobius_scalar_mul_bwd: bad arguments");
    if (!r_dev || !x_dev || !g_dev || !gr_dev || !gx_dev) return hm_fail(nullptr, HM_E_ARG, "hm_rows_mobius_scalar_mul_bwd: NULL pointer");
    if (b == 0) return HM_OK;
    const int lsh = pb_lsh(d), vec = (d & 3) == 0 && pb_al(x_dev, ld) && pb_al(g_dev, ld_g) && pb_al(gx_dev, ld_out);
    HM_PB_LAUNCH(hm_pb_scalar_mul_bwd_kernel, r_dev, x_dev, g_dev, ld_g, b, ld, d, sqrtf(c), lsh, vec, gr_dev, gx_dev, ld_out);
}

static int pb_zero_map(const char* who, int is_log, const float* v_dev, int64_t b, int64_t ld, int d, float c, float* out_dev,
                       int64_t ld_out, void* stream)
{
    if (pb_bad_shape(b, d) || ld < d || ld_out < d || pb_bad_c(c)) return hm_fail(nullptr, HM_E_ARG, std::string(who) + ": bad arguments");
    if (!v_dev || !out_dev) return hm_fail(nullptr, HM_E_ARG, std::string(who) + ": NULL pointer");
    if (b == 0) return HM_OK;
    const int lsh = pb_lsh(d), vec = (d & 3) == 0 && pb_al(v_dev, ld) && pb_al(out_dev, ld_out);
    if (is_log) HM_PB_LAUNCH(hm_pb_zero_map_kernel<1>, v_dev, b, ld, d, sqrtf(c), lsh, vec, out_dev, ld_out);
    HM_PB_LAUNCH(hm_pb_zero_map_kernel<0>, v_dev, b, ld, d, sqrtf(c), lsh, vec, out_dev, ld_out);
}

static int pb_zero_map_bwd(const char* who, int is_log, const float* v_dev, const float* g_dev, int64_t ld_g, int64_t b, int64_t ld, int d,
                           float c, float* gv_dev, int64_t ld_out, void* stream)
{
    if (pb_bad_shape(b, d) || ld < d || ld_g < d || ld_out < d || pb_bad_c(c))
        return hm_fail(nullptr, HM_E_ARG, std::string(who) + ": bad arguments");
    if (!v_dev || !g_dev || !gv_dev) return hm_fail(nullptr, HM_E_ARG, std::string(who) + ": NULL pointer");
    if (b == 0) return HM_OK;
    const int lsh = pb_lsh(d), vec = (d & 3) == 0 && pb_al(v_dev, ld) && pb_al(g_dev, ld_g) && pb_al(gv_dev, ld_out);
    if (is_log) HM_PB_LAUNCH(hm_pb_zero_map_bwd_kernel<1>, v_dev, g_dev, ld_g, b, ld, d, sqrtf(c), lsh, vec, gv_dev, ld_out);
    HM_PB_LAUNCH(hm_pb_zero_map_bwd_kernel<0>, v_dev, g_dev, ld_g, b, ld, d, sqrtf(c), lsh, vec, gv_dev, ld_out);
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

extern "C" int hm_rows_lorentz_to_poincare(const float* x_dev, int64_t b, int64_t ld, int d, float c, float* out_dev, int64_t ld_out,
                                           void* stream)
{
    if (pb_bad_shape(b, d) || ld < d + 1 || ld_out < d || pb_bad_c(c))
        return hm_fail(nullptr, HM_E_ARG, "hm_rows_lorentz_to_poincare: bad arguments");
    if (!x_dev || !out_dev) return hm_fail(nullptr, HM_E_ARG, "hm_rows_lorentz_to_poincare: NULL pointer");
    if (b == 0) return HM_OK;
    const int lsh = pb_lsh(d);
    HM_PB_LAUNCH(hm_pb_l2p_kernel, x_dev, b, ld, d, sqrtf(c), lsh, out_dev, ld_out);
}

extern "C" int hm_rows_lorentz_to_poincare_bwd(const float* x_dev, const float* g_dev, int64_t ld_g, int64_t b, int64_t ld, int d, float c,
                                               float* gx_dev, int64_t ld_out, void* stream)
{
    if (pb_bad_shape(b, d) || ld < d + 1 || ld_g < d || ld_out < d + 1 || pb_bad_c(c))
        return hm_fail(nullptr, HM_E_ARG, "hm_rows_lorentz_to_poincare_bwd: bad arguments");
    if (!x_dev || !g_dev || !gx_dev) return hm_fail(nullptr, HM_E_ARG, "hm_rows_lorentz_to_poincare_bwd: NULL pointer");
    if (b == 0) return HM_OK;
    const int lsh = pb_lsh(d);
    HM_PB_LAUNCH(hm_pb_l2p_bwd_kernel, x_dev, g_dev, ld_g, b, ld, d, sqrtf(c), lsh, gx_dev, ld_out);
}

extern "C" int hm_rows_poincare_to_lorentz(const float* x_dev, int64_t b, int64_t ld, int d, float c, int standard, float* out_dev,
                                           int64_t ld_out, void* stream)
{
    if (pb_bad_shape(b, d) || ld < d || ld_out < d + 1 || pb_bad_c(c) || (standard != 0 && standard != 1))
        return hm_fail(nullptr, HM_E_ARG, "hm_rows_poincare_to_lorentz: bad arguments");
    if (!x_dev || !out_dev) return hm_fail(nullptr, HM_E_ARG, "hm_rows_poincare_to_lorentz: NULL pointer");
    if (b == 0) return HM_OK;
    const int lsh = pb_lsh(d);
    const float sc = sqrtf(c);
    HM_PB_LAUNCH(hm_pb_p2l_kernel, x_dev, b, ld, d, c, standard ? sc : 2.0f * sc, standard ? 2.0f : 1.0f, lsh, out_dev, ld_out);
}

extern "C" int hm_rows_poincare_to_lorentz_bwd(const float* x_dev, const float* g_dev, int64_t ld_g, int64_t b, int64_t ld, int d, float c,
                                               int standard, float* gx_dev, int64_t ld_out, void* stream)
{
    if (pb_bad_shape(b, d) || ld < d || ld_g < d + 1 || ld_out < d || pb_bad_c(c) || (standard != 0 && standard != 1))
        return hm_fail(nullptr, HM_E_ARG, "hm_rows_poincare_to_lorentz_bwd: bad arguments");
    if (!x_dev || !g_dev || !gx_dev) return hm_fail(nullptr, HM_E_ARG, "hm_rows_poincare_to_lorentz_bwd: NULL pointer");
    if (b == 0) return HM_OK;
    const int lsh = pb_lsh(d);
    const float sc = sqrtf(c);
    HM_PB_LAUNCH(hm_pb_p2l_bwd_kernel, x_dev, g_dev, ld_g, b, ld, d, c, standard ? sc : 2.0f * sc, standard ? 2.0f : 1.0f, lsh, gx_dev,
                 ld_out);
}
