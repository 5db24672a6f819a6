// hm_cones.hip -- the hyperbolic entailment cones of Ganea, Becigneul & Hofmann (ICML 2018) as a hinge loss on a Lorentz
// table, forward and backward.  Engine-independent like hm_edgeloss.hip; hm_riemann.hip's sparse path consumes what
// the backward kernel writes.
//
// A loss on an index [B, 2 + K] (hm_index_loss.h: the layout, the skipped slots and samples, the two forms, the backward
// body).  Of a slot's two rows one is the apex a (the parent), the other the child b: role 0 makes the anchor the apex of
// every slot, role 1 the partner.
//   u    = a0 b0 - sum_s a_s b_s                  canonical u of hm_grad_device.h ("lorentz" sign), ATen's summation order
//   n    = sqrt(sum_s a_s^2)                      the apex's spatial norm, the same order
//   w    = sqrt(u^2 - 1),  A = (b0 - a0 u) / (n w)
//   ext  = acos(clamp(A, -A_MAX, A_MAX)),  s = 2 K_ap / n,  aper = asin(min(s, S_MAX)),  m = ext - aper,  E = max(0, m)
//   loss_b = E_0 + sum_{k >= 1 live} max(0, margin - E_k)
// A partner that IS the anchor (same index), a slot with u <= 1 and an apex at the origin (n = 0) are flat: E = 0, no
// gradient.  A clamped factor is a constant; on a line (d = 1) every A is +-1 and counts as clamped.  The gradient of m
// (Euclidean, every coordinate free), with q = -1 / sqrt(1 - A^2) (0 where A is clamped):
//   alpha = q (-a0 / (n w) - A u / w^2),  beta = q (-u / (n w)),  delta = q / (n w),
//   nu    = q (-A / n) + s / (n sqrt(1 - s^2))   (second term 0 where s is clamped)
//   grad_a m = alpha (b0, -b_s) + beta e0 + (nu / n) (0, a_s),   grad_b m = alpha (a0, -a_s) + delta e0
// and the slot's factor sigma = [m > 0] (positive), -[0 < m < margin] (negative).
//
//   forward   u_k (and, role 1, n_k^2) by the whole group (rg_canon_sum), parked in lane i % G, which evaluates the slot once:
//             its share of the loss, summed over the sample's lanes by one butterfly (hm_debug_cone_loss_form), and the four
//             sigma-scaled coefficients of the weights w [B, P, 4]:
//             (alpha, the anchor's e0 factor, nu / n, the partner's e0 factor) sigma;
//   backward  il_bwd on that record.
#include "hm_index_loss.h"
#include "hm_grad_device.h"

#pragma clang fp contract(off)

#define CN_A_MAX 0.99999904632568359375f                      // 1 - 2^-20
#define CN_S_MAX 0.9990234375f                                // 1 - 2^-10

struct CnArgs : IlArgs {                                      // w [B, P] float4: the four coefficients of a slot
    int role;
    float two_k, margin;
};

// One slot: apex (a0, spatial norm^2 nn), child time b0, their u.  Returns the slot's term of the loss and leaves the
// sigma-scaled (alpha, beta, nu / n, delta) in cf.
__device__ __forceinline__ float cn_slot(float a0, float b0, float u, float nn, bool self, bool positive, bool line, float two_k,
                                         float margin, float4& cf)
{
    cf = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const float flat_term = positive ? 0.0f : margin;
    if (self || !(u > 1.0f) || !(nn > 0.0f)) return flat_term;
    const float n = __builtin_sqrtf(nn);
    const float w2 = u * u - 1.0f;
    const float nw = n * __builtin_sqrtf(w2);
    const float A = (b0 - a0 * u) / nw;
    const bool ca = line || !(fabsf(A) <= CN_A_MAX);              // on a line (d = 1) every A is +-1 whatever rounding makes of it
    const float Ac = line ? copysignf(CN_A_MAX, A) : fminf(fmaxf(A, -CN_A_MAX), CN_A_MAX);
    const float sv = two_k / n;
    const bool cs = !(sv < CN_S_MAX);
    const float m = acosf(Ac) - asinf(cs ? CN_S_MAX : sv);
    const float E = m > 0.0f ? m : 0.0f;
    const float term = positive ? E : fmaxf(margin - E, 0.0f);
    const float sigma = positive ? (m > 0.0f ? 1.0f : 0.0f) : ((m > 0.0f && margin - E > 0.0f) ? -1.0f : 0.0f);
    if (sigma == 0.0f) return term;
    const float q = ca ? 0.0f : -1.0f / __builtin_sqrtf(1.0f - Ac * Ac);      // 1 - A^2 as written: the rounding of any fp32 acos'
    const float alpha = q * (-a0 / nw - A * u / w2);
    const float nu = q * (-A / n) + (cs ? 0.0f : sv / (n * __builtin_sqrtf(1.0f - sv * sv)));
    cf = make_float4(sigma * alpha, sigma * (q * (-u / nw)), sigma * (nu / n), sigma * (q / nw));
    return term;
}

__global__ __launch_bounds__(IL_THREADS) void hm_cn_fwd_kernel(const CnArgs a)
{
    const IlWalk wk = il_walk(a);
    const RgMap& q = wk.q;
    const RgSample& s = wk.s;
    const int gid = wk.gid, S = wk.S, P = wk.P, Pp = wk.Pp;
    const int G = 1 << a.lsh, d = a.d, width = G * S;            // width: the lanes that share the sample
    const RgRow x = rg_lrow_load(a.x + (s.ok ? s.iu : 0) * a.ld, d, wk.qa, 1.0f);
    float pr[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) pr[j] = x.s[j] * x.s[j];
    const float nnx = rg_canon_sum(q, d, pr);                    // role 0: the one apex of the sample
    float4* wr = reinterpret_cast<float4*>(a.w) + q.row * (int64_t)P;

    float part = 0.0f;                                           // this lane's terms of the loss
    for (int c0 = 0; c0 < Pp; c0 += G) {
        float myu = 1.0f, myt = 1.0f, mynn = 0.0f;
        bool mylive = false, myself = false;
        for (int kk = 0; kk < G && c0 + kk < Pp; kk += IL_FLIGHT) {
            int64_t idx[IL_FLIGHT];
            bool lv[IL_FLIGHT];
            RgRow y[IL_FLIGHT];
#pragma unroll
            for (int r = 0; r < IL_FLIGHT; ++r) idx[r] = il_index(wk, c0 + kk + r);
            rg_gather<IL_FLIGHT>(a.x, a.ld, a.V, d, q, idx, 1.0f, lv, y);
#pragma unroll
            for (int r = 0; r < IL_FLIGHT; ++r) {
#pragma unroll
                for (int j = 0; j < 4; ++j) pr[j] = x.s[j] * y[r].s[j];
                const float dot = rg_canon_sum(q, d, pr);
                const float t0 = x.t * y[r].t;
                float nn = nnx;
                if (a.role) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) pr[j] = y[r].s[j] * y[r].s[j];
                    nn = rg_canon_sum(q, d, pr);
                }
                if (q.sub == kk + r) { myu = t0 - dot; myt = y[r].t; mynn = nn; mylive = lv[r]; myself = idx[r] == s.iu; }
            }
        }
        const int k = il_partner(wk, c0 + q.sub);
        float4 cf = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (mylive) {
            const float term = a.role ? cn_slot(myt, x.t, myu, mynn, myself, k == 0, d == 1, a.two_k, a.margin, cf)
                                      : cn_slot(x.t, myt, myu, mynn, myself, k == 0, d == 1, a.two_k, a.margin, cf);
            part = part + term;
            if (a.role) { const float e0 = cf.y; cf.y = cf.w; cf.w = e0; }       // .y is the anchor's e0 factor, .w the partner's
        }
        if (q.live && k < P) wr[k] = cf;
    }
    part = rg_wave_sum(width, part);
    if (q.live && q.sub == 0 && gid == 0) a.loss[q.row] = s.ok ? part : 0.0f;
}

struct CnSlot {                                               // the record of a slot: all four terms
    static constexpr bool kCone = true;
    const float4* w;
    int role;
    __device__ __forceinline__ float4 read(int64_t at) const { return w[at]; }
};

__global__ __launch_bounds__(IL_THREADS) void hm_cn_bwd_kernel(const CnArgs a) { il_bwd(a, CnSlot{reinterpret_cast<const float4*>(a.w), a.role}); }

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
static int g_cn_form = 1;

static int cn_args(const char* who, const float* x_dev, int64_t ld, int64_t V, int d1, const int64_t* index_dev, int64_t B, int64_t K,
                   float aperture_k, float margin, int apex_role, const float* weights_dev, CnArgs& a)
{
    a = CnArgs{};
    const bool own_ok = aperture_k > 0.0f && aperture_k < INFINITY && margin >= 0.0f && margin < INFINITY && (apex_role == 0 || apex_role == 1);
    if (int rc = il_args(who, x_dev, ld, V, d1, index_dev, B, K, own_ok, g_cn_form, a)) return rc;
    if (!weights_dev) return hm_fail(nullptr, HM_E_ARG, std::string(who) + ": NULL pointer");
    if (reinterpret_cast<uintptr_t>(weights_dev) & 15u) return hm_fail(nullptr, HM_E_ARG, std::string(who) + ": weights_dev must be 16-byte aligned");
    a.w = const_cast<float*>(weights_dev);
    a.role = apex_role;
    a.two_k = 2.0f * aperture_k; a.margin = margin;
    return HM_OK;
}

// Test / tuning hook: 0 = one lane group per sample, 1 = one wave per sample (the default), for the calls that follow.  The
// two forms differ in the order of the sums over the partners, not in any slot's u, m or coefficients.
extern "C" int hm_debug_cone_loss_form(int form) { return il_set_form("hm_debug_cone_loss_form", form, g_cn_form); }

extern "C" int hm_cone_loss_fwd(const float* x_dev, int64_t ld, int64_t table_rows, int d1, const int64_t* index_dev, int64_t n, int64_t k,
                                float aperture_k, float margin, int apex_role, float* loss_dev, float* weights_dev, void* stream)
{
    CnArgs a;
    if (int rc = cn_args("hm_cone_loss_fwd", x_dev, ld, table_rows, d1, index_dev, n, k, aperture_k, margin, apex_role, weights_dev, a)) return rc;
    if (!loss_dev) return hm_fail(nullptr, HM_E_ARG, "hm_cone_loss_fwd: NULL pointer");
    a.loss = loss_dev;
    return il_launch(hm_cn_fwd_kernel, a, stream);
}

extern "C" int hm_cone_loss_bwd(const float* x_dev, int64_t ld, int64_t table_rows, int d1, const int64_t* index_dev, int64_t n, int64_t k,
                                float aperture_k, float margin, int apex_role, const float* weights_dev, const float* grad_loss_dev,
                                float* values_dev, int64_t* coo_dev, void* stream)
{
    CnArgs a;
    if (int rc = cn_args("hm_cone_loss_bwd", x_dev, ld, table_rows, d1, index_dev, n, k, aperture_k, margin, apex_role, weights_dev, a)) return rc;
    if (!grad_loss_dev || !values_dev || !coo_dev) return hm_fail(nullptr, HM_E_ARG, "hm_cone_loss_bwd: NULL pointer");
    a.gl = grad_loss_dev; a.val = values_dev; a.coo = coo_dev;
    return il_launch(hm_cn_bwd_kernel, a, stream);
}
