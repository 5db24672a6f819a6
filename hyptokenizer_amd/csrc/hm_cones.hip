// hm_cones.hip -- the hyperbolic entailment cones of Ganea, Becigneul & Hofmann (ICML 2018) as a hinge loss on a Lorentz
// table, forward and backward.  Engine-independent like hm_edgeloss.hip, whose index layout, lane-group walk
// and sparse output it shares; hm_riemann.hip's sparse path consumes what the backward kernel writes.
//
// index [B, 2 + K] int64: column 0 the anchor, column 1 the positive, columns 2.. the negatives.  Partner k = 0 is the
// positive, partner k >= 1 the negative of column 1 + k; P = 1 + K partners.  A negative outside [0, V) is a skipped slot, a
// sample whose anchor or positive lies outside [0, V) is skipped whole; neither is ever dereferenced.  Of a slot's two rows
// one is the apex a (the parent), the other the child b: role 0 makes the anchor the apex of every slot, role 1 the partner.
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
// Layout: hm_edgeloss.hip's.  A group keeps the anchor row in registers and walks partners in flights of CN_FLIGHT rows
// (rg_gather); form 0 gives a sample to a GROUP, form 1 to a WAVE whose S groups take the partners k = g, g + S, ...
// (hm_debug_cone_loss_form, rg_split_map).  "Position" i of group g is partner k = g + S i.
//   forward   u_k (and, role 1, n_k^2) by the whole group (rg_canon_sum), parked in lane i % G, which evaluates the slot once:
//             its share of the loss, summed over the sample's lanes by one butterfly, and the four sigma-scaled coefficients
//             of the weights w [B, P, 4]:  (alpha, the anchor's e0 factor, nu / n, the partner's e0 factor) sigma;
//   backward  re-gathers the partner rows and forms scaled row sums only: the anchor's sum carried in registers across the
//             partner loop and folded across the groups, every value row [B, 2 + K, d1] and every COO index written exactly
//             once: no atomics, no LDS, no workspace but w.
#include "hm_rowgroup.h"
#include "hm_grad_device.h"

#pragma clang fp contract(off)

#define CN_THREADS HM_RG_WAVE                                 // one wave per block: 4 or 2 samples, so that small batches spread
#define CN_FLIGHT 4                                           // partner rows in flight per group
#define CN_A_MAX 0.99999904632568359375f                      // 1 - 2^-20
#define CN_S_MAX 0.9990234375f                                // 1 - 2^-10

struct CnArgs {
    const float* x;
    const int64_t* index;
    float4* w;                                                // [B, P]: the four coefficients of a slot
    float* loss;                                              // forward: [B]
    const float* gl;                                          // backward: upstream gradient of loss [B]
    float* val;                                               // backward: [B * (2 + K), d1]
    int64_t* coo;                                             // backward: [B * (2 + K)]
    int64_t ld, B, V;
    int K, d, lsh, split, role;
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

__global__ __launch_bounds__(CN_THREADS) void hm_cn_fwd_kernel(const CnArgs a)
{
    int gid, S;
    const RgMap q = rg_split_map(a.lsh, a.split, a.B, gid, S);
    const RgSample s = rg_sample(a.index, a.K, a.V, q);
    const int G = 1 << a.lsh, d = a.d, P = 1 + a.K;
    const int Pp = (P + S - 1) / S, width = G * S;               // positions per group; lanes that share the sample
    RgMap qa = q;
    qa.live = s.ok;
    const RgRow x = rg_lrow_load(a.x + (s.ok ? s.iu : 0) * a.ld, d, qa, 1.0f);
    float pr[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) pr[j] = x.s[j] * x.s[j];
    const float nnx = rg_canon_sum(q, d, pr);                    // role 0: the one apex of the sample
    float4* wr = a.w + q.row * (int64_t)P;

    float part = 0.0f;                                           // this lane's terms of the loss
    for (int c0 = 0; c0 < Pp; c0 += G) {
        float myu = 1.0f, myt = 1.0f, mynn = 0.0f;
        bool mylive = false, myself = false;
        for (int kk = 0; kk < G && c0 + kk < Pp; kk += CN_FLIGHT) {
            int64_t idx[CN_FLIGHT];
            bool lv[CN_FLIGHT];
            RgRow y[CN_FLIGHT];
#pragma unroll
            for (int r = 0; r < CN_FLIGHT; ++r) {
                const int k = gid + S * (c0 + kk + r);
                idx[r] = (s.ok && k < P) ? s.ix[1 + k] : -1;
            }
            rg_gather<CN_FLIGHT>(a.x, a.ld, a.V, d, q, idx, 1.0f, lv, y);
#pragma unroll
            for (int r = 0; r < CN_FLIGHT; ++r) {
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
        const int k = gid + S * (c0 + q.sub);
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

__global__ __launch_bounds__(CN_THREADS) void hm_cn_bwd_kernel(const CnArgs a)
{
    int gid, S;
    const RgMap q = rg_split_map(a.lsh, a.split, a.B, gid, S);
    const RgSample s = rg_sample(a.index, a.K, a.V, q);
    const int d = a.d, d1 = a.d + 1, P = 1 + a.K;
    const int Pp = (P + S - 1) / S;
    RgMap qa = q;
    qa.live = s.ok;
    const RgRow x = rg_lrow_load(a.x + (s.ok ? s.iu : 0) * a.ld, d, qa, 0.0f);
    RgRow acc = {0.0f, {0.0f, 0.0f, 0.0f, 0.0f}};              // the anchor's sum over this group's partners
    float own = 0.0f;                                          // role 0: the sum of the factors of the anchor's own spatial part
    const float g = q.live ? a.gl[q.row] : 0.0f;
    const float4* wr = a.w + q.row * (int64_t)P;
    const int64_t slot0 = q.row * (int64_t)(2 + a.K);
    const int64_t fill = s.ok ? s.iu : 0;                     // COO index of a skipped slot: its value row is zero
    for (int i0 = 0; i0 < Pp; i0 += CN_FLIGHT) {
        int64_t idx[CN_FLIGHT];
        bool lv[CN_FLIGHT];
        float4 cf[CN_FLIGHT];
        RgRow y[CN_FLIGHT];
#pragma unroll
        for (int r = 0; r < CN_FLIGHT; ++r) {
            const int k = gid + S * (i0 + r);
            idx[r] = (s.ok && k < P) ? s.ix[1 + k] : -1;
            cf[r] = rg_in(idx[r], a.V) ? wr[k] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
        rg_gather<CN_FLIGHT>(a.x, a.ld, a.V, d, q, idx, 0.0f, lv, y);
#pragma unroll
        for (int r = 0; r < CN_FLIGHT; ++r) {
            const int k = gid + S * (i0 + r);
            if (k >= P) continue;
            acc.t = acc.t + (cf[r].x * y[r].t + cf[r].y);
            const float ga = g * cf[r].x, gz = a.role ? g * cf[r].z : 0.0f;
            if (!a.role) own = own + cf[r].z;
            RgRow v;
            v.t = lv[r] ? ga * x.t + g * cf[r].w : 0.0f;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                acc.s[j] = acc.s[j] - cf[r].x * y[r].s[j];
                v.s[j] = lv[r] ? gz * y[r].s[j] - ga * x.s[j] : 0.0f;
            }
            rg_lrow_store(a.val + (slot0 + 1 + k) * d1, d, q, v);
            if (q.live && q.sub == 0) a.coo[slot0 + 1 + k] = lv[r] ? idx[r] : fill;
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) acc.s[j] = acc.s[j] + own * x.s[j];
    rg_fold_groups(a.lsh, S, acc);                             // form 1: group 0 stores the anchor's row
    RgRow v;
    v.t = s.ok ? g * acc.t : 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) v.s[j] = s.ok ? g * acc.s[j] : 0.0f;
    RgMap q0 = q;
    q0.live = q.live && gid == 0;
    rg_lrow_store(a.val + slot0 * d1, d, q0, v);
    if (q0.live && q.sub == 0) a.coo[slot0] = fill;
}

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
static int g_cn_form = 1;

static int cn_args(const char* who, const float* x_dev, int64_t ld, int64_t V, int d1, const int64_t* index_dev, int64_t B, int64_t K,
                   float aperture_k, float margin, int apex_role, const float* weights_dev, CnArgs& a)
{
    if (rg_bad_table(d1, ld, V) || B < 0 || B >= ((int64_t)1 << 31) || K < 0 || K > ((int64_t)1 << 20) ||
        (B + 1) * (K + 2) > ((int64_t)1 << 40) || !(aperture_k > 0.0f) || !(aperture_k < INFINITY) || !(margin >= 0.0f) ||
        !(margin < INFINITY) || (apex_role != 0 && apex_role != 1))
        return hm_fail(nullptr, HM_E_ARG, std::string(who) + ": bad arguments");
    if (!x_dev || !index_dev || !weights_dev) return hm_fail(nullptr, HM_E_ARG, std::string(who) + ": NULL pointer");
    if (reinterpret_cast<uintptr_t>(weights_dev) & 15u) return hm_fail(nullptr, HM_E_ARG, std::string(who) + ": weights_dev must be 16-byte aligned");
    a = CnArgs{};
    a.x = x_dev; a.index = index_dev;
    a.w = reinterpret_cast<float4*>(const_cast<float*>(weights_dev));
    a.ld = ld; a.B = B; a.V = V;
    a.K = (int)K; a.d = d1 - 1; a.lsh = rg_lsh(a.d); a.split = g_cn_form; a.role = apex_role;
    a.two_k = 2.0f * aperture_k; a.margin = margin;
    return HM_OK;
}

// Test / tuning hook: 0 = one lane group per sample, 1 = one wave per sample (the default), for the calls that follow.  The
// two forms differ in the order of the sums over the partners, not in any slot's u, m or coefficients.
extern "C" int hm_debug_cone_loss_form(int form)
{
    if (form != 0 && form != 1) return hm_fail(nullptr, HM_E_ARG, "hm_debug_cone_loss_form: form must be 0 or 1");
    g_cn_form = form;
    return HM_OK;
}

extern "C" int hm_cone_loss_fwd(const float* x_dev, int64_t ld, int64_t table_rows, int d1, const int64_t* index_dev, int64_t n, int64_t k,
                                float aperture_k, float margin, int apex_role, float* loss_dev, float* weights_dev, void* stream)
{
    CnArgs a;
    if (int rc = cn_args("hm_cone_loss_fwd", x_dev, ld, table_rows, d1, index_dev, n, k, aperture_k, margin, apex_role, weights_dev, a)) return rc;
    if (!loss_dev) return hm_fail(nullptr, HM_E_ARG, "hm_cone_loss_fwd: NULL pointer");
    if (n == 0) return HM_OK;
    a.loss = loss_dev;
    hipLaunchKernelGGL(hm_cn_fwd_kernel, rg_split_grid(a.B, a.lsh, a.split, CN_THREADS), dim3(CN_THREADS), 0, (hipStream_t)stream, a);
    HM_HIP0(hipGetLastError());
    return HM_OK;
}

extern "C" int hm_cone_loss_bwd(const float* x_dev, int64_t ld, int64_t table_rows, int d1, const int64_t* index_dev, int64_t n, int64_t k,
                                float aperture_k, float margin, int apex_role, const float* weights_dev, const float* grad_loss_dev,
                                float* values_dev, int64_t* coo_dev, void* stream)
{
    CnArgs a;
    if (int rc = cn_args("hm_cone_loss_bwd", x_dev, ld, table_rows, d1, index_dev, n, k, aperture_k, margin, apex_role, weights_dev, a)) return rc;
    if (!grad_loss_dev || !values_dev || !coo_dev) return hm_fail(nullptr, HM_E_ARG, "hm_cone_loss_bwd: NULL pointer");
    if (n == 0) return HM_OK;
    a.gl = grad_loss_dev; a.val = values_dev; a.coo = coo_dev;
    hipLaunchKernelGGL(hm_cn_bwd_kernel, rg_split_grid(a.B, a.lsh, a.split, CN_THREADS), dim3(CN_THREADS), 0, (hipStream_t)stream, a);
    HM_HIP0(hipGetLastError());
    return HM_OK;
}
