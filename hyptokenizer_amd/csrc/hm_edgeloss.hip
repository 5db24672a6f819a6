// hm_edgeloss.hip -- the graph-embedding objective of Nickel & Kiela (2017, 2018) on a Lorentz table, forward and backward
// (DESIGN.md 5.17).  Engine-independent like hm_riemann.hip, whose sparse path consumes what the backward kernel writes.
//
// index [B, 2 + K] int64: column 0 the anchor u, column 1 the positive, columns 2.. the negatives.  Partner k = 0 is the
// positive, partner k >= 1 the negative of column 1 + k; P = 1 + K partners.  A negative outside [0, V) is a skipped slot, a
// sample whose anchor or positive lies outside [0, V) is skipped whole; neither is ever dereferenced.
//   u_k    = x_u0 x_k0 - sum_s x_us x_ks          canonical u of hm_grad_device.h ("lorentz" sign), ATen's summation order;
//                                                 a partner that IS the anchor (same index) has u_k = 1 by definition
//   d_k    = acosh(max(u_k, 1)) / sqrt(c)         hm::dist_from_u: the bits of hm_rows_distance
//   loss_b = d_0 + log sum_{k live} exp(-d_k)     shifted by max_k(-d_k) = -min_k d_k
//   a_k    = ([k = 0] - p_k) / (sqrt(c) sqrt(u_k^2 - 1)), p = softmax(-d) over the live slots; a_k = 0 where u_k <= 1
//   grad   anchor: sum_k a_k (x_k0, -x_ks);  partner k: a_k (x_u0, -x_us)            (Euclidean, -J x = (x0, -xs))
//
// Layout: Lorentz rows gathered on the lane groups of hm_rowgroup.h.  A group keeps the anchor row in
// registers and walks partners in flights of EL_FLIGHT rows (rg_gather's).  Two forms (hm_debug_edge_loss_form, rg_split_map):
//   form 0  one GROUP per sample: the group walks all P partners;
//   form 1  one WAVE per sample: its S groups take the partners k = g, g + S, g + 2 S, ... and combine d_min, the sum of
//           exponentials and the anchor's gradient by butterflies across the wave -- S times the waves, P / S the walk.
// Below, "position" i of group g is partner k = g + S i (form 0: S = 1, g = 0).
//   forward   pass 1: u_k by the whole group (rg_canon_sum: hm_halfwave_sum's chains laid over the group's slots), parked in
//             lane k % G, which evaluates d_k once and stores u_k to the weights w [B, P];
//             pass 2: every lane re-reads the u_k IT stored, sums exp(-(d_k - d_min)), one butterfly;
//             pass 3: the same lanes turn their u_k into a_k in place.
//   backward  re-gathers the partner rows, carries the anchor's sum in registers across the partner loop, and writes every
//             value row [B, 2 + K, d1] and every COO index exactly once: no atomics, no workspace but w.
#include "hm_rowgroup.h"
#include "hm_grad_device.h"

#pragma clang fp contract(off)

#define EL_THREADS HM_RG_WAVE                                 // one wave per block: 4 or 2 samples, so that small batches spread
#define EL_FLIGHT 4                                           // partner rows in flight per group

struct ElArgs {
    const float* x;
    const int64_t* index;
    float* w;                                                 // [B, P]: u_k inside the forward kernel, a_k once it has finished
    float* loss;                                              // forward: [B]
    const float* gl;                                          // backward: upstream gradient of loss [B]
    float* val;                                               // backward: [B * (2 + K), d1]
    int64_t* coo;                                             // backward: [B * (2 + K)]
    int64_t ld, B, V;
    int K, d, lsh, split;
    float sqrt_c;
};

__global__ __launch_bounds__(EL_THREADS) void hm_el_fwd_kernel(const ElArgs a)
{
    int gid, S;
    const RgMap q = rg_split_map(a.lsh, a.split, a.B, gid, S);
    const RgSample s = rg_sample(a.index, a.K, a.V, q);
    const int G = 1 << a.lsh, d = a.d, P = 1 + a.K;
    const int Pp = (P + S - 1) / S, width = G * S;               // positions per group; lanes that share the sample
    RgMap qa = q;
    qa.live = s.ok;
    // The rows of this kernel are written out, not RgRow / rg_gather: with the rows in structs the compiler emits the same
    // 4508 instructions in a schedule that measures 0.6 - 0.9 % slower.
    const float* xr = a.x + (s.ok ? s.iu : 0) * a.ld;
    float xs[4];
    const float x0 = s.ok ? xr[0] : 1.0f;
    rg_load(xr + 1, d, qa, xs);
    float* wr = a.w + q.row * (int64_t)P;

    // pass 1: u_k, parked in lane k % G; d_min and d_0
    float dmin = INFINITY, d0 = 0.0f;
    for (int c0 = 0; c0 < Pp; c0 += G) {
        float myu = 1.0f;
        bool mylive = false;
        for (int kk = 0; kk < G && c0 + kk < Pp; kk += EL_FLIGHT) {
            int64_t idx[EL_FLIGHT];
            bool lv[EL_FLIGHT];
            float y0[EL_FLIGHT], ys[EL_FLIGHT][4];
#pragma unroll
            for (int r = 0; r < EL_FLIGHT; ++r) {
                const int k = gid + S * (c0 + kk + r);
                idx[r] = (s.ok && k < P) ? s.ix[1 + k] : -1;
                lv[r] = rg_in(idx[r], a.V);
            }
#pragma unroll
            for (int r = 0; r < EL_FLIGHT; ++r) {
                RgMap qk = q;
                qk.live = lv[r];
                const float* yr = a.x + (lv[r] ? idx[r] : 0) * a.ld;
                y0[r] = lv[r] ? yr[0] : 1.0f;
                rg_load(yr + 1, d, qk, ys[r]);
            }
#pragma unroll
            for (int r = 0; r < EL_FLIGHT; ++r) {
                float pr[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) pr[j] = xs[j] * ys[r][j];
                const float S = rg_canon_sum(q, d, pr);
                const float t0 = x0 * y0[r];
                const float u = (idx[r] == s.iu) ? 1.0f : t0 - S;
                if (q.sub == kk + r) { myu = u; mylive = lv[r]; }
            }
        }
        const int k = gid + S * (c0 + q.sub);
        const float dk = mylive ? hm::dist_from_u(myu, a.sqrt_c) : INFINITY;
        if (q.live && k < P) wr[k] = mylive ? myu : 1.0f;
        if (c0 == 0) d0 = __shfl(dk, 0, width);                  // partner 0: position 0 of group 0
        dmin = fminf(dmin, rg_wave_min(width, dk));
    }

    // pass 2: the shifted sum, every lane over the slots it stored
    float sum = 0.0f;
    for (int c0 = 0; c0 < Pp; c0 += G) {
        const int k = gid + S * (c0 + q.sub);
        if (s.ok && k < P && rg_in(s.ix[1 + k], a.V)) sum = sum + expf(dmin - hm::dist_from_u(wr[k], a.sqrt_c));
    }
    sum = rg_wave_sum(width, sum);
    const float lse = logf(sum) - dmin;
    if (q.live && q.sub == 0 && gid == 0) a.loss[q.row] = s.ok ? d0 + lse : 0.0f;

    // pass 3: u_k -> a_k in place
    for (int c0 = 0; c0 < Pp; c0 += G) {
        const int k = gid + S * (c0 + q.sub);
        if (!q.live || k >= P) continue;
        float ak = 0.0f;
        if (s.ok && rg_in(s.ix[1 + k], a.V)) {
            const float u = wr[k];
            if (u > 1.0f) {
                const float p = expf(dmin - hm::dist_from_u(u, a.sqrt_c)) / sum;
                ak = ((k == 0 ? 1.0f : 0.0f) - p) / (a.sqrt_c * __builtin_sqrtf(u * u - 1.0f));
            }
        }
        wr[k] = ak;
    }
}

__global__ __launch_bounds__(EL_THREADS) void hm_el_bwd_kernel(const ElArgs a)
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
    const float g = q.live ? a.gl[q.row] : 0.0f;
    const float* wr = a.w + q.row * (int64_t)P;
    const int64_t slot0 = q.row * (int64_t)(2 + a.K);
    const int64_t fill = s.ok ? s.iu : 0;                     // COO index of a skipped slot: its value row is zero
    for (int i0 = 0; i0 < Pp; i0 += EL_FLIGHT) {
        int64_t idx[EL_FLIGHT];
        bool lv[EL_FLIGHT];
        float ak[EL_FLIGHT];
        RgRow y[EL_FLIGHT];
#pragma unroll
        for (int r = 0; r < EL_FLIGHT; ++r) {
            const int k = gid + S * (i0 + r);
            idx[r] = (s.ok && k < P) ? s.ix[1 + k] : -1;
            ak[r] = rg_in(idx[r], a.V) ? wr[k] : 0.0f;
        }
        rg_gather<EL_FLIGHT>(a.x, a.ld, a.V, d, q, idx, 0.0f, lv, y);
#pragma unroll
        for (int r = 0; r < EL_FLIGHT; ++r) {
            const int k = gid + S * (i0 + r);
            if (k >= P) continue;
            acc.t = acc.t + ak[r] * y[r].t;
            RgRow v;
            const float ga = g * ak[r];
            v.t = lv[r] ? ga * x.t : 0.0f;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                acc.s[j] = acc.s[j] - ak[r] * y[r].s[j];
                v.s[j] = lv[r] ? -(ga * x.s[j]) : 0.0f;
            }
            rg_lrow_store(a.val + (slot0 + 1 + k) * d1, d, q, v);
            if (q.live && q.sub == 0) a.coo[slot0 + 1 + k] = lv[r] ? idx[r] : fill;
        }
    }
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
static int g_el_form = 1;

static int el_args(const char* who, const float* x_dev, int64_t ld, int64_t V, int d1, const int64_t* index_dev, int64_t B, int64_t K,
                   float c, ElArgs& a)
{
    if (rg_bad_table(d1, ld, V) || B < 0 || B >= ((int64_t)1 << 31) || K < 0 || K > ((int64_t)1 << 20) ||
        (B + 1) * (K + 2) > ((int64_t)1 << 40) || !(c > 0.0f) || !(c < INFINITY))
        return hm_fail(nullptr, HM_E_ARG, std::string(who) + ": bad arguments");
    if (!x_dev || !index_dev) return hm_fail(nullptr, HM_E_ARG, std::string(who) + ": NULL pointer");
    a = ElArgs{};
    a.x = x_dev; a.index = index_dev;
    a.ld = ld; a.B = B; a.V = V;
    a.K = (int)K; a.d = d1 - 1; a.lsh = rg_lsh(a.d); a.split = g_el_form;
    a.sqrt_c = sqrtf(c);
    return HM_OK;
}

// Test / tuning hook: 0 = one lane group per sample, 1 = one wave per sample (the default), for the calls that follow.  The
// two forms differ in the order of the sums over the partners, not in any u_k or d_k.
extern "C" int hm_debug_edge_loss_form(int form)
{
    if (form != 0 && form != 1) return hm_fail(nullptr, HM_E_ARG, "hm_debug_edge_loss_form: form must be 0 or 1");
    g_el_form = form;
    return HM_OK;
}

extern "C" int hm_edge_loss_fwd(const float* x_dev, int64_t ld, int64_t table_rows, int d1, const int64_t* index_dev, int64_t n, int64_t k,
                                float c, float* loss_dev, float* weights_dev, void* stream)
{
    ElArgs a;
    if (int rc = el_args("hm_edge_loss_fwd", x_dev, ld, table_rows, d1, index_dev, n, k, c, a)) return rc;
    if (!loss_dev || !weights_dev) return hm_fail(nullptr, HM_E_ARG, "hm_edge_loss_fwd: NULL pointer");
    if (n == 0) return HM_OK;
    a.loss = loss_dev; a.w = weights_dev;
    hipLaunchKernelGGL(hm_el_fwd_kernel, rg_split_grid(a.B, a.lsh, a.split, EL_THREADS), dim3(EL_THREADS), 0, (hipStream_t)stream, a);
    HM_HIP0(hipGetLastError());
    return HM_OK;
}

extern "C" int hm_edge_loss_bwd(const float* x_dev, int64_t ld, int64_t table_rows, int d1, const int64_t* index_dev, int64_t n, int64_t k,
                                float c, const float* weights_dev, const float* grad_loss_dev, float* values_dev, int64_t* coo_dev,
                                void* stream)
{
    ElArgs a;
    if (int rc = el_args("hm_edge_loss_bwd", x_dev, ld, table_rows, d1, index_dev, n, k, c, a)) return rc;
    if (!weights_dev || !grad_loss_dev || !values_dev || !coo_dev) return hm_fail(nullptr, HM_E_ARG, "hm_edge_loss_bwd: NULL pointer");
    if (n == 0) return HM_OK;
    a.w = const_cast<float*>(weights_dev); a.gl = grad_loss_dev; a.val = values_dev; a.coo = coo_dev;
    hipLaunchKernelGGL(hm_el_bwd_kernel, rg_split_grid(a.B, a.lsh, a.split, EL_THREADS), dim3(EL_THREADS), 0, (hipStream_t)stream, a);
    HM_HIP0(hipGetLastError());
    return HM_OK;
}
