// hm_edgeloss.hip -- the graph-embedding objective of Nickel & Kiela (2017, 2018) on a Lorentz table, forward and backward
// (DESIGN.md 5.17).  Engine-independent like hm_riemann.hip, whose sparse path consumes what the backward kernel writes.
//
// A loss on an index [B, 2 + K] (hm_index_loss.h: the layout, the skipped slots and samples, the two forms, the backward
// body).  With u the anchor and k = 0 .. K its partners:
//   u_k    = x_u0 x_k0 - sum_s x_us x_ks          canonical u of hm_grad_device.h ("lorentz" sign), ATen's summation order;
//                                                 a partner that IS the anchor (same index) has u_k = 1 by definition
//   d_k    = acosh(max(u_k, 1)) / sqrt(c)         hm::dist_from_u: the bits of hm_rows_distance
//   loss_b = d_0 + log sum_{k live} exp(-d_k)     shifted by max_k(-d_k) = -min_k d_k
//   a_k    = ([k = 0] - p_k) / (sqrt(c) sqrt(u_k^2 - 1)), p = softmax(-d) over the live slots; a_k = 0 where u_k <= 1
//   grad   anchor: sum_k a_k (x_k0, -x_ks);  partner k: a_k (x_u0, -x_us)            (Euclidean, -J x = (x0, -xs))
//
// In form 1 (hm_debug_edge_loss_form) the S groups of a wave combine d_min, the sum of exponentials and the anchor's gradient
// by butterflies across the wave -- S times the waves, P / S the walk.
//   forward   pass 1: u_k by the whole group (rg_canon_sum: hm_halfwave_sum's chains laid over the group's slots), parked in
//             lane k % G, which evaluates d_k once and stores u_k to the weights w [B, P];
//             pass 2: every lane re-reads the u_k IT stored, sums exp(-(d_k - d_min)), one butterfly;
//             pass 3: the same lanes turn their u_k into a_k in place.
//   backward  il_bwd on the record a_k alone.
#include "hm_index_loss.h"
#include "hm_grad_device.h"

#pragma clang fp contract(off)

struct ElArgs : IlArgs {                                      // w [B, P]: u_k inside the forward kernel, a_k once it has finished
    float sqrt_c;
};

__global__ __launch_bounds__(IL_THREADS) void hm_el_fwd_kernel(const ElArgs a)
{
    const IlWalk wk = il_walk(a);
    const RgMap& q = wk.q;
    const RgSample& s = wk.s;
    const int gid = wk.gid, S = wk.S, P = wk.P, Pp = wk.Pp;
    const int G = 1 << a.lsh, d = a.d, width = G * S;            // width: the lanes that share the sample
    // The rows of this kernel are written out, not RgRow / rg_gather: with the rows in structs the compiler emits the same
    // 4508 instructions in a schedule that measures 0.6 - 0.9 % slower.
    const float* xr = a.x + (s.ok ? s.iu : 0) * a.ld;
    float xs[4];
    const float x0 = s.ok ? xr[0] : 1.0f;
    rg_load(xr + 1, d, wk.qa, xs);
    float* wr = a.w + q.row * (int64_t)P;

    // pass 1: u_k, parked in lane k % G; d_min and d_0
    float dmin = INFINITY, d0 = 0.0f;
    for (int c0 = 0; c0 < Pp; c0 += G) {
        float myu = 1.0f;
        bool mylive = false;
        for (int kk = 0; kk < G && c0 + kk < Pp; kk += IL_FLIGHT) {
            int64_t idx[IL_FLIGHT];
            bool lv[IL_FLIGHT];
            float y0[IL_FLIGHT], ys[IL_FLIGHT][4];
#pragma unroll
            for (int r = 0; r < IL_FLIGHT; ++r) {
                idx[r] = il_index(wk, c0 + kk + r);
                lv[r] = rg_in(idx[r], a.V);
            }
#pragma unroll
            for (int r = 0; r < IL_FLIGHT; ++r) {
                RgMap qk = q;
                qk.live = lv[r];
                const float* yr = a.x + (lv[r] ? idx[r] : 0) * a.ld;
                y0[r] = lv[r] ? yr[0] : 1.0f;
                rg_load(yr + 1, d, qk, ys[r]);
            }
#pragma unroll
            for (int r = 0; r < IL_FLIGHT; ++r) {
                float pr[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) pr[j] = xs[j] * ys[r][j];
                const float S = rg_canon_sum(q, d, pr);
                const float t0 = x0 * y0[r];
                const float u = (idx[r] == s.iu) ? 1.0f : t0 - S;
                if (q.sub == kk + r) { myu = u; mylive = lv[r]; }
            }
        }
        const int k = il_partner(wk, c0 + q.sub);
        const float dk = mylive ? hm::dist_from_u(myu, a.sqrt_c) : INFINITY;
        if (q.live && k < P) wr[k] = mylive ? myu : 1.0f;
        if (c0 == 0) d0 = __shfl(dk, 0, width);                  // partner 0: position 0 of group 0
        dmin = fminf(dmin, rg_wave_min(width, dk));
    }

    // pass 2: the shifted sum, every lane over the slots it stored
    float sum = 0.0f;
    for (int c0 = 0; c0 < Pp; c0 += G) {
        const int k = il_partner(wk, c0 + q.sub);
        if (s.ok && k < P && rg_in(s.ix[1 + k], a.V)) sum = sum + expf(dmin - hm::dist_from_u(wr[k], a.sqrt_c));
    }
    sum = rg_wave_sum(width, sum);
    const float lse = logf(sum) - dmin;
    if (q.live && q.sub == 0 && gid == 0) a.loss[q.row] = s.ok ? d0 + lse : 0.0f;

    // pass 3: u_k -> a_k in place
    for (int c0 = 0; c0 < Pp; c0 += G) {
        const int k = il_partner(wk, c0 + q.sub);
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

struct ElSlot {                                               // the record of a slot is a_k: the x term alone
    static constexpr bool kCone = false;
    const float* w;
    __device__ __forceinline__ float4 read(int64_t at) const { return make_float4(w[at], 0.0f, 0.0f, 0.0f); }
};

__global__ __launch_bounds__(IL_THREADS) void hm_el_bwd_kernel(const ElArgs a) { il_bwd(a, ElSlot{a.w}); }

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
static int g_el_form = 1;

static int el_args(const char* who, const float* x_dev, int64_t ld, int64_t V, int d1, const int64_t* index_dev, int64_t B, int64_t K,
                   float c, ElArgs& a)
{
    a = ElArgs{};
    if (int rc = il_args(who, x_dev, ld, V, d1, index_dev, B, K, c > 0.0f && c < INFINITY, g_el_form, a)) return rc;
    a.sqrt_c = sqrtf(c);
    return HM_OK;
}

// Test / tuning hook: 0 = one lane group per sample, 1 = one wave per sample (the default), for the calls that follow.  The
// two forms differ in the order of the sums over the partners, not in any u_k or d_k.
extern "C" int hm_debug_edge_loss_form(int form) { return il_set_form("hm_debug_edge_loss_form", form, g_el_form); }

extern "C" int hm_edge_loss_fwd(const float* x_dev, int64_t ld, int64_t table_rows, int d1, const int64_t* index_dev, int64_t n, int64_t k,
                                float c, float* loss_dev, float* weights_dev, void* stream)
{
    ElArgs a;
    if (int rc = el_args("hm_edge_loss_fwd", x_dev, ld, table_rows, d1, index_dev, n, k, c, a)) return rc;
    if (!loss_dev || !weights_dev) return hm_fail(nullptr, HM_E_ARG, "hm_edge_loss_fwd: NULL pointer");
    a.loss = loss_dev; a.w = weights_dev;
    return il_launch(hm_el_fwd_kernel, a, stream);
}

extern "C" int hm_edge_loss_bwd(const float* x_dev, int64_t ld, int64_t table_rows, int d1, const int64_t* index_dev, int64_t n, int64_t k,
                                float c, const float* weights_dev, const float* grad_loss_dev, float* values_dev, int64_t* coo_dev,
                                void* stream)
{
    ElArgs a;
    if (int rc = el_args("hm_edge_loss_bwd", x_dev, ld, table_rows, d1, index_dev, n, k, c, a)) return rc;
    if (!weights_dev || !grad_loss_dev || !values_dev || !coo_dev) return hm_fail(nullptr, HM_E_ARG, "hm_edge_loss_bwd: NULL pointer");
    a.w = const_cast<float*>(weights_dev); a.gl = grad_loss_dev; a.val = values_dev; a.coo = coo_dev;
    return il_launch(hm_el_bwd_kernel, a, stream);
}
