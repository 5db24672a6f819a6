// hm_pool.hip -- Lorentz-centroid pooling of token rows (Law, Liao, Snell, Zemel, ICML 2019), forward and backward
// (DESIGN.md 5.18).  Engine-independent like hm_edgeloss.hip; the backward writes the same uncoalesced COO gradient, which
// the sparse path of hm_riemann.hip steps.
//
// table [V, ld] fp32 points of the unit hyperboloid x0^2 - |x_s|^2 = 1, ids int64 [T], offsets int64 [n + 1], lengths int32 [n]
// or NULL, weights fp32 [T] or NULL.  Segment i is ids[offsets[i] : offsets[i] + len_i], len_i = lengths[i] clamped to the span
// offsets[i + 1] - offsets[i] (the whole span without lengths); offsets are clamped into [0, T].  A token is live when it lies
// inside its segment's length and its id lies in [0, V); nothing else is dereferenced.
//   s_i  = sum_t w_t x_{ids[t]} over the live tokens, all d1 columns (w_t = 1 without weights)
//   q_i  = s_i0^2 - |s_is|^2,  nu_i = sqrt(q_i),  mu_i = s_i / nu_i
//   degenerate (no live token, or q_i not positive and finite): mu_i = (1, 0, .., 0), 1 / nu_i stored as 0, zero gradient
//   h_i  = (g_i + (g_i . mu_i) J mu_i) / nu_i, J = diag(-1, 1, .., 1), Euclidean dot
//   table gradient: position t of segment i -> COO index ids[t], value row w_t h_i;  dL/dw_t = h_i . x_{ids[t]}
//   a skipped position (slack, id outside [0, V), outside every span): index 0, zero value row, zero weight gradient
//
// Layout: Lorentz rows gathered on the lane groups of hm_rowgroup.h.  Two forms (hm_debug_centroid_form,
// rg_split_map):
//   form 0  one GROUP per segment: the group walks all tokens of its segment;
//   form 1  one WAVE per segment: its S groups take the tokens g, g + S, g + 2 S, ... and combine s by rg_fold_groups.
// A walk goes in flights of PL_FLIGHT token rows per group (rg_gather's): the ids and weights of a round are loaded before its
// rows.  Trip counts are made uniform over the wave (the longest walk of its groups); a group whose segment has ended runs
// the remaining rounds with every access predicated off.
//   forward   s_i stays in registers; writes mu_i and 1 / nu_i.
//   backward  forms h_i once per segment, then walks the span [offsets[i], offsets[i + 1]) -- segment 0 from position 0 and
//             segment n - 1 up to T, so that one launch covers [0, T) -- and writes every value row and every COO index
//             exactly once: no atomics, no workspace.  It re-gathers x_{ids[t]} only when the weight gradient is asked for.
#include "hm_rowgroup.h"

#pragma clang fp contract(off)

#define PL_THREADS HM_RG_WAVE                                 // one wave per block: 4 or 2 segments (form 0) or one (form 1)
#define PL_FLIGHT 4                                           // token rows in flight per group

struct PlArgs {
    const float* x;
    const int64_t* ids;
    const int64_t* off;
    const int32_t* len;                                       // or NULL
    const float* w;                                           // or NULL
    float* mu;                                                // [n, d1]: written by the forward, read by the backward
    float* inv;                                               // [n]: 1 / nu_i, 0 for a degenerate segment
    const float* g;                                           // backward: upstream gradient [n, d1]
    float* val;                                               // backward: [T, d1]
    int64_t* coo;                                             // backward: [T]
    float* gw;                                                // backward: [T] or NULL
    int64_t ld, n, V, T;
    int d, lsh, split;
};

// the positions of a segment: the live tokens are [b, e), the backward's walk covers [lo, hi); all inside [0, T]
struct PlSeg {
    int64_t b, e, lo, hi;
};

__device__ __forceinline__ PlSeg pl_seg(const PlArgs& a, const RgMap& q)
{
    PlSeg s = {0, 0, 0, 0};
    if (!q.live) return s;
    int64_t o0 = a.off[q.row], o1 = a.off[q.row + 1];
    o0 = o0 < 0 ? 0 : (o0 > a.T ? a.T : o0);
    o1 = o1 < o0 ? o0 : (o1 > a.T ? a.T : o1);
    int64_t L = o1 - o0;
    if (a.len) {
        const int64_t l = a.len[q.row];
        L = l < 0 ? 0 : (l < L ? l : L);
    }
    s.b = o0;
    s.e = o0 + L;
    s.lo = q.row == 0 ? 0 : o0;
    s.hi = q.row == a.n - 1 ? a.T : o1;
    return s;
}

// rounds of a walk over `count` positions by the group gid of S, the same on every lane of the wave
__device__ __forceinline__ int64_t pl_rounds(int64_t count, int gid, int S)
{
    int64_t c = count > gid ? (count - gid + S - 1) / S : 0;
    for (int off = 32; off > 0; off >>= 1) {
        const int64_t o = __shfl_xor(c, off, 64);
        c = o > c ? o : c;
    }
    return c;
}

// Butterfly sum over the group in double.  The scalars of a segment -- q_i, nu_i, g_i . mu_i, h_i, once per segment, and h_i . x
// per token of the weight gradient -- are differences of products many times their size (s_0^2 against |s_s|^2 for rows far
// from the origin), so they are formed in double from the fp32 sums and rounded once; the walk over the rows stays fp32.
__device__ __forceinline__ double pl_sum_d(const RgMap& m, double a)
{
    for (int off = (1 << m.lsh) >> 1; off > 0; off >>= 1) a = a + __shfl_xor(a, off, 64);
    return a;
}

__global__ __launch_bounds__(PL_THREADS) void hm_pl_fwd_kernel(const PlArgs a)
{
    int gid, S;
    const RgMap q = rg_split_map(a.lsh, a.split, a.n, gid, S);
    const PlSeg sg = pl_seg(a, q);
    const int d = a.d;
    const int64_t rounds = pl_rounds(sg.e - sg.b, gid, S);
    RgRow s = {0.0f, {0.0f, 0.0f, 0.0f, 0.0f}};
    for (int64_t i0 = 0; i0 < rounds; i0 += PL_FLIGHT) {
        int64_t idx[PL_FLIGHT];
        bool lv[PL_FLIGHT];
        float wt[PL_FLIGHT];
        RgRow y[PL_FLIGHT];
#pragma unroll
        for (int r = 0; r < PL_FLIGHT; ++r) {
            const int64_t p = sg.b + gid + S * (i0 + r);
            const bool in = p < sg.e;
            idx[r] = in ? a.ids[p] : -1;
            wt[r] = (in && a.w) ? a.w[p] : 1.0f;
        }
        rg_gather<PL_FLIGHT>(a.x, a.ld, a.V, d, q, idx, 0.0f, lv, y);
#pragma unroll
        for (int r = 0; r < PL_FLIGHT; ++r) {
            const float w = lv[r] ? wt[r] : 0.0f;             // a skipped token adds w x = 0 * 0
            s.t = fmaf(w, y[r].t, s.t);
#pragma unroll
            for (int j = 0; j < 4; ++j) s.s[j] = fmaf(w, y[r].s[j], s.s[j]);
        }
    }
    rg_fold_groups(a.lsh, S, s);                              // form 1: every group ends with the segment's sum
    double sq = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) sq = sq + (double)s.s[j] * (double)s.s[j];
    sq = pl_sum_d(q, sq);
    const double qq = (double)s.t * (double)s.t - sq;
    const bool ok = qq > 0.0 && qq < (double)INFINITY;        // false for NaN as well
    const double nu = __builtin_sqrt(ok ? qq : 1.0);
    RgRow m;
    m.t = ok ? (float)((double)s.t / nu) : 1.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) m.s[j] = ok ? (float)((double)s.s[j] / nu) : 0.0f;
    RgMap q0 = q;
    q0.live = q.live && gid == 0;
    if (q0.live && q.sub == 0) a.inv[q.row] = ok ? (float)(1.0 / nu) : 0.0f;
    rg_lrow_store(a.mu + q.row * (int64_t)(d + 1), d, q0, m);
}

template <bool GW>
__global__ __launch_bounds__(PL_THREADS) void hm_pl_bwd_kernel(const PlArgs a)
{
    int gid, S;
    const RgMap q = rg_split_map(a.lsh, a.split, a.n, gid, S);
    const PlSeg sg = pl_seg(a, q);
    const int d = a.d, d1 = a.d + 1;
    // The rows of this kernel are written out, not RgRow / rg_gather / rg_lrow_store: a position's time column and COO index
    // go under ONE exec mask (two `if`s on the same lane stay two divergent regions in the machine code, 1 - 2 % of the
    // kernel), and the table rows are gathered only for the weight gradient.
    // h_i, on every lane of every group of the segment
    const float* gr = a.g + q.row * (int64_t)d1;
    const float* mr = a.mu + q.row * (int64_t)d1;
    float gs[4], ms[4], hs[4];
    const float g0 = q.live ? gr[0] : 0.0f;
    const float m0 = q.live ? mr[0] : 1.0f;
    const float inv = q.live ? a.inv[q.row] : 0.0f;
    rg_load(gr + 1, d, q, gs);
    rg_load(mr + 1, d, q, ms);
    double dot = 0.0, hd[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) dot = dot + (double)gs[j] * (double)ms[j];
    dot = pl_sum_d(q, dot) + (double)g0 * (double)m0;
    const bool ok = inv > 0.0f;
    const double h0d = ok ? ((double)g0 - dot * (double)m0) * (double)inv : 0.0;
    const float h0 = (float)h0d;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        hd[j] = ok ? ((double)gs[j] + dot * (double)ms[j]) * (double)inv : 0.0;
        hs[j] = (float)hd[j];
    }

    const int64_t rounds = pl_rounds(sg.hi - sg.lo, gid, S);
    for (int64_t i0 = 0; i0 < rounds; i0 += PL_FLIGHT) {
        int64_t pos[PL_FLIGHT], idx[PL_FLIGHT];
        bool lv[PL_FLIGHT];
        float wt[PL_FLIGHT], y0[PL_FLIGHT], ys[PL_FLIGHT][4];
#pragma unroll
        for (int r = 0; r < PL_FLIGHT; ++r) {
            pos[r] = sg.lo + gid + S * (i0 + r);
            const bool in = pos[r] >= sg.b && pos[r] < sg.e;
            idx[r] = in ? a.ids[pos[r]] : -1;
            wt[r] = (in && a.w) ? a.w[pos[r]] : 1.0f;
        }
#pragma unroll
        for (int r = 0; r < PL_FLIGHT; ++r) {
            lv[r] = rg_in(idx[r], a.V);
            if (GW) {
                RgMap qk = q;
                qk.live = lv[r];
                const float* yr = a.x + (lv[r] ? idx[r] : 0) * a.ld;
                y0[r] = lv[r] ? yr[0] : 0.0f;
                rg_load(yr + 1, d, qk, ys[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < PL_FLIGHT; ++r) {
            RgMap qp = q;
            qp.live = pos[r] < sg.hi;                         // dead groups have lo = hi = 0
            float vs[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) vs[j] = lv[r] ? wt[r] * hs[j] : 0.0f;
            float* vr = a.val + (qp.live ? pos[r] : 0) * (int64_t)d1;
            if (qp.live && q.sub == 0) {
                vr[0] = lv[r] ? wt[r] * h0 : 0.0f;
                a.coo[pos[r]] = lv[r] ? idx[r] : 0;
            }
            rg_store(vr + 1, d, qp, vs);
            if (GW) {
                double hx = 0.0;
#pragma unroll
                for (int j = 0; j < 4; ++j) hx = hx + hd[j] * (double)ys[r][j];
                hx = pl_sum_d(q, hx) + h0d * (double)y0[r];
                if (qp.live && q.sub == 0) a.gw[pos[r]] = (lv[r] && ok) ? (float)hx : 0.0f;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
static int g_pl_form = -1;

// The form of a launch without a forced one, from what the host knows without a read-back: n and the mean span t / n.  A wave
// per segment won or tied every kernel row of tools/pooling_probe.py (n = 1 024 and 16 384, about 32 tokens a line, DESIGN.md
// 5.18) and is taken whenever the mean span gives every group of the wave a token; below that (under 4 or 2 tokens a line)
// one group per segment keeps the lanes busy -- that side of the switch has not been measured.
static int pl_auto_form(int64_t n, int64_t t, int lsh)
{
    const int64_t S = PL_THREADS >> lsh;
    return n > 0 && t / n >= S ? 1 : 0;
}

static int pl_args(const char* who, const float* x_dev, int64_t ld, int64_t V, int d1, const int64_t* ids_dev, int64_t t,
                   const int64_t* offsets_dev, const int32_t* lengths_dev, const float* weights_dev, int64_t n, PlArgs& a)
{
    if (!x_dev) return hm_fail(nullptr, HM_E_ARG, std::string(who) + ": NULL table");
    if (rg_bad_table(d1, ld, V) || n < 0 || n >= ((int64_t)1 << 31) || t < 0 || t > ((int64_t)1 << 40))
        return hm_fail(nullptr, HM_E_ARG, std::string(who) + ": bad arguments");
    if ((n > 0 && !offsets_dev) || (t > 0 && !ids_dev)) return hm_fail(nullptr, HM_E_ARG, std::string(who) + ": NULL pointer");
    a = PlArgs{};
    a.x = x_dev; a.ids = ids_dev; a.off = offsets_dev; a.len = lengths_dev; a.w = weights_dev;
    a.ld = ld; a.n = n; a.V = V; a.T = t;
    a.d = d1 - 1; a.lsh = rg_lsh(a.d);
    a.split = g_pl_form >= 0 ? g_pl_form : pl_auto_form(n, t, a.lsh);
    return HM_OK;
}

// Test / tuning hook: 0 = one lane group per segment, 1 = one wave per segment, -1 = chosen per call from n and the mean
// segment length (the default), for the calls that follow.  The two forms differ in the order of the sum over the tokens.
extern "C" int hm_debug_centroid_form(int form)
{
    if (form < -1 || form > 1) return hm_fail(nullptr, HM_E_ARG, "hm_debug_centroid_form: form must be -1, 0 or 1");
    g_pl_form = form;
    return HM_OK;
}

extern "C" int hm_centroid_fwd(const float* x_dev, int64_t ld, int64_t table_rows, int d1, const int64_t* ids_dev, int64_t t,
                               const int64_t* offsets_dev, const int32_t* lengths_dev, const float* weights_dev, int64_t n,
                               float* mu_dev, float* inv_nu_dev, void* stream)
{
    PlArgs a;
    if (int rc = pl_args("hm_centroid_fwd", x_dev, ld, table_rows, d1, ids_dev, t, offsets_dev, lengths_dev, weights_dev, n, a)) return rc;
    if (n == 0) return HM_OK;
    if (!mu_dev || !inv_nu_dev) return hm_fail(nullptr, HM_E_ARG, "hm_centroid_fwd: NULL pointer");
    a.mu = mu_dev; a.inv = inv_nu_dev;
    hipLaunchKernelGGL(hm_pl_fwd_kernel, rg_split_grid(n, a.lsh, a.split, PL_THREADS), dim3(PL_THREADS), 0, (hipStream_t)stream, a);
    HM_HIP0(hipGetLastError());
    return HM_OK;
}

extern "C" int hm_centroid_bwd(const float* x_dev, int64_t ld, int64_t table_rows, int d1, const int64_t* ids_dev, int64_t t,
                               const int64_t* offsets_dev, const int32_t* lengths_dev, const float* weights_dev, int64_t n,
                               const float* mu_dev, const float* inv_nu_dev, const float* grad_dev, float* values_dev, int64_t* coo_dev,
                               float* grad_weights_dev, void* stream)
{
    PlArgs a;
    if (int rc = pl_args("hm_centroid_bwd", x_dev, ld, table_rows, d1, ids_dev, t, offsets_dev, lengths_dev, weights_dev, n, a)) return rc;
    if (t == 0) return HM_OK;
    if (!values_dev || !coo_dev) return hm_fail(nullptr, HM_E_ARG, "hm_centroid_bwd: NULL pointer");
    if (n == 0) {                                             // no segment: every position is outside every span
        HM_HIP0(hipMemsetAsync(values_dev, 0, (size_t)t * (size_t)d1 * sizeof(float), (hipStream_t)stream));
        HM_HIP0(hipMemsetAsync(coo_dev, 0, (size_t)t * sizeof(int64_t), (hipStream_t)stream));
        if (grad_weights_dev) HM_HIP0(hipMemsetAsync(grad_weights_dev, 0, (size_t)t * sizeof(float), (hipStream_t)stream));
        return HM_OK;
    }
    if (!mu_dev || !inv_nu_dev || !grad_dev) return hm_fail(nullptr, HM_E_ARG, "hm_centroid_bwd: NULL pointer");
    a.mu = const_cast<float*>(mu_dev); a.inv = const_cast<float*>(inv_nu_dev); a.g = grad_dev;
    a.val = values_dev; a.coo = coo_dev; a.gw = grad_weights_dev;
    const dim3 grid = rg_split_grid(n, a.lsh, a.split, PL_THREADS);
    if (grad_weights_dev)
        hipLaunchKernelGGL(hm_pl_bwd_kernel<true>, grid, dim3(PL_THREADS), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(hm_pl_bwd_kernel<false>, grid, dim3(PL_THREADS), 0, (hipStream_t)stream, a);
    HM_HIP0(hipGetLastError());
    return HM_OK;
}
