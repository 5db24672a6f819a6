// hm_index_loss.h -- a loss on a Lorentz table and an index [B, 2 + K]: what hm_edgeloss.hip and hm_cones.hip share, on the
// lane groups and gathered walks of hm_rowgroup.h.
//
// index [B, 2 + K] int64: column 0 the anchor, column 1 the positive, columns 2.. the negatives.  Partner k = 0 is the
// positive, partner k >= 1 the negative of column 1 + k; P = 1 + K partners.  A negative outside [0, V) is a skipped slot, a
// sample whose anchor or positive lies outside [0, V) is skipped whole; neither is ever dereferenced.  The sampler
// (hm_negsample.hip) writes this layout, hm_riemann.hip's sparse path consumes the COO gradient the backward body writes.
//
// A group keeps the anchor row in registers and walks partners in flights of IL_FLIGHT rows (rg_gather).  Two forms
// (rg_split_map): form 0 gives a sample to a GROUP, which walks all P partners; form 1 to a WAVE whose S groups take the
// partners k = g, g + S, g + 2 S, ... and combine across the wave.  "Position" i of group g is partner k = g + S i.
// The forward kernel of a loss is its own and leaves one record per slot in the weights w [B, P]; the backward kernel is
// il_bwd over the loss's slot policy: it re-gathers the partner rows and forms scaled row sums only, the anchor's sum carried
// in registers across the partner loop and folded across the groups, every value row [B, 2 + K, d1] and every COO index
// written exactly once: no atomics, no LDS, no workspace but w.
#pragma once
#include "hm_rowgroup.h"

#pragma clang fp contract(off)

#define IL_THREADS HM_RG_WAVE                                 // one wave per block: 4 or 2 samples, so that small batches spread
#define IL_FLIGHT 4                                           // partner rows in flight per group

struct IlArgs {                                               // a loss derives its own block and adds its scalars
    const float* x;
    const int64_t* index;
    float* w;                                                 // [B, P] records of the loss's own shape: forward writes, backward reads
    float* loss;                                              // forward: [B]
    const float* gl;                                          // backward: upstream gradient of loss [B]
    float* val;                                               // backward: [B * (2 + K), d1]
    int64_t* coo;                                             // backward: [B * (2 + K)]
    int64_t ld, B, V;
    int K, d, lsh, split;
};

// the sample of this group (anchor, positive, K negatives): its anchor and whether it is served -- a sample whose anchor or
// positive lies outside [0, V) is not
struct RgSample {
    const int64_t* ix;
    int64_t iu;
    bool ok;
};

__device__ __forceinline__ RgSample rg_sample(const int64_t* __restrict__ index, int K, int64_t V, const RgMap& q)
{
    RgSample s;
    s.ix = index + q.row * (int64_t)(2 + K);
    s.iu = q.live ? s.ix[0] : -1;
    const int64_t iv = q.live ? s.ix[1] : -1;
    s.ok = q.live && rg_in(s.iu, V) && rg_in(iv, V);
    return s;
}

// What every kernel opens with: the group's lanes q, its number gid among the S that share the sample, the sample s, the P
// partners of which a group takes Pp positions, and qa = q with live = "the sample is served", for the load of the anchor row.
struct IlWalk {
    RgMap q, qa;
    RgSample s;
    int gid, S, P, Pp;
};

__device__ __forceinline__ IlWalk il_walk(const IlArgs& a)
{
    IlWalk w;
    w.q = rg_split_map(a.lsh, a.split, a.B, w.gid, w.S);
    w.s = rg_sample(a.index, a.K, a.V, w.q);
    w.P = 1 + a.K;
    w.Pp = (w.P + w.S - 1) / w.S;
    w.qa = w.q;
    w.qa.live = w.s.ok;
    return w;
}

__device__ __forceinline__ int il_partner(const IlWalk& w, int pos) { return w.gid + w.S * pos; }

// the table row of the partner at position pos of this group: -1, "no position", past P and in a sample that is not served
__device__ __forceinline__ int64_t il_index(const IlWalk& w, int pos)
{
    const int k = il_partner(w, pos);
    return (w.s.ok && k < w.P) ? w.s.ix[1 + k] : -1;
}

// The backward kernel of a loss whose slot k contributes, with its record (cx, ca, cz, cp) = slot.read(),
//   to the anchor's row    cx (y0, -y_s) + ca e0   and, role 0,  cz (0, x_s)        x the anchor's row, y the partner's
//   to the partner's row   cx (x0, -x_s) + cp e0   and, role 1,  cz (0, y_s)
// times the upstream gradient g of the sample.  Slot::kCone says at compile time whether ca, cp and cz exist (the cones) or
// the record is cx alone (the edge loss, whose instantiation holds no instruction for them); slot.role, at run time, whose
// own spatial part cz scales.
template <class Slot>
__device__ __forceinline__ void il_bwd(const IlArgs& a, const Slot slot)
{
    const IlWalk w = il_walk(a);
    const RgMap& q = w.q;
    const int d = a.d, d1 = a.d + 1;
    const RgRow x = rg_lrow_load(a.x + (w.s.ok ? w.s.iu : 0) * a.ld, d, w.qa, 0.0f);
    RgRow acc = {0.0f, {0.0f, 0.0f, 0.0f, 0.0f}};              // the anchor's sum over this group's partners
    float own = 0.0f;                                          // role 0: the sum of the factors of the anchor's own spatial part
    const float g = q.live ? a.gl[q.row] : 0.0f;
    const int64_t w0 = q.row * (int64_t)w.P, slot0 = q.row * (int64_t)(2 + a.K);
    // The COO index of a skipped slot, whose value row is zero: its anchor, row 0 in a sample that is not served.
    const int64_t fill = w.s.ok ? w.s.iu : 0;
    for (int i0 = 0; i0 < w.Pp; i0 += IL_FLIGHT) {
        int64_t idx[IL_FLIGHT];
        bool lv[IL_FLIGHT];
        float4 cf[IL_FLIGHT];
        RgRow y[IL_FLIGHT];
#pragma unroll
        for (int r = 0; r < IL_FLIGHT; ++r) {
            idx[r] = il_index(w, i0 + r);
            cf[r] = rg_in(idx[r], a.V) ? slot.read(w0 + il_partner(w, i0 + r)) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
        rg_gather<IL_FLIGHT>(a.x, a.ld, a.V, d, q, idx, 0.0f, lv, y);
#pragma unroll
        for (int r = 0; r < IL_FLIGHT; ++r) {
            const int k = il_partner(w, i0 + r);
            if (k >= w.P) continue;
            if constexpr (Slot::kCone) acc.t = acc.t + (cf[r].x * y[r].t + cf[r].y);
            else acc.t = acc.t + cf[r].x * y[r].t;
            const float ga = g * cf[r].x;
            float gz = 0.0f;                                   // role 1: the factor of the partner's own spatial part
            RgRow v;
            if constexpr (Slot::kCone) {
                gz = slot.role ? g * cf[r].z : 0.0f;
                if (!slot.role) own = own + cf[r].z;
                v.t = lv[r] ? ga * x.t + g * cf[r].w : 0.0f;
            } else {
                v.t = lv[r] ? ga * x.t : 0.0f;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                acc.s[j] = acc.s[j] - cf[r].x * y[r].s[j];
                if constexpr (Slot::kCone) v.s[j] = lv[r] ? gz * y[r].s[j] - ga * x.s[j] : 0.0f;
                else v.s[j] = lv[r] ? -(ga * x.s[j]) : 0.0f;
            }
            rg_lrow_store(a.val + (slot0 + 1 + k) * d1, d, q, v);
            if (q.live && q.sub == 0) a.coo[slot0 + 1 + k] = lv[r] ? idx[r] : fill;
        }
    }
    if constexpr (Slot::kCone) {
#pragma unroll
        for (int j = 0; j < 4; ++j) acc.s[j] = acc.s[j] + own * x.s[j];
    }
    rg_fold_groups(a.lsh, w.S, acc);                           // form 1: group 0 stores the anchor's row
    RgRow v;
    v.t = w.s.ok ? g * acc.t : 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) v.s[j] = w.s.ok ? g * acc.s[j] : 0.0f;
    RgMap q0 = q;
    q0.live = q.live && w.gid == 0;
    rg_lrow_store(a.val + slot0 * d1, d, q0, v);
    if (q0.live && q.sub == 0) a.coo[slot0] = fill;
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
// The bounds and the two pointers every entry point of a loss takes, and the common block of its arguments.  `own_ok` is
// the caller's verdict on its own scalars: they fail with the bounds, as "bad arguments", before any pointer is looked at.
static inline int il_args(const char* who, const float* x_dev, int64_t ld, int64_t V, int d1, const int64_t* index_dev, int64_t B, int64_t K,
                          bool own_ok, int form, IlArgs& a)
{
    if (rg_bad_table(d1, ld, V) || B < 0 || B >= ((int64_t)1 << 31) || K < 0 || K > ((int64_t)1 << 20) ||
        (B + 1) * (K + 2) > ((int64_t)1 << 40) || !own_ok)
        return hm_fail(nullptr, HM_E_ARG, std::string(who) + ": bad arguments");
    if (!x_dev || !index_dev) return hm_fail(nullptr, HM_E_ARG, std::string(who) + ": NULL pointer");
    a.x = x_dev; a.index = index_dev;
    a.ld = ld; a.B = B; a.V = V;
    a.K = (int)K; a.d = d1 - 1; a.lsh = rg_lsh(a.d); a.split = form;
    return HM_OK;
}

// one wave per block in either form; an empty batch launches nothing
template <class Args>
static inline int il_launch(void (*kernel)(const Args), const Args& a, void* stream)
{
    if (a.B == 0) return HM_OK;
    hipLaunchKernelGGL(kernel, rg_split_grid(a.B, a.lsh, a.split, IL_THREADS), dim3(IL_THREADS), 0, (hipStream_t)stream, a);
    HM_HIP0(hipGetLastError());
    return HM_OK;
}

// Test / tuning hook of a loss: 0 = one lane group per sample, 1 = one wave per sample, for the calls that follow
static inline int il_set_form(const char* who, int form, int& slot)
{
    if (form != 0 && form != 1) return hm_fail(nullptr, HM_E_ARG, std::string(who) + ": form must be 0 or 1");
    slot = form;
    return HM_OK;
}
