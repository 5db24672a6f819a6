// hm_recon.hip -- graph reconstruction (mean rank, mean average precision) of a Lorentz table as one walk over the pair tiles,
// without a [nodes, V] distance slab.
//
// A slot is a directed edge e = (u, o), o in N(u).  With D[u, v] the canonical fp32 distance at c = 1 (the bits of
// hm_batch_distance) the call writes per slot
//   less_all[e]  = #{ v != u    : D[u, v] <  D[u, o] }      equal_all[e] = #{ v != u    : D[u, v] == D[u, o] }
//   less_nb[e]   = #{ v in N(u) : D[u, v] <  D[u, o] }      equal_nb[e]  = #{ v in N(u) : D[u, v] == D[u, o] }
// NaN orders as in hm_retrieval.hip: greater than every number, equal to NaN.
//
// All-keys walk: the pair-tile walk of hm_retrieval.hip whose pivot is an arbitrary row per slot.  A block of 256 threads
// owns 64 slots, thread (r = lane, q = wave) holds the anchor row of slot r and evaluates the canonical u against rows
// 16 q .. 16 q + 15 of every 64-row tile of the table, ascending.  The pivot rows of the block are staged once as a gathered
// tile and u(u, o) goes through the same code as every other pair, so it has the bits the walk meets at v = o.  The decision
// rules are those of hm_retrieval_rank_kernel (proof in the header of hm_retrieval.hip): equal clamped u => equal distance;
// outside [u (1 - 2^-10), u (1 + 2^-10)] the order of u is the order of the distances; inside, the distances are compared.
// The clamped pivot u of every slot is parked in an fp32 vector.
//
// Neighbour counts: they need no table row.  The u of the slots of one anchor were all produced by the walk's code path with
// the same anchor row, so thread e compares u_pivot[e] with u_pivot[e'] of every e' of its segment by the same three-way
// rule.  One thread per slot: a hub's segment is spread over degree / 256 blocks, not given to one wave.
//
// Every output element is written once by one thread; the four waves' partial counts are added in a fixed order; no atomics.
#include "hm_retrieval_device.h"

#pragma clang fp contract(off)

#define HM_RC_MAX_ROWS (((int64_t)1 << 31) - 1)
#define HM_RC_NB_THREADS 256

namespace {

// the pivot of a slot: its clamped u, its distance and the band outside which u decides
struct hm_rc_pivot {
    float u, d, lo, hi;
};

__device__ __forceinline__ hm_rc_pivot hm_rc_make_pivot(float uc)
{
    return {uc, hm::dist_from_u(uc, 1.0f), uc * HM_RT_BAND_LO, uc * HM_RT_BAND_HI};
}

// one pair with clamped u `uc` against the pivot: 1 = less, 2 = equal, 0 = greater
__device__ __forceinline__ int hm_rc_cmp(const hm_rc_pivot p, float uc)
{
    const bool pnan = p.u != p.u;
    if (uc != uc) return pnan ? 2 : 0;                         // NaN is never less; it equals a NaN pivot
    if (pnan) return 1;                                        // every number is less than NaN
    if (uc == p.u) return 2;
    if (uc < p.lo) return 1;
    if (uc > p.hi) return 0;
    const float dj = hm::dist_from_u(uc, 1.0f);
    return dj < p.d ? 1 : (dj == p.d ? 2 : 0);
}

// anchor and pivot row of slot e0 + r into sa[r], sp[r]; -1 for both past the end or where either lies outside [0, V)
__device__ __forceinline__ void hm_rc_load_slots(const int32_t* __restrict__ anchor, const int32_t* __restrict__ pivot, int64_t n_slots,
                                                 int64_t V, int64_t e0, int* sa, int* sp)
{
    if (threadIdx.x < HM_PT) {
        const int64_t e = e0 + threadIdx.x;
        int a = -1, p = -1;
        if (e < n_slots) {
            a = anchor[e];
            p = pivot[e];
            if (a < 0 || (int64_t)a >= V || p < 0 || (int64_t)p >= V) a = p = -1;
        }
        sa[threadIdx.x] = a;
        sp[threadIdx.x] = p;
    }
}

// the four waves' partial counts in a fixed order; a slot with an index outside the table gets -1
__device__ __forceinline__ void hm_rc_finish(int (*part_lt)[HM_PT], int (*part_eq)[HM_PT], int r, int q, int lt, int eq, int64_t e,
                                             int64_t n_slots, bool live, float upiv, int32_t* __restrict__ less_all,
                                             int32_t* __restrict__ equal_all, float* __restrict__ u_out)
{
    part_lt[q][r] = lt;
    part_eq[q][r] = eq;
    __syncthreads();
    if (q == 0 && e < n_slots) {
        int sl = 0, se = 0;
        for (int w = 0; w < 4; ++w) sl += part_lt[w][r];
        for (int w = 0; w < 4; ++w) se += part_eq[w][r];
        less_all[e] = live ? sl : -1;
        equal_all[e] = live ? se : -1;
        u_out[e] = live ? upiv : __builtin_nanf("");
    }
}

// ---- anchor and partner rows in LDS (the layout of hm_grad_device.h): every width, the only one for d1 < 9 ----
__global__ __launch_bounds__(HM_PT_THREADS) void hm_recon_walk_kernel(const float* __restrict__ X, int64_t V, int64_t ld, int d1,
                                                                       const int32_t* __restrict__ anchor, const int32_t* __restrict__ pivot,
                                                                       int64_t n_slots, int32_t* __restrict__ less_all,
                                                                       int32_t* __restrict__ equal_all, float* __restrict__ u_out)
{
    extern __shared__ float hm_pt_lds[];
    __shared__ int part_lt[4][HM_PT], part_eq[4][HM_PT];
    __shared__ int sa[HM_PT], sp[HM_PT];
    const int SA = hm_pt_stride(d1);
    float* As = hm_pt_lds;
    float* Bs = As + HM_PT * SA;
    const int r = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int64_t e0 = (int64_t)blockIdx.x * HM_PT, e = e0 + r;
    hm_rc_load_slots(anchor, pivot, n_slots, V, e0, sa, sp);
    __syncthreads();
    for (int idx = threadIdx.x; idx < HM_PT * d1; idx += HM_PT_THREADS) {      // the gathered anchor and pivot tiles
        const int rr = idx / d1, k = idx - rr * d1;
        const int a = sa[rr], p = sp[rr];
        As[rr * SA + k] = a >= 0 ? X[(int64_t)a * ld + k] : 0.0f;
        Bs[rr * SA + k] = p >= 0 ? X[(int64_t)p * ld + k] : 0.0f;
    }
    __syncthreads();
    const int64_t me = sa[r];
    const bool live = me >= 0;
    const hm_rc_pivot piv = hm_rc_make_pivot(hm::clamp_min_one(hm_g_u(As + r * SA, Bs + r * SA, d1, 1)));
    __syncthreads();
    int lt = 0, eq = 0;
    for (int64_t j0 = 0; j0 < V; j0 += HM_PT) {
        hm_pt_stage(X, V, ld, d1, j0, Bs);
        __syncthreads();
        for (int jj = 0; jj < HM_PT_JPT; ++jj) {
            const int jl = q * HM_PT_JPT + jj;
            const int64_t j = j0 + jl;
            if (j >= V) break;                                                 // wave-uniform
            if (!live || j == me) continue;
            const int c = hm_rc_cmp(piv, hm::clamp_min_one(hm_g_u(As + r * SA, Bs + jl * SA, d1, 1)));
            lt += c & 1;
            eq += c >> 1;
        }
        __syncthreads();
    }
    hm_rc_finish(part_lt, part_eq, r, q, lt, eq, e, n_slots, live, piv.u, less_all, equal_all, u_out);
}

// ---- the anchor row in registers, partner rows read as 16-byte LDS broadcasts (hm_retrieval_device.h); d1 >= 9 ----
template <int MAXN>
__global__ __launch_bounds__(HM_PT_THREADS) void hm_recon_walk_reg_kernel(const float* __restrict__ X, int64_t V, int64_t ld, int d1,
                                                                           const int32_t* __restrict__ anchor,
                                                                           const int32_t* __restrict__ pivot, int64_t n_slots,
                                                                           int32_t* __restrict__ less_all, int32_t* __restrict__ equal_all,
                                                                           float* __restrict__ u_out)
{
    extern __shared__ float hm_pt_lds[];
    __shared__ int part_lt[4][HM_PT], part_eq[4][HM_PT];
    __shared__ int sa[HM_PT], sp[HM_PT];
    constexpr int SB = MAXN + 4;
    float* Bs = hm_pt_lds;
    const int r = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int64_t e0 = (int64_t)blockIdx.x * HM_PT, e = e0 + r;
    const int ns = d1 - 1;
    hm_rc_load_slots(anchor, pivot, n_slots, V, e0, sa, sp);
    __syncthreads();
    const int64_t me = sa[r];
    const bool live = me >= 0;
    float a[MAXN];
    const float* arow = X + (live ? me : 0) * ld;
#pragma unroll
    for (int s = 0; s < MAXN; ++s) a[s] = (s < ns && live) ? arow[1 + s] : 0.0f;
    const float a0 = live ? arow[0] : 0.0f;
    for (int idx = threadIdx.x; idx < HM_PT * d1; idx += HM_PT_THREADS) {      // the gathered pivot tile
        const int rr = idx / d1, k = idx - rr * d1;
        const int p = sp[rr];
        Bs[rr * SB + (k == 0 ? MAXN : k - 1)] = p >= 0 ? X[(int64_t)p * ld + k] : 0.0f;
    }
    __syncthreads();
    const hm_rc_pivot piv = hm_rc_make_pivot(hm::clamp_min_one(hm_rt_u_reg<MAXN>(a, a0, Bs + r * SB, ns, 1)));
    __syncthreads();
    int lt = 0, eq = 0;
    for (int64_t j0 = 0; j0 < V; j0 += HM_PT) {
        hm_rt_stage_reg<MAXN>(X, V, ld, d1, j0, Bs);
        __syncthreads();
#pragma unroll 1
        for (int jj = 0; jj < HM_PT_JPT; ++jj) {
            const int jl = q * HM_PT_JPT + jj;
            const int64_t j = j0 + jl;
            if (j >= V) break;                                                 // wave-uniform
            const float uc = hm::clamp_min_one(hm_rt_u_reg<MAXN>(a, a0, Bs + jl * SB, ns, 1));
            if (!live || j == me) continue;
            const int c = hm_rc_cmp(piv, uc);
            lt += c & 1;
            eq += c >> 1;
        }
        __syncthreads();
    }
    hm_rc_finish(part_lt, part_eq, r, q, lt, eq, e, n_slots, live, piv.u, less_all, equal_all, u_out);
}

// ---- neighbour counts: thread e against the parked u of its segment ----
__global__ __launch_bounds__(HM_RC_NB_THREADS) void hm_recon_nb_kernel(const float* __restrict__ u, const int32_t* __restrict__ slot_seg,
                                                                       const int64_t* __restrict__ seg_ptr, int64_t n_slots, int64_t n_seg,
                                                                       const int32_t* __restrict__ less_all, int32_t* __restrict__ less_nb,
                                                                       int32_t* __restrict__ equal_nb)
{
    const int64_t e = (int64_t)blockIdx.x * HM_RC_NB_THREADS + threadIdx.x;
    if (e >= n_slots) return;
    const int64_t g = slot_seg[e];
    int lt = -1, eq = -1;
    if (g >= 0 && g < n_seg && less_all[e] >= 0) {
        int64_t lo = seg_ptr[g], hi = seg_ptr[g + 1];
        if (lo < 0) lo = 0;
        if (hi > n_slots) hi = n_slots;
        const hm_rc_pivot piv = hm_rc_make_pivot(u[e]);
        lt = eq = 0;
        for (int64_t f = lo; f < hi; ++f) {
            const int c = hm_rc_cmp(piv, u[f]);
            lt += c & 1;
            eq += c >> 1;
        }
    }
    less_nb[e] = lt;
    equal_nb[e] = eq;
}

// ---- the slots of a CSR: thread e finds its segment in seg_ptr and reads its anchor and pivot ----
__global__ __launch_bounds__(HM_RC_NB_THREADS) void hm_recon_slots_kernel(const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                                          int64_t V, int64_t nnz, const int64_t* __restrict__ nodes,
                                                                          int64_t n_seg, const int64_t* __restrict__ seg_ptr, int64_t n_slots,
                                                                          int32_t* __restrict__ anchor, int32_t* __restrict__ pivot,
                                                                          int32_t* __restrict__ slot_seg)
{
    const int64_t e = (int64_t)blockIdx.x * HM_RC_NB_THREADS + threadIdx.x;
    if (e >= n_slots) return;
    int64_t lo = 0, hi = n_seg;                                // the last segment g with seg_ptr[g] <= e
    while (hi - lo > 1) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (seg_ptr[mid] <= e) lo = mid;
        else hi = mid;
    }
    const int64_t g = lo, node = nodes ? nodes[g] : g;
    int32_t a = -1, p = -1;
    if (node >= 0 && node < V) {
        const int64_t at = row_ptr[node] + (e - seg_ptr[g]);
        if (at >= row_ptr[node] && at < row_ptr[node + 1] && at < nnz) {
            a = (int32_t)node;
            p = col[at];
        }
    }
    anchor[e] = a;
    pivot[e] = p;
    slot_seg[e] = (int32_t)g;
}

inline unsigned hm_rc_blocks(int64_t n_slots) { return (unsigned)((n_slots + HM_PT - 1) / HM_PT); }

template <int MAXN>
int hm_rc_reg_launch(const float* X, int64_t V, int64_t ld, int d1, const int32_t* anchor, const int32_t* pivot, int64_t n_slots,
                     int32_t* less_all, int32_t* equal_all, float* u_out, hipStream_t s)
{
    const size_t lds = sizeof(float) * HM_PT * (MAXN + 4);
    hipLaunchKernelGGL(hm_recon_walk_reg_kernel<MAXN>, dim3(hm_rc_blocks(n_slots)), dim3(HM_PT_THREADS), lds, s, X, V, ld, d1, anchor, pivot,
                       n_slots, less_all, equal_all, u_out);
    return HM_OK;
}

}  // namespace

// The default layout: the anchor row in registers from this width on (rows that fill three quarters of the MAXN = 128 class),
// both rows in LDS below.  The register walk costs about the same for every width of a class, the LDS walk grows with the
// width: measured, the LDS walk wins at every width up to 66 but 65 (7 % behind) and loses by 24 - 30 % at 101 and 129
// (DESIGN.md 5.19).
#define HM_RC_REG_MIN_D1 97
static int g_rc_layout = 0;

extern "C" int hm_recon_slots(const int64_t* row_ptr_dev, const int32_t* col_dev, int64_t V, int64_t nnz, const int64_t* nodes_dev,
                              int64_t n_seg, const int64_t* seg_ptr_dev, int64_t n_slots, int32_t* slot_anchor_dev, int32_t* slot_pivot_dev,
                              int32_t* slot_seg_dev, void* stream)
{
    if (V < 1 || V > HM_RC_MAX_ROWS || nnz < 0 || nnz > HM_RC_MAX_ROWS || n_seg < 0 || n_seg > HM_RC_MAX_ROWS || n_slots < 0 ||
        n_slots > HM_RC_MAX_ROWS)
        return hm_fail(nullptr, HM_E_ARG, "hm_recon_slots: V must lie in [1, 2^31) and nnz, n_seg, n_slots in [0, 2^31)");
    if (n_slots > 0 && n_seg < 1) return hm_fail(nullptr, HM_E_ARG, "hm_recon_slots: slots without a segment");
    if (!row_ptr_dev || !seg_ptr_dev || (n_slots > 0 && (!col_dev || !slot_anchor_dev || !slot_pivot_dev || !slot_seg_dev)))
        return hm_fail(nullptr, HM_E_ARG, "hm_recon_slots: NULL pointer");
    if (n_slots == 0) return HM_OK;
    hipLaunchKernelGGL(hm_recon_slots_kernel, dim3((unsigned)((n_slots + HM_RC_NB_THREADS - 1) / HM_RC_NB_THREADS)), dim3(HM_RC_NB_THREADS), 0,
                       (hipStream_t)stream, row_ptr_dev, col_dev, V, nnz, nodes_dev, n_seg, seg_ptr_dev, n_slots, slot_anchor_dev,
                       slot_pivot_dev, slot_seg_dev);
    HM_HIP0(hipGetLastError());
    return HM_OK;
}

extern "C" int hm_recon_counts(const float* x_dev, int64_t ld, int64_t V, int d1, const int32_t* slot_anchor_dev,
                               const int32_t* slot_pivot_dev, const int32_t* slot_seg_dev, const int64_t* seg_ptr_dev, int64_t n_slots,
                               int64_t n_seg, int32_t* less_all_dev, int32_t* equal_all_dev, int32_t* less_nb_dev, int32_t* equal_nb_dev,
                               float* u_scratch_dev, void* stream)
{
    if (d1 < 2 || d1 > 129 || ld < d1) return hm_fail(nullptr, HM_E_ARG, "hm_recon_counts: d1 must lie in 2..129 and ld >= d1");
    if (V < 1 || V > HM_RC_MAX_ROWS) return hm_fail(nullptr, HM_E_ARG, "hm_recon_counts: V must lie in [1, 2^31)");
    if (n_slots < 0 || n_slots > HM_RC_MAX_ROWS || n_seg < 0 || n_seg > HM_RC_MAX_ROWS)
        return hm_fail(nullptr, HM_E_ARG, "hm_recon_counts: n_slots and n_seg must lie in [0, 2^31)");
    if (n_slots > 0 && n_seg < 1) return hm_fail(nullptr, HM_E_ARG, "hm_recon_counts: slots without a segment");
    if (!x_dev || !seg_ptr_dev ||
        (n_slots > 0 && (!slot_anchor_dev || !slot_pivot_dev || !slot_seg_dev || !less_all_dev || !equal_all_dev || !less_nb_dev ||
                         !equal_nb_dev || !u_scratch_dev)))
        return hm_fail(nullptr, HM_E_ARG, "hm_recon_counts: NULL pointer");
    if (n_slots == 0) return HM_OK;
    hipStream_t s = (hipStream_t)stream;
    const int layout = g_rc_layout ? g_rc_layout : (d1 >= HM_RC_REG_MIN_D1 ? 2 : 1);
    if (layout == 2 && d1 >= 9) {
        if (d1 <= 33) hm_rc_reg_launch<32>(x_dev, V, ld, d1, slot_anchor_dev, slot_pivot_dev, n_slots, less_all_dev, equal_all_dev, u_scratch_dev, s);
        else if (d1 <= 65) hm_rc_reg_launch<64>(x_dev, V, ld, d1, slot_anchor_dev, slot_pivot_dev, n_slots, less_all_dev, equal_all_dev, u_scratch_dev, s);
        else hm_rc_reg_launch<128>(x_dev, V, ld, d1, slot_anchor_dev, slot_pivot_dev, n_slots, less_all_dev, equal_all_dev, u_scratch_dev, s);
    } else {
        const size_t lds = sizeof(float) * hm_pt_lds_floats(d1, false);
        HM_HIP0(hm_pt_allow_lds(hm_recon_walk_kernel, lds));
        hipLaunchKernelGGL(hm_recon_walk_kernel, dim3(hm_rc_blocks(n_slots)), dim3(HM_PT_THREADS), lds, s, x_dev, V, ld, d1, slot_anchor_dev,
                           slot_pivot_dev, n_slots, less_all_dev, equal_all_dev, u_scratch_dev);
    }
    hipLaunchKernelGGL(hm_recon_nb_kernel, dim3((unsigned)((n_slots + HM_RC_NB_THREADS - 1) / HM_RC_NB_THREADS)), dim3(HM_RC_NB_THREADS), 0, s,
                       u_scratch_dev, slot_seg_dev, seg_ptr_dev, n_slots, n_seg, less_all_dev, less_nb_dev, equal_nb_dev);
    HM_HIP0(hipGetLastError());
    return HM_OK;
}

extern "C" int hm_debug_recon_layout(int layout)
{
    if (layout < 0 || layout > 2) return hm_fail(nullptr, HM_E_ARG, "hm_debug_recon_layout: layout must be 0, 1 or 2");
    g_rc_layout = layout;
    return HM_OK;
}
