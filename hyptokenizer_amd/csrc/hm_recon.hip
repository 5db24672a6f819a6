// hm_recon.hip -- graph reconstruction (mean rank, mean average precision) of a Lorentz table as one walk over the pair tiles,
// without a [nodes, V] distance slab.
//
// A slot is a directed edge e = (u, o), o in N(u).  With D[u, v] the canonical fp32 distance at c = 1 (the bits of
// hm_batch_distance) the call writes per slot
//   less_all[e]  = #{ v != u    : D[u, v] <  D[u, o] }      equal_all[e] = #{ v != u    : D[u, v] == D[u, o] }
//   less_nb[e]   = #{ v in N(u) : D[u, v] <  D[u, o] }      equal_nb[e]  = #{ v in N(u) : D[u, v] == D[u, o] }
// NaN orders as in hm_retrieval.hip: greater than every number, equal to NaN.
//
// All-keys walk: the rank walk of hm_retrieval_device.h whose pivot is an arbitrary row per slot.  A block of 256 threads
// owns 64 slots, thread (r = lane, q = wave) holds the anchor row of slot r and evaluates the canonical u against rows
// 16 q .. 16 q + 15 of every 64-row tile of the table, ascending.  The pivot rows of the block are staged once as a gathered
// tile and u(u, o) goes through the same code as every other pair, so it has the bits the walk meets at v = o.  The decision
// rules are those of hm_rk_cmp (proof in the header of hm_retrieval.hip): equal clamped u => equal distance;
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

// MAXN = 0: anchor and partner rows in LDS (every width, the only layout for d1 < 9); 32 / 64 / 128: the anchor row in
// registers, d1 >= 9 (hm_rk_layout).  The anchor's own row is skipped, every equal counts, a dead slot gets -1 / NaN.
template <int MAXN>
__global__ __launch_bounds__(HM_PT_THREADS) void hm_recon_walk_kernel(const float* __restrict__ X, int64_t V, int64_t ld, int d1,
                                                                       const int32_t* __restrict__ anchor, const int32_t* __restrict__ pivot,
                                                                       int64_t n_slots, int32_t* __restrict__ less_all,
                                                                       int32_t* __restrict__ equal_all, float* __restrict__ u_out)
{
    extern __shared__ float hm_pt_lds[];
    __shared__ int sa[HM_PT], sp[HM_PT];
    const int r = threadIdx.x & 63;
    const int64_t e0 = (int64_t)blockIdx.x * HM_PT, e = e0 + r;
    hm_rc_load_slots(anchor, pivot, n_slots, V, e0, sa, sp);
    __syncthreads();
    const int64_t me = sa[r];
    const bool live = me >= 0;
    hm_rk_layout<MAXN> lay(hm_pt_lds, d1, 1);
    lay.load_owner(X, V, ld, [&](int rr) -> int64_t { return sa[rr]; });
    lay.stage(X, V, ld, [&](int rr) -> int64_t { return sp[rr]; });              // the gathered pivot tile
    __syncthreads();
    const hm_rk_pivot_t piv = hm_rk_pivot(hm::clamp_min_one(lay.u(r, r)));
    __syncthreads();
    int lt = 0, eq = 0;
    hm_rk_walk(lay, X, V, ld, [&](int64_t j, float uc) {
        if (!live || j == me) return;
        const int c = hm_rk_cmp(piv, uc);
        lt += c & 1;
        eq += c >> 1;
    });
    hm_rk_reduce(lt, eq);
    if (threadIdx.x < HM_PT && e < n_slots) {
        less_all[e] = live ? lt : -1;
        equal_all[e] = live ? eq : -1;
        u_out[e] = live ? piv.u : __builtin_nanf("");
    }
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
        const hm_rk_pivot_t piv = hm_rk_pivot(u[e]);
        lt = eq = 0;
        for (int64_t f = lo; f < hi; ++f) {
            const int c = hm_rk_cmp(piv, u[f]);
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
    if (int rc = hm_rk_launch([](auto maxn) { return hm_recon_walk_kernel<decltype(maxn)::value>; },
                              g_rc_layout ? g_rc_layout : (d1 >= HM_RC_REG_MIN_D1 ? 2 : 1), n_slots, d1, s, x_dev, V, ld, d1, slot_anchor_dev,
                              slot_pivot_dev, n_slots, less_all_dev, equal_all_dev, u_scratch_dev))
        return rc;
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
