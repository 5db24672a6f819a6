// hm_rowgroup.h -- "a group of lanes owns a row": the layout of the row-wise kernels that keep a whole row in registers
// (hm_poincare.hip, hm_riemann.hip, hm_edgeloss.hip, hm_cones.hip, hm_pool.hip).
//
// A row of width d <= HM_RG_MAX_D is owned by a group of 16 (d <= 64) or 32 lanes of one wave; a wave therefore carries 4
// or 2 rows and a load instruction of the wave always covers whole rows.  A lane holds four slots of its row:
//   vector form (d % 4 == 0, every leading dimension % 4 == 0, every base 16-byte aligned): slots 4 sub .. 4 sub + 3, one
//     16-byte load / store per operand;
//   scalar form (everything else, and every row whose slots start one column in): slots sub + lanes * j, coalesced 4-byte
//     accesses.
// Sums are butterflies over the group (__shfl_xor), so every lane ends with the row scalars; the rows past the last one
// ("dead" rows) keep zeros and take part in the butterflies only.  Loads and stores take the ROW pointer -- the caller forms
// p + row * ld -- and dereference it only when the row is live.
//
// Lorentz rows and gathered walks (second section): a row of d + 1 columns is its time column, a per-row scalar every lane
// of the group carries, beside the four slots of its spatial part, always in the scalar form (RgRow).  A row index taken
// from memory is tested by rg_in, the one predicate: an index outside [0, V) makes the row dead, a dead row is never
// dereferenced, reads as (dead_t, 0, .., 0) and takes part in butterflies only.  rg_gather is the flight of such rows; two
// kernels (edge-loss forward, pooling backward) keep theirs written out for speed.  A kernel that walks gathered rows
// is launched in one of two forms (rg_split_map): a group per row, or a wave per row whose S groups share the walk and
// fold their partial sums across the wave (rg_fold_groups).
#pragma once
#include "hm_common.h"

#pragma clang fp contract(off)

#define HM_RG_MAX_D 128
#define HM_RG_THREADS 256

struct RgMap {
    int sub, lsh, vec;                                        // lane within the group, log2 of the group, vector form
    int64_t row;
    bool live;
};

__device__ __forceinline__ RgMap rg_map(int lsh, int vec, int64_t rows)
{
    RgMap m;
    const int64_t gl = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    m.lsh = lsh;
    m.vec = vec;
    m.sub = (int)(threadIdx.x & ((1u << lsh) - 1u));
    m.row = gl >> lsh;
    m.live = m.row < rows;
    return m;
}

// column of slot j
__device__ __forceinline__ int rg_idx(const RgMap& m, int j) { return m.vec ? 4 * m.sub + j : m.sub + (j << m.lsh); }

// columns 0 .. d - 1 of the row at r into the lane's slots; slots past d, and every slot of a dead row, are 0
__device__ __forceinline__ void rg_load(const float* __restrict__ r, int d, const RgMap& m, float (&v)[4])
{
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = 0.0f;
    if (!m.live) return;
    if (m.vec) {
        if (4 * m.sub < d) {
            const float4 t = *reinterpret_cast<const float4*>(r + 4 * m.sub);
            v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = rg_idx(m, j);
            if (k < d) v[j] = r[k];
        }
    }
}

__device__ __forceinline__ void rg_store(float* __restrict__ r, int d, const RgMap& m, const float (&v)[4])
{
    if (!m.live) return;
    if (m.vec) {
        if (4 * m.sub < d) *reinterpret_cast<float4*>(r + 4 * m.sub) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = rg_idx(m, j);
            if (k < d) r[k] = v[j];
        }
    }
}

__device__ __forceinline__ float rg_sum(const RgMap& m, float a)
{
    for (int off = (1 << m.lsh) >> 1; off > 0; off >>= 1) a = a + __shfl_xor(a, off, 64);
    return a;
}

__device__ __forceinline__ float rg_dot(const RgMap& m, const float (&a)[4], const float (&b)[4])
{
    return rg_sum(m, (a[0] * b[0] + a[1] * b[1]) + (a[2] * b[2] + a[3] * b[3]));
}

// ------------------------------------------------------------------------------------------------
// Lorentz rows and gathered walks
// ------------------------------------------------------------------------------------------------
#define HM_RG_WAVE 64                                         // the block of a kernel launched in either form of rg_split_map

struct RgRow { float t; float s[4]; };                        // time column beside the slots of the spatial part

__device__ __forceinline__ bool rg_in(int64_t i, int64_t V) { return i >= 0 && i < V; }

// the row of d + 1 columns at r: the time column first (read by every lane of a live group), then the slots
__device__ __forceinline__ RgRow rg_lrow_load(const float* __restrict__ r, int d, const RgMap& m, float dead_t)
{
    RgRow v;
    v.t = m.live ? r[0] : dead_t;
    rg_load(r + 1, d, m, v.s);
    return v;
}

// the time column by the group's first lane, the spatial part by rg_store
__device__ __forceinline__ void rg_lrow_store(float* __restrict__ r, int d, const RgMap& m, const RgRow& v)
{
    if (m.live && m.sub == 0) r[0] = v.t;
    rg_store(r + 1, d, m, v.s);
}

// lane -> (row, group of the row, lane of the group) of a one-wave block: split = 0 is rg_map (a group per row, gid = 0 of
// S = 1), split = 1 gives the wave to row blockIdx.x, whose S = 4 or 2 groups are numbered gid
__device__ __forceinline__ RgMap rg_split_map(int lsh, int split, int64_t rows, int& gid, int& S)
{
    if (!split) {
        gid = 0;
        S = 1;
        return rg_map(lsh, 0, rows);
    }
    RgMap m;
    m.lsh = lsh;
    m.vec = 0;
    m.sub = (int)(threadIdx.x & ((1u << lsh) - 1u));
    m.row = (int64_t)blockIdx.x;
    m.live = m.row < rows;
    gid = (int)(threadIdx.x >> lsh);
    S = HM_RG_WAVE >> lsh;
    return m;
}

// A flight of F gathered rows of the table x [V, ld]: idx[r] is a row index, -1 for "no position".  lv[r] tells whether it
// lies in [0, V); the row pointer is predicated to row 0 when it does not and is then not dereferenced -- the row reads as
// (dead_t, 0, .., 0).  All F rows are issued before the caller consumes the first.
template <int F>
__device__ __forceinline__ void rg_gather(const float* __restrict__ x, int64_t ld, int64_t V, int d, const RgMap& q,
                                          const int64_t (&idx)[F], float dead_t, bool (&lv)[F], RgRow (&y)[F])
{
#pragma unroll
    for (int r = 0; r < F; ++r) lv[r] = rg_in(idx[r], V);
#pragma unroll
    for (int r = 0; r < F; ++r) {
        RgMap qk = q;
        qk.live = lv[r];
        y[r] = rg_lrow_load(x + (lv[r] ? idx[r] : 0) * ld, d, qk, dead_t);
    }
}

// split form: the groups' partial sums of a row, lane by lane across the wave (S = 1: nothing to do)
__device__ __forceinline__ void rg_fold_groups(int lsh, int S, RgRow& v)
{
    for (int off = 1 << lsh; off < (S << lsh); off <<= 1) {
        v.t = v.t + __shfl_xor(v.t, off, 64);
#pragma unroll
        for (int j = 0; j < 4; ++j) v.s[j] = v.s[j] + __shfl_xor(v.s[j], off, 64);
    }
}

__device__ __forceinline__ float rg_pick(const float (&p)[4], int j) { return j == 0 ? p[0] : j == 1 ? p[1] : j == 2 ? p[2] : p[3]; }

// Sum of the row's d products pr (element e in slot e >> lsh of lane e & (G - 1); slots past d hold 0) in the order of
// hm::torch_order_sum, bit for bit, on every lane of the group.  ATen's 32 chains: chain t takes elements t, t + 32, ... below
// 32 ilp; a group of 32 lanes holds chain t in lane t (slots 0 .. ilp - 1), a group of 16 holds chains t and t + 16 in lane t
// (even and odd slots).  Then hm_halfwave_sum's combine: leftover vectors of 8 into chains 0..7, chains l, l + 8, l + 16,
// l + 24 added in that order, the scalar tail summed from zero, the eight sums in order.  Every branch is uniform.
__device__ __forceinline__ float rg_canon_sum(const RgMap& q, int d, const float (&pr)[4])
{
    const int G = 1 << q.lsh, t = q.sub;
    if (d < 8) {                                              // scalar form: element e is slot 0 of lane e (G = 16)
        float ps[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        const int full = (d >> 2) * 4;
#pragma unroll
        for (int e = 0; e < 7; ++e) {
            const float v = __shfl(pr[0], e, 16);
            if (e < full) ps[e & 3] = ps[e & 3] + v;
            else if (e < d) ps[0] = ps[0] + v;
        }
        ps[0] = ps[0] + ps[1];
        ps[0] = ps[0] + ps[2];
        ps[0] = ps[0] + ps[3];
        return ps[0];
    }
    const int vec = d >> 3, ilp = vec >> 2, nleft = vec - ilp * 4, ntail = d - vec * 8;
    float pa = 0.0f, pb = 0.0f;
    float c1, c2, c3;
    if (q.lsh == 5) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < ilp) pa = pa + pr[j];
    } else {
#pragma unroll
        for (int i = 0; i < 2; ++i)
            if (i < ilp) { pa = pa + pr[2 * i]; pb = pb + pr[2 * i + 1]; }
    }
#pragma unroll
    for (int v = 0; v < 3; ++v) {
        if (v < nleft) {
            const int e0 = 32 * ilp + 8 * v;                  // first element of the leftover vector: 8 elements of one slot
            const float got = __shfl(rg_pick(pr, e0 >> q.lsh), (e0 & (G - 1)) + (t & 7), G);
            if (t < 8) pa = pa + got;
        }
    }
    if (q.lsh == 5) {
        c1 = __shfl(pa, (t & 7) + 8, 32);
        c2 = __shfl(pa, (t & 7) + 16, 32);
        c3 = __shfl(pa, (t & 7) + 24, 32);
    } else {
        c1 = __shfl(pa, (t & 7) + 8, 16);
        c2 = __shfl(pb, (t & 7), 16);
        c3 = __shfl(pb, (t & 7) + 8, 16);
    }
    const float r = ((pa + c1) + c2) + c3;                    // meaningful on lanes t < 8
    float acc = 0.0f;
#pragma unroll
    for (int v = 0; v < 7; ++v) {
        if (v < ntail) {
            const int e = vec * 8 + v;
            acc = acc + __shfl(rg_pick(pr, e >> q.lsh), e & (G - 1), G);
        }
    }
#pragma unroll
    for (int l = 0; l < 8; ++l) acc = acc + __shfl(r, l, G);
    return acc;
}

// butterflies over the lanes that share a sample: `width` = the group (a group per row) or the wave (a wave per row)
__device__ __forceinline__ float rg_wave_min(int width, float a)
{
    for (int off = width >> 1; off > 0; off >>= 1) a = fminf(a, __shfl_xor(a, off, 64));
    return a;
}
__device__ __forceinline__ float rg_wave_sum(int width, float a)
{
    for (int off = width >> 1; off > 0; off >>= 1) a = a + __shfl_xor(a, off, 64);
    return a;
}

// host side
static inline int rg_lsh(int d) { return d <= 64 ? 4 : 5; }      // log2 of the lanes per row: 4 slots each cover d <= 128
static inline bool rg_al(const void* p, int64_t ld) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0 && (ld & 3) == 0; }
static inline dim3 rg_grid(int64_t rows, int lsh) { return dim3((unsigned)(((rows << lsh) + HM_RG_THREADS - 1) / HM_RG_THREADS)); }
static inline dim3 rg_split_grid(int64_t rows, int lsh, int split, int threads)
{
    return dim3((unsigned)(split ? rows : ((rows << lsh) + threads - 1) / threads));
}
// Lorentz rows of d1 columns at leading dimension ld that a lane group cannot hold; a gathered table [V, ld] of them that
// the walks cannot address
static inline bool rg_bad_lrow(int d1, int64_t ld) { return d1 < 2 || d1 > HM_RG_MAX_D + 1 || ld < d1; }
static inline bool rg_bad_table(int d1, int64_t ld, int64_t V) { return rg_bad_lrow(d1, ld) || V < 0 || V > ((int64_t)1 << 40); }
