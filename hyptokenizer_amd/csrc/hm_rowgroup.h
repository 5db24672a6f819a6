// hm_rowgroup.h -- "a group of lanes owns a row": the layout of the row-wise kernels that keep a whole row in registers
// (hm_poincare.hip, hm_riemann.hip).
//
// A row of width d <= HM_RG_MAX_D is owned by a group of 16 (d <= 64) or 32 lanes of one wave; a wave therefore carries 4
// or 2 rows and a load instruction of the wave always covers whole rows.  A lane holds four slots of its row:
//   vector form (d % 4 == 0, every leading dimension % 4 == 0, every base 16-byte aligned): slots 4 sub .. 4 sub + 3, one
//     16-byte load / store per operand;
//   scalar form (everything else, and every row whose slots start one column in): slots sub + lanes * j, coalesced 4-byte
//     accesses.
// Sums are butterflies over the group (__shfl_xor), so every lane ends with the row scalars; the rows past the last one
// ("dead" rows) keep zeros and take part in the butterflies only.  Loads and stores take the ROW pointer -- the caller forms
// p + row * ld (+ 1 for the spatial part of a Lorentz row) -- and dereference it only when the row is live.
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

// host side
static inline int rg_lsh(int d) { return d <= 64 ? 4 : 5; }      // log2 of the lanes per row: 4 slots each cover d <= 128
static inline bool rg_al(const void* p, int64_t ld) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0 && (ld & 3) == 0; }
static inline dim3 rg_grid(int64_t rows, int lsh) { return dim3((unsigned)(((rows << lsh) + HM_RG_THREADS - 1) / HM_RG_THREADS)); }
