// hm_retrieval_device.h -- what the rank walks of hm_retrieval.hip and hm_recon.hip share: the band in which a comparison of
// two distances has to be made on the distances themselves (proof: header of hm_retrieval.hip), and the register layout of the
// pair-tile walk (the anchor row in registers, the partner tile read as 16-byte LDS broadcasts).
#pragma once
#include "hm_grad_device.h"

#pragma clang fp contract(off)

#define HM_RT_BAND_LO 0.9990234375f          // 1 - 2^-10
#define HM_RT_BAND_HI 1.0009765625f          // 1 + 2^-10

// Thread (r, q) keeps row r of A in MAXN + 1 registers for the whole kernel; only the B tile lives in LDS, one row per
// MAXN + 4 floats: spatial column s at offset s (so that eight consecutive terms are two aligned float4), the time column at
// offset MAXN.  A whole wave reads the same B row: every ds_read_b128 is a broadcast.  One instantiation per column class
// (MAXN = 32, 64, 128).  hm_rt_u_reg is hm::torch_order_sum unrolled to the class's length with wave-uniform guards in place
// of the run-time loop bounds: every accumulator receives the same terms in the same order, so u has the same bits
// (tests/test_gpu_retrieval.py runs both layouts against the oracle).  n = d1 - 1 >= 8; narrower rows take the LDS layout.
template <int MAXN>
__device__ __forceinline__ float hm_rt_u_reg(const float (&a)[MAXN], float a0, const float* __restrict__ b, int n, int sign_mode)
{
    constexpr int NV = MAXN / 8;
    const int vec_size = n >> 3, main_end = (vec_size >> 2) << 2;
    float ps[4][8];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int l = 0; l < 8; ++l) ps[k][l] = 0.0f;
    float acc = 0.0f;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        if (v <= vec_size) {
            const float4 b0 = *reinterpret_cast<const float4*>(b + 8 * v);
            const float4 b1 = *reinterpret_cast<const float4*>(b + 8 * v + 4);
            const float bb[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
            if (v < main_end) {                                 // the 4-way interleaved part: vector v feeds accumulator v & 3
#pragma unroll
                for (int l = 0; l < 8; ++l) ps[v & 3][l] = ps[v & 3][l] + a[8 * v + l] * bb[l];
            } else if (v < vec_size) {                          // the remaining whole vectors feed accumulator 0
#pragma unroll
                for (int l = 0; l < 8; ++l) ps[0][l] = ps[0][l] + a[8 * v + l] * bb[l];
            } else {                                            // the scalar tail, added up from 0 before the vector sums
#pragma unroll
                for (int l = 0; l < 8; ++l)
                    if (8 * v + l < n) acc = acc + a[8 * v + l] * bb[l];
            }
        }
    }
#pragma unroll
    for (int k = 1; k < 4; ++k)
#pragma unroll
        for (int l = 0; l < 8; ++l) ps[0][l] = ps[0][l] + ps[k][l];
#pragma unroll
    for (int l = 0; l < 8; ++l) acc = acc + ps[0][l];
    const float t = a0 * b[MAXN];
    const float m = t - acc;
    return sign_mode ? m : -m;
}

// rows [r0, r0 + HM_PT) of M into the register layout's tile
template <int MAXN>
__device__ __forceinline__ void hm_rt_stage_reg(const float* __restrict__ M, int64_t n, int64_t ld, int d1, int64_t r0, float* tile)
{
    constexpr int SB = MAXN + 4;
    for (int idx = threadIdx.x; idx < HM_PT * d1; idx += HM_PT_THREADS) {
        const int r = idx / d1, k = idx - r * d1;
        tile[r * SB + (k == 0 ? MAXN : k - 1)] = r0 + r < n ? M[(r0 + r) * ld + k] : 0.0f;
    }
}
