// hm_gromov.hip -- Gromov delta-hyperbolicity of a distance matrix per base point, as one fused walk over the (max, min)
// semiring without a Gromov-product matrix.
//
// D(i, j) := d[min(i, j), max(i, j)] (only the upper triangle is read).  For a base point w
//   int16:  B(i, j) = D(i, w) + D(j, w) - D(i, j)                          (twice the Gromov product, an integer)
//           value   = max_{i <= j} [ max_k min(B(i, k), B(k, j)) - B(i, j) ]                       (int32, 2 delta_w)
//   fp32:   A(i, j) = 0.5f * ((D(i, w) + D(j, w)) - D(i, j)) + 0.0f        (this order, no contraction; -0 stored as +0)
//           value   = max_{i <= j} fl( max_k min(A(i, k), A(k, j)) - A(i, j) )                      (float, delta_w)
// Both products are symmetric bit for bit (the one sum of two operands commutes), so the operand B(k, j) of the inner
// product is staged as B(j, k): both operands of a tile are "row tile x k chunk" pieces of the same form.
//
// Order domain: every product is an int32 whose order is the order of the number -- the integer itself, or for a finite
// float the key bits(x) for x >= 0 and bits(x) ^ 0x7fffffff below (its own inverse).  max and min of keys are v_max_i32 /
// v_min_i32: fmaxf / fminf in the inner loop make the compiler canonicalise its operands (three v_max_f32 for one min).
// The winner is mapped back before the one subtraction.  Packed form (int16 only): 0 <= B <= 65534 under the preconditions,
// so two outputs share a 32-bit lane and the loop is v_pk_min_u16 / v_pk_max_u16; the operand B(i, k) is staged in both
// halves of its word.
//
// Tile kernel: a block of 256 threads owns one 128 x 128 tile (i-tile <= j-tile) of one base (grid.y), thread (ti, tj) of
// 16 x 16 an 8 x 8 register tile of running maxima.  k is walked in chunks of 32: thread (r = tid & 127, half = tid >> 7)
// forms the products of row r of both tiles with 16 positions of the chunk from D and the base's column and writes them to
// LDS as [k][r] (lanes run along r: conflict-free writes; reads are ds_read_b128 at a stride of 16 bytes per lane).  After
// the walk every thread subtracts B(i, j), formed the same way, keeps its best (value, i, j) under the order "larger value,
// then smaller i, then smaller j", the block folds them with a butterfly of that total order and writes ONE record.  The
// finishing kernel (one block per base) folds the records under the same order and walks k once more for the winning pair:
// the smallest k that attains the inner maximum.  Every output is written once by one thread; no atomics; no index is ever
// derived from matrix data.
#include "hm_common.h"
#include "hm_gromov_plan.h"

#pragma clang fp contract(off)

#define HM_GR_THREADS 256
#define HM_GR_HALF (HM_GR_TILE / 2)
#define HM_GR_STAGE 8                                          // positions a thread stages per round (it stages HM_GR_KCHUNK / 2 per chunk)
#define HM_GR_PAD_KEY ((int32_t)0x80000000)                    // below every key: a k, i or j past the end never wins

namespace {

typedef unsigned short hm_gr_u16x2 __attribute__((ext_vector_type(2)));

template <typename T> struct hm_gr_wide;
template <> struct hm_gr_wide<int16_t> { typedef int32_t type; };
template <> struct hm_gr_wide<float> { typedef float type; };

__device__ __forceinline__ int32_t hm_gr_fkey(float x)
{
    const int32_t b = __float_as_int(x);
    return b >= 0 ? b : b ^ 0x7fffffff;
}
__device__ __forceinline__ float hm_gr_funkey(int32_t k) { return __int_as_float(k >= 0 ? k : k ^ 0x7fffffff); }

// D(a, b) from the upper triangle; a, b in [0, n)
template <typename T>
__device__ __forceinline__ typename hm_gr_wide<T>::type hm_gr_D(const T* __restrict__ d, int64_t ld, int a, int b)
{
    const int lo = a < b ? a : b, hi = a < b ? b : a;
    return (typename hm_gr_wide<T>::type)d[(int64_t)lo * ld + hi];
}

// the product of (r, k) in the order domain from D(r, w), D(k, w), D(r, k)
__device__ __forceinline__ int32_t hm_gr_product(int32_t dr, int32_t dk, int32_t drk) { return dr + dk - drk; }
__device__ __forceinline__ int32_t hm_gr_product(float dr, float dk, float drk) { return hm_gr_fkey(0.5f * ((dr + dk) - drk) + 0.0f); }

// inner maximum minus the pair's own product, both in the order domain, result in the order domain
template <typename T> __device__ __forceinline__ int32_t hm_gr_minus(int32_t m, int32_t p);
template <> __device__ __forceinline__ int32_t hm_gr_minus<int16_t>(int32_t m, int32_t p) { return m - p; }
template <> __device__ __forceinline__ int32_t hm_gr_minus<float>(int32_t m, int32_t p) { return hm_gr_fkey(hm_gr_funkey(m) - hm_gr_funkey(p)); }

// (value, i, j): larger value first, then smaller i, then smaller j -- a total order, so a butterfly ends on the same record in every lane
struct hm_gr_best { int32_t v, i, j; };
__device__ __forceinline__ bool hm_gr_better(int32_t v, int32_t i, int32_t j, const hm_gr_best& o)
{
    return v > o.v || (v == o.v && (i < o.i || (i == o.i && j < o.j)));
}
__device__ __forceinline__ void hm_gr_wave_fold(hm_gr_best& b)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const int32_t v = __shfl_xor(b.v, off, 64), i = __shfl_xor(b.i, off, 64), j = __shfl_xor(b.j, off, 64);
        if (hm_gr_better(v, i, j, b)) { b.v = v; b.i = i; b.j = j; }
    }
}
// the block's best on every thread; s: one int4 per wave
__device__ __forceinline__ void hm_gr_block_fold(hm_gr_best& b, int4* s)
{
    hm_gr_wave_fold(b);
    const int wv = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s[wv] = make_int4(b.v, b.i, b.j, 0);
    __syncthreads();
    b = {s[0].x, s[0].y, s[0].z};
#pragma unroll
    for (int q = 1; q < HM_GR_THREADS / 64; ++q)
        if (hm_gr_better(s[q].x, s[q].y, s[q].z, b)) b = {s[q].x, s[q].y, s[q].z};
}

// rows of the register tile: local row of entry a (0..7) of thread coordinate t (0..15): 4 t + a and 64 + 4 t + (a - 4)
__device__ __forceinline__ int hm_gr_split_local(int t, int a) { return (a < 4 ? 0 : HM_GR_HALF - 4) + 4 * t + a; }

template <typename T, bool PACKED>
__global__ __launch_bounds__(HM_GR_THREADS) void hm_gromov_tile_kernel(const T* __restrict__ d, int n, int64_t ld,
                                                                        const int32_t* __restrict__ base, int nt, int64_t tiles,
                                                                        int4* __restrict__ rec)
{
    typedef typename hm_gr_wide<T>::type W;
    static_assert(!PACKED || sizeof(T) == 2, "the packed form takes int16 distances");
    // [k][r]; packed: sPi holds B(i, k) in both halves of a word, sPj is read as uint16 [k][128]
    __shared__ __attribute__((aligned(16))) uint32_t sPi[HM_GR_KCHUNK][HM_GR_TILE];
    __shared__ __attribute__((aligned(16))) uint32_t sPj[PACKED ? HM_GR_KCHUNK / 2 : HM_GR_KCHUNK][HM_GR_TILE];
    __shared__ W sDi[HM_GR_TILE], sDj[HM_GR_TILE];
    __shared__ int4 sfold[HM_GR_THREADS / 64];
    const int w = base[blockIdx.y];
    if (w < 0 || w >= n) return;                               // the whole block: the finishing kernel reports the base
    int ti, tj;
    hm_gr_tile_of(nt, blockIdx.x, &ti, &tj);
    const int I0 = ti * HM_GR_TILE, J0 = tj * HM_GR_TILE, tid = threadIdx.x;
    {
        const int r = (tid < HM_GR_TILE ? I0 : J0 - HM_GR_TILE) + tid;
        const W v = r < n ? hm_gr_D(d, ld, r, w) : (W)0;
        if (tid < HM_GR_TILE) sDi[tid] = v;
        else sDj[tid - HM_GR_TILE] = v;
    }
    __syncthreads();
    const int ty = tid >> 4, tx = tid & 15;
    // staging role
    const int sr = tid & (HM_GR_TILE - 1), sk = (tid >> 7) * (HM_GR_KCHUNK / 2);
    const int ri = I0 + sr, rj = J0 + sr, ric = min(ri, n - 1), rjc = min(rj, n - 1);
    const W dri = sDi[sr], drj = sDj[sr];
    const int32_t pad = PACKED ? 0 : HM_GR_PAD_KEY;

    int32_t acc[8][8];                                         // packed: acc[a][0..3] hold two outputs each
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
        for (int b = 0; b < 8; ++b) acc[a][b] = pad;

    for (int k0 = 0; k0 < n; k0 += HM_GR_KCHUNK) {
        // in rounds of HM_GR_STAGE positions: every load of a round is issued before the first is used.  The loads are
        // unconditional at clamped positions (a branch per element would wait for each load in turn: measured, the walk
        // of a small matrix spent its time there); what lies past the end is replaced afterwards.
#pragma unroll
        for (int q0 = 0; q0 < HM_GR_KCHUNK / 2; q0 += HM_GR_STAGE) {
            W dk[HM_GR_STAGE], dik[HM_GR_STAGE], djk[HM_GR_STAGE];
#pragma unroll
            for (int q = 0; q < HM_GR_STAGE; ++q) {
                const int kc = min(k0 + sk + q0 + q, n - 1);
                dk[q] = hm_gr_D(d, ld, kc, w);
                dik[q] = hm_gr_D(d, ld, ric, kc);
                djk[q] = ti == tj ? dik[q] : hm_gr_D(d, ld, rjc, kc);
            }
#pragma unroll
            for (int q = 0; q < HM_GR_STAGE; ++q) {
                const int kk = sk + q0 + q;
                const bool k_in = k0 + kk < n;
                const int32_t pi = k_in && ri < n ? hm_gr_product(dri, dk[q], dik[q]) : pad;
                const int32_t pj = k_in && rj < n ? hm_gr_product(drj, dk[q], djk[q]) : pad;
                if (PACKED) {
                    sPi[kk][sr] = ((uint32_t)pi & 0xffffu) | ((uint32_t)pi << 16);
                    reinterpret_cast<uint16_t*>(&sPj[0][0])[kk * HM_GR_TILE + sr] = (uint16_t)pj;
                } else {
                    sPi[kk][sr] = (uint32_t)pi;
                    sPj[kk][sr] = (uint32_t)pj;
                }
            }
        }
        __syncthreads();
#pragma unroll 4
        for (int kk = 0; kk < HM_GR_KCHUNK; ++kk) {
            const uint4 a0 = *reinterpret_cast<const uint4*>(&sPi[kk][4 * ty]);
            const uint4 a1 = *reinterpret_cast<const uint4*>(&sPi[kk][HM_GR_HALF + 4 * ty]);
            const uint32_t av[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
            if (PACKED) {
                const uint4 bw = *reinterpret_cast<const uint4*>(reinterpret_cast<const uint16_t*>(&sPj[0][0]) + kk * HM_GR_TILE + 8 * tx);
                const uint32_t bv[4] = {bw.x, bw.y, bw.z, bw.w};
#pragma unroll
                for (int a = 0; a < 8; ++a)
#pragma unroll
                    for (int p = 0; p < 4; ++p) {
                        const hm_gr_u16x2 m = __builtin_elementwise_min(__builtin_bit_cast(hm_gr_u16x2, av[a]), __builtin_bit_cast(hm_gr_u16x2, bv[p]));
                        acc[a][p] = __builtin_bit_cast(int32_t, __builtin_elementwise_max(__builtin_bit_cast(hm_gr_u16x2, acc[a][p]), m));
                    }
            } else {
                const uint4 b0 = *reinterpret_cast<const uint4*>(&sPj[kk][4 * tx]);
                const uint4 b1 = *reinterpret_cast<const uint4*>(&sPj[kk][HM_GR_HALF + 4 * tx]);
                const uint32_t bv[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
                for (int a = 0; a < 8; ++a)
#pragma unroll
                    for (int b = 0; b < 8; ++b) {
                        const int32_t m = min((int32_t)av[a], (int32_t)bv[b]);
                        acc[a][b] = max(acc[a][b], m);
                    }
            }
        }
        __syncthreads();
    }

    // the pair's own product and the block's best (value, i, j)
    hm_gr_best best = {HM_GR_PAD_KEY, 0x7fffffff, 0x7fffffff};
#pragma unroll
    for (int a = 0; a < 8; ++a) {
        const int il = hm_gr_split_local(ty, a), i = I0 + il;
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const int jl = PACKED ? 8 * tx + b : hm_gr_split_local(tx, b), j = J0 + jl;
            if (i >= n || j >= n || i > j) continue;
            const int32_t m = PACKED ? (int32_t)(((uint32_t)acc[a][b >> 1] >> (16 * (b & 1))) & 0xffffu) : acc[a][b];
            const int32_t p = hm_gr_product(sDi[il], sDj[jl], (W)d[(int64_t)i * ld + j]);
            const int32_t v = hm_gr_minus<T>(m, p);
            if (hm_gr_better(v, i, j, best)) best = {v, i, j};
        }
    }
    hm_gr_block_fold(best, sfold);
    if (tid == 0) rec[(int64_t)blockIdx.y * tiles + blockIdx.x] = make_int4(best.v, best.i, best.j, 0);
}

// one block per base: the best record in the fixed order, then the smallest k that attains the winning pair's inner maximum
template <typename T>
__global__ __launch_bounds__(HM_GR_THREADS) void hm_gromov_finish_kernel(const T* __restrict__ d, int n, int64_t ld,
                                                                          const int32_t* __restrict__ base, int64_t tiles,
                                                                          const int4* __restrict__ rec, void* __restrict__ value_out,
                                                                          int32_t* __restrict__ witness)
{
    typedef typename hm_gr_wide<T>::type W;
    __shared__ int4 sfold[HM_GR_THREADS / 64];
    const int64_t b = blockIdx.x;
    const int w = base[b], tid = threadIdx.x;
    if (w < 0 || w >= n) {
        if (tid == 0) {
            if (sizeof(T) == 2) static_cast<int32_t*>(value_out)[b] = -1;
            else static_cast<float*>(value_out)[b] = -1.0f;
            witness[3 * b] = witness[3 * b + 1] = witness[3 * b + 2] = -1;
        }
        return;
    }
    hm_gr_best best = {HM_GR_PAD_KEY, 0x7fffffff, 0x7fffffff};
    for (int64_t t = tid; t < tiles; t += HM_GR_THREADS) {
        const int4 r = rec[b * tiles + t];
        if (hm_gr_better(r.x, r.y, r.z, best)) best = {r.x, r.y, r.z};
    }
    hm_gr_block_fold(best, sfold);
    // the records hold positions the tile kernel wrote: i <= j < n.  Clamped all the same: a stale workspace cannot send a read astray
    const int i = min(max(best.i, 0), n - 1), j = min(max(best.j, 0), n - 1);
    const W diw = hm_gr_D(d, ld, i, w), djw = hm_gr_D(d, ld, j, w);
    // (inner value, k): larger value first, then smaller k; the same fold with k in the place of i
    hm_gr_best at = {HM_GR_PAD_KEY, 0x7fffffff, 0};
    for (int k = tid; k < n; k += HM_GR_THREADS) {
        const W dk = hm_gr_D(d, ld, k, w);
        const int32_t m = min(hm_gr_product(diw, dk, hm_gr_D(d, ld, i, k)), hm_gr_product(djw, dk, hm_gr_D(d, ld, j, k)));
        if (hm_gr_better(m, k, 0, at)) at = {m, k, 0};
    }
    hm_gr_block_fold(at, sfold);
    if (tid == 0) {
        if (sizeof(T) == 2) static_cast<int32_t*>(value_out)[b] = best.v;
        else static_cast<float*>(value_out)[b] = hm_gr_funkey(best.v);
        witness[3 * b] = i;
        witness[3 * b + 1] = j;
        witness[3 * b + 2] = at.i;
    }
}

// 0 = the default, 1 = int16 through the 32-bit path, 2 = int16 through the packed path (hm_debug_gromov_form)
int g_gr_form = 0;
#define HM_GR_DEFAULT_FORM 2

template <typename T, bool PACKED>
int hm_gromov_launch(const char* who, const T* d, int64_t n, int64_t ld, const int32_t* base, int64_t n_base, void* value_out,
                     int32_t* witness, void* workspace, void* stream)
{
    if (const int what = hm_gr_check_args(d, n, ld, base, n_base, value_out, witness, workspace))
        return hm_fail(nullptr, HM_E_ARG, std::string(who) + ": " + hm_gr_arg_text(what));
    if (n_base == 0) return HM_OK;
    const int64_t nt = hm_gr_edge_tiles(n), tiles = hm_gr_tiles(n);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL((hm_gromov_tile_kernel<T, PACKED>), dim3((unsigned)tiles, (unsigned)n_base), dim3(HM_GR_THREADS), 0, s, d, (int)n, ld,
                       base, (int)nt, tiles, static_cast<int4*>(workspace));
    HM_HIP0(hipGetLastError());
    hipLaunchKernelGGL(hm_gromov_finish_kernel<T>, dim3((unsigned)n_base), dim3(HM_GR_THREADS), 0, s, d, (int)n, ld, base, tiles,
                       static_cast<const int4*>(workspace), value_out, witness);
    HM_HIP0(hipGetLastError());
    return HM_OK;
}

}  // namespace

extern "C" int64_t hm_gromov_workspace_bytes(int64_t n, int64_t n_base) { return hm_gr_workspace_bytes(n, n_base); }

extern "C" int hm_gromov_delta_i16(const int16_t* d_dev, int64_t n, int64_t ld, const int32_t* base_dev, int64_t n_base,
                                   int32_t* value_out_dev, int32_t* witness_out_dev, void* workspace, void* stream)
{
    if ((g_gr_form ? g_gr_form : HM_GR_DEFAULT_FORM) == 2)
        return hm_gromov_launch<int16_t, true>("hm_gromov_delta_i16", d_dev, n, ld, base_dev, n_base, value_out_dev, witness_out_dev, workspace,
                                               stream);
    return hm_gromov_launch<int16_t, false>("hm_gromov_delta_i16", d_dev, n, ld, base_dev, n_base, value_out_dev, witness_out_dev, workspace,
                                            stream);
}

extern "C" int hm_gromov_delta_f32(const float* d_dev, int64_t n, int64_t ld, const int32_t* base_dev, int64_t n_base, float* value_out_dev,
                                   int32_t* witness_out_dev, void* workspace, void* stream)
{
    return hm_gromov_launch<float, false>("hm_gromov_delta_f32", d_dev, n, ld, base_dev, n_base, value_out_dev, witness_out_dev, workspace, stream);
}

extern "C" int hm_debug_gromov_form(int form)
{
    if (form < 0 || form > 2) return hm_fail(nullptr, HM_E_ARG, "hm_debug_gromov_form: form must be 0, 1 or 2");
    g_gr_form = form;
    return HM_OK;
}
