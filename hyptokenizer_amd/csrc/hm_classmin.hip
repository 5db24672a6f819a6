// hm_classmin.hip -- per-class running minima of the pair distance (HierarchicalHyperbolicTokenizer's step selection,
// DESIGN.md section 5.10).
//
// Every live row r carries a code c(r) in [0, HM_CM_CODES) set by the host (hm_classmin_set_codes).  A pair i < j
// belongs to class cls(c(i), c(j)) of the HM_CM_CLASSES unordered code pairs.  What is kept per class is the
// lexicographic minimum of (bits(d), i, j) over its pairs, d the canonical fp32 distance of the engine (the same u as
// hm_exact.hip and hm_newrow_key_kernel, hm::dist_from_u); NaN distances belong to no class.  No threshold: the host
// decides whether a minimum is a candidate (d < thr), so the state survives every threshold change.
//
//   hm_classmin_build   one pass over all pairs of the table: (bits(d), i) per class by atomicMin (LDS per block, then
//                       global), then the smallest j of each class's (d, i) by a row pass of row i -- 72 bits of key
//                       without a 72-bit atomic.
//   hm_classmin_fold    row m against rows [0, m): (bits(d), i) per class (j = m for all of them), and the host-listed
//                       partners of m (flag bits 28 / 29: the two exception lists) into two extra slots.
//
// Rows are only appended and existing distances never change, so the host keeps the running minima: after a merge
// the minimum of a class is lexmin(previous, fold of the new row).
#include "hm_table.h"
#include "hm_rows_device.h"

#pragma clang fp contract(off)

#define HM_CM_WAVES 3              // partner tiles per block of the build pass; LDS = (1 + HM_CM_WAVES) row tiles

struct hm_classmin {
    hm_engine* e = nullptr;
    DevBuf<uint8_t> d_codes;                   // [max_rows]
    DevBuf<unsigned long long> d_keys;         // [HM_CM_SLOTS] (bits(d) << 32) | partner
    DevBuf<unsigned long long, true> h_keys;   // pinned mirror
    DevBuf<int32_t> d_partners;                // fold: host-listed partners (index | flags)
    int64_t codes_set = 0;                     // rows [0, codes_set) have codes
};

namespace {

__host__ __device__ __forceinline__ int hm_cm_class(int a, int b)
{
    const int lo = a < b ? a : b, hi = a < b ? b : a;
    return lo * HM_CM_CODES - lo * (lo - 1) / 2 + (hi - lo);
}

// fold a key into an LDS slot: read first, the atomic only when it would lower the slot
__device__ __forceinline__ void hm_cm_lds_min(unsigned long long* slot, unsigned long long k)
{
    if (k < *reinterpret_cast<volatile unsigned long long*>(slot)) atomicMin(slot, k);
}

__device__ __forceinline__ void hm_cm_global_min(unsigned long long* slot, unsigned long long k)
{
    if (k < __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(slot, k);
}

struct BuildArgs {
    const float* img;
    const uint8_t* codes;
    int RS, d, sign_mode;
    float sqrt_c;
    int n;
    int ti0, ntj;
    unsigned long long* keys;      // [HM_CM_CLASSES]
};

// the tile decomposition of hm_exact_scan_kernel: block (x, y) = fixed row tile ti0 + y against HM_CM_WAVES partner tiles
// from the diagonal on, one lane per partner row
__global__ __launch_bounds__(64 * HM_CM_WAVES) void hm_cm_build_kernel(const BuildArgs a)
{
    extern __shared__ __align__(16) float lds[];
    __shared__ unsigned long long smin[HM_CM_CLASSES];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int tile_floats = HM_TILE_ROWS * a.RS;
    float* fixed = lds;
    float* tile = lds + (1 + wv) * tile_floats;
    const int ti = a.ti0 + (int)blockIdx.y;
    const int tj = ti + (int)blockIdx.x * HM_CM_WAVES + wv;
    const bool active = tj < a.ntj;
    TileRegs tr;
    if (active) hm_tile_load(a.img, a.RS, (int64_t)tj * HM_TILE_ROWS, a.n, tr, lane);
    {
        const int64_t r0 = (int64_t)ti * HM_TILE_ROWS;
        const int rows = (int)std::min<int64_t>(HM_TILE_ROWS, (int64_t)a.n - r0);
        const int nvec = rows > 0 ? rows * (a.RS >> 2) : 0;
        const uint4* src = reinterpret_cast<const uint4*>(a.img + r0 * a.RS);
        uint4* dst = reinterpret_cast<uint4*>(fixed);
        for (int q = threadIdx.x; q < HM_TILE_ROWS * (a.RS >> 2); q += blockDim.x) dst[q] = q < nvec ? src[q] : make_uint4(0, 0, 0, 0);
    }
    for (int q = threadIdx.x; q < HM_CM_CLASSES; q += blockDim.x) smin[q] = ~0ull;
    if (active) hm_tile_store(tile, a.RS, tr, lane);
    __syncthreads();
    if (active) {
        const int j = tj * HM_TILE_ROWS + lane;
        const int cj = j < a.n ? (int)a.codes[j] : 0;
        const int i_lo = ti * HM_TILE_ROWS, i_hi = std::min(a.n, (ti + 1) * HM_TILE_ROWS);
        for (int i = i_lo; i < i_hi; ++i) {
            const float u = hm_tile_u(tile, a.RS, a.d, fixed + (i - i_lo) * a.RS, a.sign_mode, lane);
            const float dd = hm::dist_from_u(u, a.sqrt_c);
            if (j > i && j < a.n && dd == dd) {
                const unsigned long long k = ((unsigned long long)hm::fbits(dd) << 32) | (unsigned long long)(uint32_t)i;
                hm_cm_lds_min(&smin[hm_cm_class((int)a.codes[i], cj)], k);
            }
        }
    }
    __syncthreads();
    for (int q = threadIdx.x; q < HM_CM_CLASSES; q += blockDim.x)
        if (smin[q] != ~0ull) hm_cm_global_min(&a.keys[q], smin[q]);
}

// row `row` against partner rows [p0, p1) (the row itself skipped): (bits(d) << 32) | partner per class into keys[0..CLASSES);
// blocks past the tiles take the host-listed partners: entry = index | (1 << 28) (slot CLASSES) | (1 << 29) (slot CLASSES + 1)
__global__ __launch_bounds__(64) void hm_cm_row_kernel(const float* __restrict__ img, const uint8_t* __restrict__ codes, int RS, int d,
                                                       int sign_mode, float sqrt_c, int64_t row, int64_t p0, int64_t p1,
                                                       const int32_t* __restrict__ partners, int64_t n_partners, int tile_blocks,
                                                       unsigned long long* __restrict__ keys)
{
    extern __shared__ __align__(16) float lds[];
    __shared__ unsigned long long smin[HM_CM_CLASSES];
    const int lane = threadIdx.x;
    if ((int)blockIdx.x >= tile_blocks) {           // the listed partners, one lane each (wave-uniform branch)
        unsigned long long k2 = ~0ull, k3 = ~0ull;
        for (int64_t q = (int64_t)(blockIdx.x - tile_blocks) * 64 + lane; q < n_partners; q += (int64_t)(gridDim.x - tile_blocks) * 64) {
            const uint32_t ent = (uint32_t)partners[q];
            const int64_t p = (int64_t)(ent & 0x0fffffffu);
            const float dd = hm::dist_from_u(hm_img_u(img, RS, d, row, p, sign_mode), sqrt_c);
            if (dd == dd) {
                const unsigned long long k = ((unsigned long long)hm::fbits(dd) << 32) | (unsigned long long)(uint32_t)p;
                if (ent & (1u << 28)) k2 = k < k2 ? k : k2;
                if (ent & (1u << 29)) k3 = k < k3 ? k : k3;
            }
        }
        k2 = hm_wave_min_u64(k2);
        k3 = hm_wave_min_u64(k3);
        if (lane == 0 && k2 != ~0ull) atomicMin(&keys[HM_CM_CLASSES], k2);
        if (lane == 0 && k3 != ~0ull) atomicMin(&keys[HM_CM_CLASSES + 1], k3);
        return;
    }
    float* xs = lds;
    float* tile = lds + HM_MAX_D1 + 4;
    for (int q = lane; q < HM_CM_CLASSES; q += 64) smin[q] = ~0ull;
    const int64_t t0 = p0 / HM_TILE_ROWS, nt = (p1 + HM_TILE_ROWS - 1) / HM_TILE_ROWS;
    int64_t tl = t0 + blockIdx.x;
    TileRegs tr;
    if (tl < nt) hm_tile_load(img, RS, tl * HM_TILE_ROWS, p1, tr, lane);
    for (int k = lane; k < RS; k += 64) xs[k] = img[row * RS + k];
    const int crow = (int)codes[row];
    hm_wave_lds_sync();
    for (; tl < nt; tl += tile_blocks) {
        hm_tile_store(tile, RS, tr, lane);
        hm_wave_lds_sync();
        const int64_t nxt = tl + tile_blocks;
        if (nxt < nt) hm_tile_load(img, RS, nxt * HM_TILE_ROWS, p1, tr, lane);
        const float u = hm_tile_u(tile, RS, d, xs, sign_mode, lane);
        const int64_t p = tl * HM_TILE_ROWS + lane;
        const float dd = hm::dist_from_u(u, sqrt_c);
        if (p >= p0 && p < p1 && p != row && dd == dd) {
            const unsigned long long k = ((unsigned long long)hm::fbits(dd) << 32) | (unsigned long long)(uint32_t)p;
            hm_cm_lds_min(&smin[hm_cm_class(crow, (int)codes[p])], k);
        }
        hm_wave_lds_sync();
    }
    for (int q = lane; q < HM_CM_CLASSES; q += 64)
        if (smin[q] != ~0ull) atomicMin(&keys[q], smin[q]);
}

int hm_cm_check(hm_classmin* cm, const char* what)
{
    if (!cm || !cm->e) return hm_fail(nullptr, HM_E_ARG, std::string(what) + ": NULL handle");
    return HM_OK;
}

size_t hm_cm_row_lds(hm_engine* e) { return sizeof(float) * ((size_t)HM_MAX_D1 + 4 + (size_t)HM_TILE_ROWS * e->RS); }

int hm_cm_set_attrs(hm_engine* e)
{
    const void* kb = reinterpret_cast<const void*>(&hm_cm_build_kernel);
    const void* kr = reinterpret_cast<const void*>(&hm_cm_row_kernel);
    if (e->attr_done.find(kb) == e->attr_done.end()) {
        HM_HIP(hipFuncSetAttribute(kb, hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)(sizeof(float) * (size_t)(1 + HM_CM_WAVES) * HM_TILE_ROWS * 4 * HM_TILE_MAXQ)));
        e->attr_done.insert(kb);
    }
    if (e->attr_done.find(kr) == e->attr_done.end()) {
        HM_HIP(hipFuncSetAttribute(kr, hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)(sizeof(float) * ((size_t)HM_MAX_D1 + 4 + (size_t)HM_TILE_ROWS * 4 * HM_TILE_MAXQ))));
        e->attr_done.insert(kr);
    }
    return HM_OK;
}

// keys[0..CLASSES) (and the two exception slots) <- min over row `row`'s partners in [p0, p1) and the listed partners
int hm_cm_row_launch(hm_classmin* cm, int64_t row, int64_t p0, int64_t p1, int64_t n_partners, float sqrt_c, hipStream_t s)
{
    hm_engine* e = cm->e;
    const int64_t nt = p1 > p0 ? (p1 + HM_TILE_ROWS - 1) / HM_TILE_ROWS - p0 / HM_TILE_ROWS : 0;
    const int tile_blocks = (int)std::max<int64_t>(1, std::min<int64_t>(nt, 1024));
    const int list_blocks = (int)std::min<int64_t>((n_partners + 63) / 64, 256);
    hipLaunchKernelGGL(hm_cm_row_kernel, dim3((unsigned)(tile_blocks + list_blocks)), dim3(64), hm_cm_row_lds(e), s, e->img, cm->d_codes.p,
                       e->RS, e->d, e->sign_mode, sqrt_c, row, p0, p1, (const int32_t*)cm->d_partners.p, n_partners, tile_blocks, cm->d_keys.p);
    HM_HIP(hipGetLastError());
    return HM_OK;
}

}  // namespace

extern "C" int hm_classmin_create(hm_classmin** out, hm_engine* e)
{
    if (!out) return hm_fail(nullptr, HM_E_ARG, "hm_classmin_create: out is NULL");
    *out = nullptr;
    if (!e) return hm_fail(nullptr, HM_E_ARG, "hm_classmin_create: engine is NULL");
    HM_HIP(hipSetDevice(e->device));
    std::unique_ptr<hm_classmin> cm(new hm_classmin());
    cm->e = e;
    if (cm->d_codes.alloc(e->max_rows) != hipSuccess || cm->d_keys.alloc(HM_CM_SLOTS) != hipSuccess
        || cm->h_keys.alloc(HM_CM_SLOTS) != hipSuccess || hipMemset(cm->d_codes.p, 0, (size_t)e->max_rows) != hipSuccess)
        return hm_fail(nullptr, HM_E_NOMEM, "hm_classmin_create: allocation failed");
    *out = cm.release();
    return HM_OK;
}

extern "C" int hm_classmin_destroy(hm_classmin* cm)
{
    if (!cm) return HM_OK;
    if (cm->e) (void)hipSetDevice(cm->e->device);   // every entry point synchronises its stream: nothing is in flight
    delete cm;
    return HM_OK;
}

extern "C" int hm_classmin_set_codes(hm_classmin* cm, const uint8_t* codes, int64_t row_begin, int64_t row_end, void* stream)
{
    if (int rc = hm_cm_check(cm, "hm_classmin_set_codes")) return rc;
    hm_engine* e = cm->e;
    if (row_begin < 0 || row_end < row_begin || row_end > e->max_rows || (row_end > row_begin && !codes))
        return hm_fail(e, HM_E_ARG, "hm_classmin_set_codes: bad row range");
    for (int64_t r = 0; r < row_end - row_begin; ++r)
        if (codes[r] >= HM_CM_CODES) return hm_fail(e, HM_E_ARG, "hm_classmin_set_codes: code out of range");
    if (row_end == row_begin) return HM_OK;
    HM_HIP(hipSetDevice(e->device));
    hipStream_t s = (hipStream_t)stream;
    HM_HIP(hipMemcpyAsync(cm->d_codes.p + row_begin, codes, (size_t)(row_end - row_begin), hipMemcpyHostToDevice, s));
    HM_HIP(hipStreamSynchronize(s));       // `codes` is pageable caller memory
    if (row_begin <= cm->codes_set) cm->codes_set = std::max(cm->codes_set, row_end);
    return HM_OK;
}

extern "C" int hm_classmin_build(hm_classmin* cm, float c, uint32_t* out, void* stream)
{
    if (int rc = hm_cm_check(cm, "hm_classmin_build")) return rc;
    hm_engine* e = cm->e;
    if (!out || !(c > 0.0f)) return hm_fail(e, HM_E_ARG, "hm_classmin_build: bad arguments");
    if (cm->codes_set < e->n) return hm_fail(e, HM_E_STATE, "hm_classmin_build: codes not set for every live row");
    HM_HIP(hipSetDevice(e->device));
    if (int rc = hm_cm_set_attrs(e)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const float sqrt_c = sqrtf(c);
    const int n = (int)e->n;
    HM_HIP(hipMemsetAsync(cm->d_keys.p, 0xff, sizeof(unsigned long long) * HM_CM_SLOTS, s));
    if (n >= 2) {
        BuildArgs a;
        a.img = e->img; a.codes = cm->d_codes.p; a.RS = e->RS; a.d = e->d; a.sign_mode = e->sign_mode; a.sqrt_c = sqrt_c; a.n = n;
        a.ntj = (n + HM_TILE_ROWS - 1) / HM_TILE_ROWS; a.keys = cm->d_keys.p;
        const size_t lds = sizeof(float) * (size_t)(1 + HM_CM_WAVES) * HM_TILE_ROWS * e->RS;
        for (int t0 = 0; t0 < a.ntj; t0 += 32768) {
            const int nt = std::min(32768, a.ntj - t0);
            a.ti0 = t0;
            const int groups = (a.ntj - t0 + HM_CM_WAVES - 1) / HM_CM_WAVES;
            hipLaunchKernelGGL(hm_cm_build_kernel, dim3((unsigned)groups, (unsigned)nt), dim3(64 * HM_CM_WAVES), lds, s, a);
            HM_HIP(hipGetLastError());
        }
    }
    HM_HIP(hipMemcpyAsync(cm->h_keys.p, cm->d_keys.p, sizeof(unsigned long long) * HM_CM_CLASSES, hipMemcpyDeviceToHost, s));
    HM_HIP(hipStreamSynchronize(s));
    unsigned long long first[HM_CM_CLASSES];
    memcpy(first, cm->h_keys.p, sizeof(first));
    // the smallest j of each class's (d, i): a row pass of row i over partners (i, n), one per distinct i
    for (int q = 0; q < HM_CM_CLASSES; ++q) {
        uint32_t* o = out + 4 * q;
        o[0] = 0; o[1] = 0; o[2] = 0xffffffffu; o[3] = 0xffffffffu;
    }
    for (int q = 0; q < HM_CM_CLASSES; ++q) {
        if (first[q] == ~0ull || out[4 * q] != 0) continue;
        const int64_t i = (int64_t)(uint32_t)first[q];
        HM_HIP(hipMemsetAsync(cm->d_keys.p, 0xff, sizeof(unsigned long long) * HM_CM_SLOTS, s));
        if (int rc = hm_cm_row_launch(cm, i, i + 1, n, 0, sqrt_c, s)) return rc;
        HM_HIP(hipMemcpyAsync(cm->h_keys.p, cm->d_keys.p, sizeof(unsigned long long) * HM_CM_CLASSES, hipMemcpyDeviceToHost, s));
        HM_HIP(hipStreamSynchronize(s));
        for (int r = q; r < HM_CM_CLASSES; ++r) {          // every class whose minimum sits on row i
            if (first[r] == ~0ull || (int64_t)(uint32_t)first[r] != i) continue;
            const unsigned long long k = cm->h_keys.p[r];
            if (k == ~0ull || (k >> 32) != (first[r] >> 32))
                return hm_fail(e, HM_E_STATE, "hm_classmin_build: row pass disagrees with the pair pass (internal error)");
            uint32_t* o = out + 4 * r;
            o[0] = 1; o[1] = (uint32_t)(k >> 32); o[2] = (uint32_t)i; o[3] = (uint32_t)k;
        }
    }
    return HM_OK;
}

extern "C" int hm_classmin_fold(hm_classmin* cm, int64_t row, float c, const int32_t* partners, int64_t n_partners, uint32_t* out,
                                void* stream)
{
    if (int rc = hm_cm_check(cm, "hm_classmin_fold")) return rc;
    hm_engine* e = cm->e;
    if (!out || !(c > 0.0f) || row < 0 || row >= e->n || n_partners < 0 || (n_partners > 0 && !partners))
        return hm_fail(e, HM_E_ARG, "hm_classmin_fold: bad arguments");
    if (cm->codes_set <= row) return hm_fail(e, HM_E_STATE, "hm_classmin_fold: codes not set up to this row");
    for (int64_t q = 0; q < n_partners; ++q) {
        const uint32_t ent = (uint32_t)partners[q];
        if ((int64_t)(ent & 0x0fffffffu) >= row || (ent & 0xc0000000u) != 0u)
            return hm_fail(e, HM_E_ARG, "hm_classmin_fold: partner not below the row, or unknown flag bits");
    }
    HM_HIP(hipSetDevice(e->device));
    if (int rc = hm_cm_set_attrs(e)) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (n_partners > 0) {
        HM_HIP(cm->d_partners.grow(std::max<int64_t>(1024, n_partners)));
        HM_HIP(hipMemcpyAsync(cm->d_partners.p, partners, sizeof(int32_t) * n_partners, hipMemcpyHostToDevice, s));
    }
    HM_HIP(hipMemsetAsync(cm->d_keys.p, 0xff, sizeof(unsigned long long) * HM_CM_SLOTS, s));
    if (int rc = hm_cm_row_launch(cm, row, 0, row, n_partners, sqrtf(c), s)) return rc;
    HM_HIP(hipMemcpyAsync(cm->h_keys.p, cm->d_keys.p, sizeof(unsigned long long) * HM_CM_SLOTS, hipMemcpyDeviceToHost, s));
    HM_HIP(hipStreamSynchronize(s));
    for (int q = 0; q < HM_CM_SLOTS; ++q) {
        const unsigned long long k = cm->h_keys.p[q];
        uint32_t* o = out + 4 * q;
        if (k == ~0ull) { o[0] = 0; o[1] = 0; o[2] = 0xffffffffu; o[3] = 0xffffffffu; continue; }
        o[0] = 1; o[1] = (uint32_t)(k >> 32); o[2] = (uint32_t)k; o[3] = (uint32_t)row;
    }
    return HM_OK;
}
