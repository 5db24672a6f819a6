// hm_ngram.hip -- exact histogram of the character n-grams (n = 2..5) of a list of words
// (HierarchicalHyperbolicTokenizer._compute_corpus_statistics).
//
// Input: distinct words as code points, cps[offsets[w] .. offsets[w + 1]), and one int64 weight per word.  Every position p of
// word w with p + n <= end(w) holds the n-gram cps[p .. p + n):
//   HM_NGRAM_WEIGHTED  count(g) = sum over occurrences of weight(w)      (the reference's per-occurrence loop over a Counter
//                      of words: a word met k times adds its n-grams k times)
//   HM_NGRAM_DISTINCT  count(g) = number of words that contain g          (each word at most once, weights ignored)
//
// Key: a slot holds a REFERENCE to the first occurrence that claimed it, (n << 56) | p -- the code points themselves are read
// from the input when two references meet, so any code point (21 bits) and any word length are exact without packing 105 bits
// of key.  ~0 marks a free slot (n <= 5 never makes a top byte of 0xff).  Inserting: 64-bit CAS of the reference into a free
// slot, or compare the n code points with those of the slot's reference; linear probing.  Counts are 64-bit adds.
// The distinct mode also keeps a set of (slot, word) pairs (64-bit keys, CAS): only a pair's first insertion adds 1.
//
// Capacity: both tables are capped at load 1/2; crossing the cap or a probe sequence longer than HM_NG_PROBES raises an
// overflow flag, after which no key is inserted and the host recounts into tables four times larger.  A table of
// 2 x occurrences slots cannot overflow.
#include "hm_common.h"

#include <algorithm>

#pragma clang fp contract(off)

namespace {

constexpr unsigned long long HM_NG_EMPTY = ~0ull;
constexpr int HM_NG_THREADS = 256;
constexpr uint64_t HM_NG_PROBES = 4096;

__host__ __device__ __forceinline__ uint64_t hm_ng_mix(uint64_t k)
{
    k ^= k >> 31;
    k *= 0x7fb5d329728ea185ull;
    k ^= k >> 27;
    k *= 0x81dadef4bc2dd44dull;
    k ^= k >> 33;
    return k;
}

struct NgTable {
    unsigned long long* keys;
    unsigned long long* counts;     // NULL for the (slot, word) set
    uint64_t mask, limit, max_probe;
    unsigned long long* distinct;
};

struct NgArgs {
    const int32_t* cps;
    const int64_t* off;             // [n_words + 1]
    const int64_t* weight;          // [n_words] (weighted mode)
    int64_t n_words, n_pos;
    int mode;
    NgTable grams, seen;
    int* overflow;
};

__device__ __forceinline__ bool hm_ng_same(const int32_t* cps, uint64_t ref, int64_t p, int n)
{
    if ((int)(ref >> 56) != n) return false;
    const int64_t q = (int64_t)(ref & ((1ull << 56) - 1));
    for (int k = 0; k < n; ++k)
        if (cps[q + k] != cps[p + k]) return false;
    return true;
}

// slot of the n-gram at p in the gram table (inserted when new); -1 on overflow
__device__ __forceinline__ int64_t hm_ng_gram_slot(const NgArgs& a, int64_t p, int n)
{
    uint64_t h = (uint64_t)n;
    for (int k = 0; k < n; ++k) h = hm_ng_mix(h ^ ((uint64_t)(uint32_t)a.cps[p + k] + 0x9e3779b97f4a7c15ull * (uint64_t)(k + 1)));
    const unsigned long long ref = ((unsigned long long)n << 56) | (unsigned long long)p;
    uint64_t slot = h & a.grams.mask;
    for (uint64_t probe = 0; probe < a.grams.max_probe; ++probe, slot = (slot + 1) & a.grams.mask) {
        unsigned long long cur = __hip_atomic_load(&a.grams.keys[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == HM_NG_EMPTY) {
            const unsigned long long prev = atomicCAS(&a.grams.keys[slot], HM_NG_EMPTY, ref);
            if (prev == HM_NG_EMPTY) {
                if (atomicAdd(a.grams.distinct, 1ull) + 1ull > a.grams.limit) { atomicExch(a.overflow, 1); return -1; }
                return (int64_t)slot;
            }
            cur = prev;
        }
        if (hm_ng_same(a.cps, cur, p, n)) return (int64_t)slot;
    }
    atomicExch(a.overflow, 1);
    return -1;
}

// insert (slot, word) into the set; true when it was not there yet
__device__ __forceinline__ bool hm_ng_first_in_word(const NgArgs& a, int64_t gslot, int64_t w, bool* ok)
{
    const unsigned long long key = ((unsigned long long)gslot << 32) | (unsigned long long)(uint32_t)w;
    uint64_t slot = hm_ng_mix(key) & a.seen.mask;
    for (uint64_t probe = 0; probe < a.seen.max_probe; ++probe, slot = (slot + 1) & a.seen.mask) {
        unsigned long long cur = __hip_atomic_load(&a.seen.keys[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == HM_NG_EMPTY) {
            const unsigned long long prev = atomicCAS(&a.seen.keys[slot], HM_NG_EMPTY, key);
            if (prev == HM_NG_EMPTY) {
                if (atomicAdd(a.seen.distinct, 1ull) + 1ull > a.seen.limit) { atomicExch(a.overflow, 1); *ok = false; return false; }
                return true;
            }
            cur = prev;
        }
        if (cur == key) return false;
    }
    atomicExch(a.overflow, 1);
    *ok = false;
    return false;
}

__global__ __launch_bounds__(HM_NG_THREADS) void hm_ng_count_kernel(const NgArgs a)
{
    const int64_t stride = (int64_t)gridDim.x * HM_NG_THREADS;
    for (int64_t p = (int64_t)blockIdx.x * HM_NG_THREADS + threadIdx.x; p < a.n_pos; p += stride) {
        if (*reinterpret_cast<volatile int*>(a.overflow)) return;
        // word of position p: the last w with off[w] <= p (empty words share offsets: the last of them is the one that holds p)
        int64_t lo = 0, hi = a.n_words;                        // off[lo] <= p < off[hi]
        while (hi - lo > 1) {
            const int64_t mid = (lo + hi) >> 1;
            if (a.off[mid] <= p) lo = mid; else hi = mid;
        }
        const int64_t w = lo, end = a.off[w + 1];
        for (int n = 2; n <= 5 && p + n <= end; ++n) {
            const int64_t s = hm_ng_gram_slot(a, p, n);
            if (s < 0) return;
            if (a.mode == HM_NGRAM_WEIGHTED) {
                atomicAdd(&a.grams.counts[s], (unsigned long long)a.weight[w]);
            } else {
                bool ok = true;
                if (hm_ng_first_in_word(a, s, w, &ok)) atomicAdd(&a.grams.counts[s], 1ull);
                if (!ok) return;
            }
        }
    }
}

__global__ void hm_ng_compact_kernel(const unsigned long long* __restrict__ keys, const unsigned long long* __restrict__ counts, uint64_t cap,
                                     unsigned long long* __restrict__ n_out, unsigned long long* __restrict__ out_ref,
                                     unsigned long long* __restrict__ out_count, uint64_t out_cap)
{
    const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= cap || keys[s] == HM_NG_EMPTY) return;
    const unsigned long long at = atomicAdd(n_out, 1ull);
    if (at < out_cap) { out_ref[at] = keys[s]; out_count[at] = counts[s]; }
}

int64_t hm_ng_pow2(int64_t x)
{
    int64_t c = 1024;
    while (c < x) c <<= 1;
    return c;
}

}  // namespace

struct hm_ngram {
    int device = 0;
    int64_t init_cap = 0;
    bool forced = false;
    unsigned long long* keys = nullptr;
    unsigned long long* counts = nullptr;
    unsigned long long* seen = nullptr;
    int64_t cap = 0, seen_cap = 0;
    unsigned long long* words = nullptr;       // [0] distinct grams [1] distinct (gram, word) [2] compacted [3] flag
    int64_t n_distinct = 0, recounts = 0;
};

namespace {

void hm_ng_free(hm_ngram* g)
{
    for (void* p : {(void*)g->keys, (void*)g->counts, (void*)g->seen}) if (p) (void)hipFree(p);
    g->keys = g->counts = g->seen = nullptr;
    g->cap = g->seen_cap = 0;
}

}  // namespace

extern "C" int hm_ngram_create(hm_ngram** out, int device, int64_t initial_capacity)
{
    if (!out) return hm_fail(nullptr, HM_E_ARG, "hm_ngram_create: out is NULL");
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return hm_fail(nullptr, HM_E_ARG, "hm_ngram_create: no HIP device available (the counter has no CPU fallback)");
    if (device < 0 || device >= ndev) return hm_fail(nullptr, HM_E_ARG, "hm_ngram_create: bad device index");
    if (initial_capacity < 0 || initial_capacity > ((int64_t)1 << 40))
        return hm_fail(nullptr, HM_E_ARG, "hm_ngram_create: initial_capacity must lie in [0, 2^40]");
    HM_HIP0(hipSetDevice(device));
    hm_ngram* g = new hm_ngram();
    g->device = device;
    g->init_cap = hm_ng_pow2(initial_capacity ? initial_capacity : ((int64_t)1 << 16));
    g->forced = initial_capacity != 0;
    if (hipMalloc(&g->words, sizeof(unsigned long long) * 4) != hipSuccess) {
        delete g;
        return hm_fail(nullptr, HM_E_NOMEM, "hm_ngram_create: device allocation failed");
    }
    *out = g;
    return HM_OK;
}

extern "C" int hm_ngram_destroy(hm_ngram* g)
{
    if (!g) return HM_OK;
    (void)hipSetDevice(g->device);
    hm_ng_free(g);
    if (g->words) (void)hipFree(g->words);
    delete g;
    return HM_OK;
}

extern "C" int hm_ngram_count(hm_ngram* g, const int32_t* cps, const int64_t* offsets, const int64_t* weights, int64_t n_words, int mode,
                              int64_t* n_distinct, void* stream)
{
    if (!g) return hm_fail(nullptr, HM_E_ARG, "hm_ngram_count: NULL counter");
    if (n_words < 0 || (n_words > 0 && !offsets) || (mode != HM_NGRAM_WEIGHTED && mode != HM_NGRAM_DISTINCT)
        || (mode == HM_NGRAM_WEIGHTED && n_words > 0 && !weights) || n_words >= ((int64_t)1 << 32))
        return hm_fail(nullptr, HM_E_ARG, "hm_ngram_count: bad arguments");
    g->n_distinct = 0;
    if (n_distinct) *n_distinct = 0;
    if (n_words == 0) return HM_OK;
    const int64_t n_pos = offsets[n_words];
    if (offsets[0] != 0 || n_pos < 0 || n_pos >= ((int64_t)1 << 40) || (n_pos > 0 && !cps))
        return hm_fail(nullptr, HM_E_ARG, "hm_ngram_count: offsets must start at 0 and end below 2^40");
    int64_t occ = 0;
    for (int64_t w = 0; w < n_words; ++w) {
        const int64_t L = offsets[w + 1] - offsets[w];
        if (L < 0) return hm_fail(nullptr, HM_E_ARG, "hm_ngram_count: offsets must not decrease");
        for (int n = 2; n <= 5; ++n) occ += std::max<int64_t>(0, L - n + 1);
        if (mode == HM_NGRAM_WEIGHTED && weights[w] < 0) return hm_fail(nullptr, HM_E_ARG, "hm_ngram_count: negative weight");
    }
    if (occ == 0) return HM_OK;
    HM_HIP0(hipSetDevice(g->device));
    hipStream_t st = (hipStream_t)stream;
    // inputs to the device (every pointer below is checked against its own size by the kernel's loop bounds)
    int32_t* d_cps = nullptr;
    int64_t *d_off = nullptr, *d_w = nullptr;
    auto release = [&]() {
        if (d_cps) (void)hipFree(d_cps);
        if (d_off) (void)hipFree(d_off);
        if (d_w) (void)hipFree(d_w);
    };
    if (hipMalloc(&d_cps, sizeof(int32_t) * std::max<int64_t>(1, n_pos)) != hipSuccess
        || hipMalloc(&d_off, sizeof(int64_t) * (n_words + 1)) != hipSuccess
        || (mode == HM_NGRAM_WEIGHTED && hipMalloc(&d_w, sizeof(int64_t) * n_words) != hipSuccess)) {
        release();
        return hm_fail(nullptr, HM_E_NOMEM, "hm_ngram_count: device allocation failed");
    }
    if (hipMemcpyAsync(d_cps, cps, sizeof(int32_t) * n_pos, hipMemcpyHostToDevice, st) != hipSuccess
        || hipMemcpyAsync(d_off, offsets, sizeof(int64_t) * (n_words + 1), hipMemcpyHostToDevice, st) != hipSuccess
        || (d_w && hipMemcpyAsync(d_w, weights, sizeof(int64_t) * n_words, hipMemcpyHostToDevice, st) != hipSuccess)) {
        release();
        return hm_fail(nullptr, HM_E_STATE, "hm_ngram_count: upload failed");
    }
    const int64_t bound = hm_ng_pow2(2 * occ);
    int64_t guess = g->init_cap;
    if (!g->forced) guess = std::max<int64_t>(guess, std::min<int64_t>(occ / 4, (int64_t)1 << 25));
    int64_t cap = std::min(bound, hm_ng_pow2(guess));
    unsigned long long words[4];
    int rc = HM_OK;
    for (;;) {
        const int64_t seen_cap = mode == HM_NGRAM_DISTINCT ? cap : 0;
        if (g->cap != cap || g->seen_cap != seen_cap) {
            hm_ng_free(g);
            if (hipMalloc(&g->keys, sizeof(unsigned long long) * cap) != hipSuccess
                || hipMalloc(&g->counts, sizeof(unsigned long long) * cap) != hipSuccess
                || (seen_cap && hipMalloc(&g->seen, sizeof(unsigned long long) * seen_cap) != hipSuccess)) {
                hm_ng_free(g);
                rc = hm_fail(nullptr, HM_E_NOMEM, "hm_ngram_count: table allocation failed");
                break;
            }
            g->cap = cap;
            g->seen_cap = seen_cap;
        }
        if (hipMemsetAsync(g->keys, 0xFF, sizeof(unsigned long long) * cap, st) != hipSuccess
            || hipMemsetAsync(g->counts, 0, sizeof(unsigned long long) * cap, st) != hipSuccess
            || (seen_cap && hipMemsetAsync(g->seen, 0xFF, sizeof(unsigned long long) * seen_cap, st) != hipSuccess)
            || hipMemsetAsync(g->words, 0, sizeof(unsigned long long) * 4, st) != hipSuccess) {
            rc = hm_fail(nullptr, HM_E_STATE, "hm_ngram_count: table reset failed");
            break;
        }
        NgArgs a;
        a.cps = d_cps; a.off = d_off; a.weight = d_w; a.n_words = n_words; a.n_pos = n_pos; a.mode = mode;
        a.grams.keys = g->keys; a.grams.counts = g->counts; a.grams.mask = (uint64_t)cap - 1; a.grams.limit = (uint64_t)cap / 2;
        a.grams.max_probe = cap < bound ? std::min<uint64_t>(HM_NG_PROBES, (uint64_t)cap) : (uint64_t)cap;
        a.grams.distinct = g->words;
        a.seen.keys = g->seen; a.seen.counts = nullptr; a.seen.mask = seen_cap ? (uint64_t)seen_cap - 1 : 0;
        a.seen.limit = (uint64_t)seen_cap / 2;
        a.seen.max_probe = seen_cap < bound ? std::min<uint64_t>(HM_NG_PROBES, (uint64_t)std::max<int64_t>(1, seen_cap)) : (uint64_t)seen_cap;
        a.seen.distinct = g->words + 1;
        a.overflow = reinterpret_cast<int*>(g->words + 3);
        const int64_t blocks = std::min<int64_t>((n_pos + HM_NG_THREADS - 1) / HM_NG_THREADS, 65536);
        hipLaunchKernelGGL(hm_ng_count_kernel, dim3((unsigned)std::max<int64_t>(1, blocks)), dim3(HM_NG_THREADS), 0, st, a);
        if (hipGetLastError() != hipSuccess
            || hipMemcpyAsync(words, g->words, sizeof(words), hipMemcpyDeviceToHost, st) != hipSuccess
            || hipStreamSynchronize(st) != hipSuccess) {
            rc = hm_fail(nullptr, HM_E_STATE, "hm_ngram_count: count kernel failed");
            break;
        }
        if (!*reinterpret_cast<const int*>(words + 3)) {
            g->n_distinct = (int64_t)words[0];
            break;
        }
        if (cap >= bound) {
            rc = hm_fail(nullptr, HM_E_STATE, "hm_ngram_count: overflow of a table sized for every occurrence (internal error)");
            break;
        }
        cap = std::min(bound, 4 * cap);                    // recount into larger tables
        ++g->recounts;
    }
    (void)hipStreamSynchronize(st);
    release();
    if (rc == HM_OK && n_distinct) *n_distinct = g->n_distinct;
    return rc;
}

extern "C" int hm_ngram_read(hm_ngram* g, int64_t* pos, int32_t* len, int64_t* counts, int64_t out_cap, int64_t* recounts, void* stream)
{
    if (!g) return hm_fail(nullptr, HM_E_ARG, "hm_ngram_read: NULL counter");
    if (recounts) *recounts = g->recounts;
    if (!pos && !len && !counts) return HM_OK;
    if (!pos || !len || !counts) return hm_fail(nullptr, HM_E_ARG, "hm_ngram_read: give all three arrays or none");
    if (out_cap < g->n_distinct) return hm_fail(nullptr, HM_E_CAPACITY, "hm_ngram_read: out_cap below the distinct count");
    if (g->n_distinct == 0) return HM_OK;
    HM_HIP0(hipSetDevice(g->device));
    hipStream_t st = (hipStream_t)stream;
    unsigned long long *d_ref = nullptr, *d_cnt = nullptr;
    if (hipMalloc(&d_ref, sizeof(unsigned long long) * g->n_distinct) != hipSuccess
        || hipMalloc(&d_cnt, sizeof(unsigned long long) * g->n_distinct) != hipSuccess) {
        if (d_ref) (void)hipFree(d_ref);
        return hm_fail(nullptr, HM_E_NOMEM, "hm_ngram_read: device allocation failed");
    }
    std::vector<unsigned long long> ref((size_t)g->n_distinct);
    int rc = HM_OK;
    if (hipMemsetAsync(g->words + 2, 0, sizeof(unsigned long long), st) != hipSuccess) rc = HM_E_STATE;
    if (rc == HM_OK) {
        hipLaunchKernelGGL(hm_ng_compact_kernel, dim3((unsigned)((g->cap + 255) / 256)), dim3(256), 0, st, g->keys, g->counts,
                           (uint64_t)g->cap, g->words + 2, d_ref, d_cnt, (uint64_t)g->n_distinct);
        if (hipGetLastError() != hipSuccess
            || hipMemcpyAsync(ref.data(), d_ref, sizeof(unsigned long long) * g->n_distinct, hipMemcpyDeviceToHost, st) != hipSuccess
            || hipMemcpyAsync(counts, d_cnt, sizeof(int64_t) * g->n_distinct, hipMemcpyDeviceToHost, st) != hipSuccess
            || hipStreamSynchronize(st) != hipSuccess)
            rc = HM_E_STATE;
    }
    (void)hipFree(d_ref);
    (void)hipFree(d_cnt);
    if (rc != HM_OK) return hm_fail(nullptr, rc, "hm_ngram_read: compaction failed");
    for (int64_t k = 0; k < g->n_distinct; ++k) {
        pos[k] = (int64_t)(ref[k] & ((1ull << 56) - 1));
        len[k] = (int32_t)(ref[k] >> 56);
    }
    return HM_OK;
}
