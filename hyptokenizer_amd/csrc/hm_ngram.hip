// hm_ngram.hip -- exact histogram of the character n-grams (n = 2..5) of a list of words
// (HierarchicalHyperbolicTokenizer._compute_corpus_statistics).
//
// Input: distinct words as code points, cps[offsets[w] .. offsets[w + 1]), and one int64 weight per word.  Every position p of
// word w with p + n <= end(w) holds the n-gram cps[p .. p + n):
//   HM_NGRAM_WEIGHTED  count(g) = sum over occurrences of weight(w)      (the reference's per-occurrence loop over a Counter
//                      of words: a word met k times adds its n-grams k times)
//   HM_NGRAM_DISTINCT  count(g) = number of words that contain g          (each word at most once, weights ignored)
//
// Key: a slot of the counting table (hm_table.h) holds a REFERENCE to the first occurrence that claimed it, (n << 56) | p --
// the code points themselves are read from the input when two references meet, so any code point (21 bits) and any word
// length are exact without packing 105 bits of key (n <= 5 never makes a top byte of 0xff, the free slot).  Counts are 64-bit
// adds.  The distinct mode also keeps a set of (slot, word) pairs in a second table: only a pair's first insertion adds 1.
//
// Capacity: when either table overflows, the host recounts into tables four times larger (hm_count_growing); tables of
// 2 x occurrences slots cannot overflow.
#include "hm_table.h"

namespace {

constexpr int HM_NG_THREADS = 256;

struct NgArgs {
    const int32_t* cps;
    const int64_t* off;             // [n_words + 1]
    const int64_t* weight;          // [n_words] (weighted mode)
    int64_t n_words, n_pos;
    int mode;
    HmTable grams, seen;            // one overflow flag for both; seen: the (slot, word) set of the distinct mode
    unsigned long long* counts;     // [slots of grams]
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
    for (int k = 0; k < n; ++k) h = hm_mix64(h ^ ((uint64_t)(uint32_t)a.cps[p + k] + 0x9e3779b97f4a7c15ull * (uint64_t)(k + 1)));
    const unsigned long long ref = ((unsigned long long)n << 56) | (unsigned long long)p;
    return hm_table_claim(a.grams, h, ref, [&](unsigned long long cur) { return hm_ng_same(a.cps, cur, p, n); });
}

__global__ __launch_bounds__(HM_NG_THREADS) void hm_ng_count_kernel(const NgArgs a)
{
    const int64_t stride = (int64_t)gridDim.x * HM_NG_THREADS;
    for (int64_t p = (int64_t)blockIdx.x * HM_NG_THREADS + threadIdx.x; p < a.n_pos; p += stride) {
        if (*reinterpret_cast<volatile int*>(a.grams.overflow)) return;
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
                atomicAdd(&a.counts[s], (unsigned long long)a.weight[w]);
            } else {                                           // only a (slot, word) pair's first insertion adds 1
                const unsigned long long key = ((unsigned long long)s << 32) | (unsigned long long)(uint32_t)w;
                bool fresh = false;
                if (hm_table_claim(a.seen, hm_mix64(key), key, [key](unsigned long long cur) { return cur == key; }, &fresh) < 0) return;
                if (fresh) atomicAdd(&a.counts[s], 1ull);
            }
        }
    }
}

int64_t hm_ng_pow2(int64_t x) { return hm_pow2_at_least(x, 1024); }

}  // namespace

struct hm_ngram {
    int device = 0;
    int64_t init_cap = 0;
    bool forced = false;
    DevBuf<unsigned long long> keys, counts, seen;   // seen is released by a weighted count
    DevBuf<unsigned long long> words;                // [0] distinct grams [1] distinct (gram, word) [2] compacted [3] flag
    int64_t n_distinct = 0, recounts = 0;
};

extern "C" int hm_ngram_create(hm_ngram** out, int device, int64_t initial_capacity)
{
    if (int e = hm_check_create("hm_ngram_create", out, device, initial_capacity)) return e;
    HM_HIP0(hipSetDevice(device));
    std::unique_ptr<hm_ngram> g(new hm_ngram());
    g->device = device;
    g->init_cap = hm_ng_pow2(initial_capacity ? initial_capacity : ((int64_t)1 << 16));
    g->forced = initial_capacity != 0;
    if (g->words.alloc(4) != hipSuccess) return hm_fail(nullptr, HM_E_NOMEM, "hm_ngram_create: device allocation failed");
    *out = g.release();
    return HM_OK;
}

extern "C" int hm_ngram_destroy(hm_ngram* g)
{
    if (!g) return HM_OK;
    (void)hipSetDevice(g->device);           // every entry point synchronises its stream: nothing is in flight
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
    // inputs to the device (every pointer below is checked against its own size by the kernel's loop bounds); every return
    // below follows a stream synchronisation or frees them, which waits for the device
    DevBuf<int32_t> d_cps;
    DevBuf<int64_t> d_off, d_w;
    HM_HIP0(d_cps.alloc(n_pos));
    HM_HIP0(d_off.alloc(n_words + 1));
    HM_HIP0(hipMemcpyAsync(d_cps.p, cps, sizeof(int32_t) * n_pos, hipMemcpyHostToDevice, st));
    HM_HIP0(hipMemcpyAsync(d_off.p, offsets, sizeof(int64_t) * (n_words + 1), hipMemcpyHostToDevice, st));
    if (mode == HM_NGRAM_WEIGHTED) {
        HM_HIP0(d_w.alloc(n_words));
        HM_HIP0(hipMemcpyAsync(d_w.p, weights, sizeof(int64_t) * n_words, hipMemcpyHostToDevice, st));
    }
    const int64_t bound = hm_ng_pow2(2 * occ);
    int64_t guess = g->init_cap;
    if (!g->forced) guess = std::max<int64_t>(guess, std::min<int64_t>(occ / 4, (int64_t)1 << 25));
    unsigned long long words[4];
    auto count = [&](int64_t cap, bool* overflow) -> int {
        if (int e = hm_column_reset(g->keys, cap, 0xFF, st)) return e;
        if (int e = hm_column_reset(g->counts, cap, 0, st)) return e;
        if (mode == HM_NGRAM_WEIGHTED) g->seen.release();
        else if (int e = hm_column_reset(g->seen, cap, 0xFF, st)) return e;
        HM_HIP0(hipMemsetAsync(g->words.p, 0, sizeof(words), st));
        int* flag = reinterpret_cast<int*>(g->words.p + 3);
        NgArgs a;
        a.cps = d_cps.p; a.off = d_off.p; a.weight = d_w.p; a.n_words = n_words; a.n_pos = n_pos; a.mode = mode;
        a.grams = hm_table_view(g->keys.p, cap, g->words.p, flag, cap < bound);      // at the bound: probe the whole table
        a.seen = hm_table_view(g->seen.p, g->seen.cap, g->words.p + 1, flag, cap < bound);
        a.counts = g->counts.p;
        const int64_t blocks = std::min<int64_t>((n_pos + HM_NG_THREADS - 1) / HM_NG_THREADS, 65536);
        hipLaunchKernelGGL(hm_ng_count_kernel, dim3((unsigned)std::max<int64_t>(1, blocks)), dim3(HM_NG_THREADS), 0, st, a);
        HM_HIP0(hipGetLastError());
        HM_HIP0(hipMemcpyAsync(words, g->words.p, sizeof(words), hipMemcpyDeviceToHost, st));
        HM_HIP0(hipStreamSynchronize(st));
        *overflow = *reinterpret_cast<const int*>(words + 3) != 0;
        return HM_OK;
    };
    if (int e = hm_count_growing("hm_ngram_count", std::min(bound, hm_ng_pow2(guess)), bound, g->recounts, count)) return e;
    g->n_distinct = (int64_t)words[0];
    if (n_distinct) *n_distinct = g->n_distinct;
    return HM_OK;
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
    DevBuf<unsigned long long> d_ref, d_cnt;
    HM_HIP0(d_ref.alloc(g->n_distinct));
    HM_HIP0(d_cnt.alloc(g->n_distinct));
    std::vector<unsigned long long> ref((size_t)g->n_distinct);
    HM_HIP0(hipMemsetAsync(g->words.p + 2, 0, sizeof(unsigned long long), st));
    hipLaunchKernelGGL(hm_table_compact_kernel<1>, dim3(hm_blocks(g->keys.cap, 256)), dim3(256), 0, st, g->keys.p,
                       HmColumns<1>{{g->counts.p}, {d_cnt.p}}, (uint64_t)g->keys.cap, g->words.p + 2, d_ref.p, (uint64_t)g->n_distinct);
    HM_HIP0(hipGetLastError());
    HM_HIP0(hipMemcpyAsync(ref.data(), d_ref.p, sizeof(unsigned long long) * g->n_distinct, hipMemcpyDeviceToHost, st));
    HM_HIP0(hipMemcpyAsync(counts, d_cnt.p, sizeof(int64_t) * g->n_distinct, hipMemcpyDeviceToHost, st));
    HM_HIP0(hipStreamSynchronize(st));
    for (int64_t k = 0; k < g->n_distinct; ++k) {
        pos[k] = (int64_t)(ref[k] & ((1ull << 56) - 1));
        len[k] = (int32_t)(ref[k] >> 56);
    }
    return HM_OK;
}
