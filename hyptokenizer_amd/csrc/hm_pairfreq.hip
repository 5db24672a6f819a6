// hm_pairfreq.hip -- exact histogram of adjacent symbol pairs of a tokenised corpus, with the first position of every
// pair (FrequencyAwareHyperbolicTokenizer._compute_pair_frequencies, frequency_aware_hyperbolic_merge.py:92-112, and
// the same loop of EnhancedFastHyperbolicTokenizer, enhanced_fast_hyperbolic_merge.py:266-289).
//
// Input of one slab: the output of hm_tokenize_batch -- sym[], offsets[n + 1], out_len[n] (NULL: the whole line,
// offsets[l + 1] - offsets[l]).  Line l holds sym[offsets[l] .. offsets[l] + len[l]); every position p with p + 1 in
// the same line contributes the pair (sym[p], sym[p + 1]) at flat position base + p.  Positions are monotone in
// (slab, line, index in the line), so sorting the distinct pairs by their smallest position gives the order in which
// the reference's dict first meets them.
//
// Key: both symbols biased by HM_PF_BIAS (symbols lie in [-(2 + 0x10FFFF), 2^21): a rule or vocabulary symbol, or a
// character outside both as -(2 + ord(c))) into 22 bits each -- key = (a' << 22) | b', lossless; ~0 marks a free slot.
//
// Counting a slab (hm_pf_count_kernel): a block takes 256 * HM_PF_ITEMS consecutive positions and aggregates them in an
// LDS hash table (key, count, smallest position); it then flushes one global insert per distinct key (64-bit CAS on the
// key, 64-bit add, 64-bit min).  A key that finds no LDS slot within HM_PF_LDS_PROBES goes to the global table at once.
// Skewed text (a few pairs dominate) thus costs one global atomic per block and key instead of one per occurrence.
//
// Capacity: every slab is counted into a slab table of its own whose load is capped at one half; crossing the cap (or
// a probe sequence longer than HM_PF_SLAB_PROBES) raises an overflow flag, after which the table takes no new key and
// the remaining blocks return at once; the host recounts the slab into a table four times larger (a table of
// 2 * positions slots cannot overflow).  The first slab's table becomes the counter's main table; a later slab's table
// is merged into it, after the main table has been grown (rehash on the device) to hold the exact number of distinct
// keys both hold, so the main table never overflows.
#include "hm_common.h"

#include <algorithm>
#include <vector>

struct hm_pairfreq;

namespace {

constexpr unsigned long long HM_PF_EMPTY = ~0ull;
constexpr int64_t HM_PF_BIAS = 0x10FFFF + 2;                // -(2 + 0x10FFFF) -> 0
constexpr int HM_PF_BITS = 22;                              // 2^21 + HM_PF_BIAS < 2^22
constexpr unsigned long long HM_PF_FIELD = (1ull << HM_PF_BITS) - 1;   // a key never reaches HM_PF_EMPTY
constexpr int HM_PF_THREADS = 256;
constexpr int HM_PF_ITEMS = 32;                             // positions per thread: 8192 per block
constexpr int HM_PF_LDS_SLOTS = 4096;                       // 16 bytes each: 64 KiB
constexpr int HM_PF_LDS_PROBES = 32;
constexpr uint64_t HM_PF_SLAB_PROBES = 4096;                // a slab table that needs more is recounted larger

__host__ __device__ __forceinline__ uint64_t hm_pf_mix(uint64_t k)
{
    k ^= k >> 31;
    k *= 0x7fb5d329728ea185ull;
    k ^= k >> 27;
    k *= 0x81dadef4bc2dd44dull;
    k ^= k >> 33;
    return k;
}

struct PfTable {
    unsigned long long* keys;     // [cap], HM_PF_EMPTY when free
    unsigned long long* counts;   // [cap]
    unsigned long long* first;    // [cap] smallest flat position
    unsigned long long* distinct; // occupied slots
    int* overflow;                // set when more than `limit` slots were taken (or a probe ran round the table)
    uint64_t mask;                // cap - 1
    unsigned long long limit;     // cap / 2: load at most one half
    uint64_t max_probe;
};

__device__ __forceinline__ bool hm_pf_overflowed(const PfTable& t)
{
    return __hip_atomic_load(t.overflow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
}

// A slab table stops taking keys once it has overflowed (the slab is recounted), and gives up after max_probe probes;
// the main table is sized to its exact key count and probes up to the whole table.
__device__ __forceinline__ void hm_pf_insert(const PfTable& t, unsigned long long key, unsigned long long cnt,
                                             unsigned long long pos)
{
    uint64_t h = hm_pf_mix(key) & t.mask;
    for (uint64_t probe = 0; probe < t.max_probe; ++probe) {
        unsigned long long cur = __hip_atomic_load(&t.keys[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == HM_PF_EMPTY) {
            if (hm_pf_overflowed(t)) return;
            cur = atomicCAS(&t.keys[h], HM_PF_EMPTY, key);
            if (cur == HM_PF_EMPTY) {
                if (atomicAdd(t.distinct, 1ull) >= t.limit) atomicOr(t.overflow, 1);
                cur = key;
            }
        }
        if (cur == key) {
            atomicAdd(&t.counts[h], cnt);
            atomicMin(&t.first[h], pos);
            return;
        }
        h = (h + 1) & t.mask;
    }
    atomicOr(t.overflow, 1);
}

__device__ __forceinline__ int64_t hm_pf_len(const int64_t* __restrict__ off, const int32_t* __restrict__ len, int64_t l)
{
    const int64_t whole = off[l + 1] - off[l];
    return len ? min((int64_t)max(len[l], 0), whole) : whole;          // a tokenised line is never longer than its input
}

// line l with off[l] <= q < off[l + 1] (empty lines skipped), searched upwards from `lo` (off[lo] <= q): galloping, then
// bisection
__device__ __forceinline__ int64_t hm_pf_line(const int64_t* __restrict__ off, int64_t n_lines, int64_t lo, int64_t q)
{
    int64_t step = 1, hi = lo + 1;                          // invariant: off[lo] <= q; find the first hi with off[hi] > q
    while (hi < n_lines && off[hi] <= q) {
        lo = hi;
        step <<= 1;
        hi = min(lo + step, n_lines);
    }
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (off[mid] <= q) lo = mid;
        else hi = mid;
    }
    return lo;
}

struct CountArgs {
    const int32_t* sym;
    const int64_t* off;           // [n_lines + 1]
    const int32_t* len;           // [n_lines] or nullptr
    int64_t n_lines;
    int64_t n;                    // off[n_lines]
    unsigned long long base;      // flat position of sym[0]
    unsigned long long* pairs;    // total pairs of the slab
    PfTable t;
};

__global__ __launch_bounds__(HM_PF_THREADS) void hm_pf_count_kernel(CountArgs a)
{
    __shared__ unsigned long long s_key[HM_PF_LDS_SLOTS];
    __shared__ uint32_t s_cnt[HM_PF_LDS_SLOTS];
    __shared__ uint32_t s_min[HM_PF_LDS_SLOTS];
    __shared__ uint32_t s_pairs;
    for (int s = threadIdx.x; s < HM_PF_LDS_SLOTS; s += HM_PF_THREADS) {
        s_key[s] = HM_PF_EMPTY;
        s_cnt[s] = 0;
        s_min[s] = 0xFFFFFFFFu;
    }
    if (threadIdx.x == 0) s_pairs = 0;
    __syncthreads();
    if (hm_pf_overflowed(a.t)) return;                      // this slab is counted again into a larger table

    const int64_t q0 = (int64_t)blockIdx.x * (HM_PF_THREADS * HM_PF_ITEMS);
    int64_t line = -1, line_next = 0, line_end = 0;         // [off[line], line_end): positions whose successor is in the line
    uint32_t mine = 0;
    for (int it = 0; it < HM_PF_ITEMS; ++it) {
        const int64_t q = q0 + (int64_t)it * HM_PF_THREADS + threadIdx.x;
        if (q >= a.n) break;
        if (line < 0 || q >= line_next) {
            int64_t lo = 0;
            if (line >= 0) lo = line + 1;
            else {                                          // first position of this lane: bisection over all lines
                int64_t hi = a.n_lines;
                while (hi - lo > 1) {
                    const int64_t mid = lo + (hi - lo) / 2;
                    if (a.off[mid] <= q) lo = mid;
                    else hi = mid;
                }
            }
            line = hm_pf_line(a.off, a.n_lines, lo, q);
            line_next = a.off[line + 1];
            line_end = a.off[line] + max<int64_t>(hm_pf_len(a.off, a.len, line) - 1, 0);
        }
        if (q >= line_end || q < a.off[line]) continue;
        const unsigned long long key = ((((unsigned long long)((int64_t)a.sym[q] + HM_PF_BIAS)) & HM_PF_FIELD) << HM_PF_BITS)
                                     | (((unsigned long long)((int64_t)a.sym[q + 1] + HM_PF_BIAS)) & HM_PF_FIELD);
        const uint32_t rel = (uint32_t)(q - q0);
        ++mine;
        uint32_t h = (uint32_t)hm_pf_mix(key) & (HM_PF_LDS_SLOTS - 1);
        bool done = false;
        for (int probe = 0; probe < HM_PF_LDS_PROBES; ++probe) {
            const unsigned long long cur = atomicCAS(&s_key[h], HM_PF_EMPTY, key);
            if (cur == HM_PF_EMPTY || cur == key) {
                atomicAdd(&s_cnt[h], 1u);
                atomicMin(&s_min[h], rel);
                done = true;
                break;
            }
            h = (h + 1) & (HM_PF_LDS_SLOTS - 1);
        }
        if (!done) hm_pf_insert(a.t, key, 1ull, a.base + (unsigned long long)q);
    }
    if (mine) atomicAdd(&s_pairs, mine);
    __syncthreads();
    for (int s = threadIdx.x; s < HM_PF_LDS_SLOTS; s += HM_PF_THREADS) {
        const unsigned long long key = s_key[s];
        if (key != HM_PF_EMPTY)
            hm_pf_insert(a.t, key, (unsigned long long)s_cnt[s], a.base + (unsigned long long)(q0 + s_min[s]));
    }
    if (threadIdx.x == 0 && s_pairs) atomicAdd(a.pairs, (unsigned long long)s_pairs);
}

// every occupied slot of `src` into `dst` (merge of a slab table, rehash of the main table)
__global__ __launch_bounds__(256) void hm_pf_merge_kernel(const unsigned long long* __restrict__ keys,
                                                          const unsigned long long* __restrict__ counts,
                                                          const unsigned long long* __restrict__ first, uint64_t cap, PfTable dst)
{
    const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= cap) return;
    const unsigned long long key = keys[s];
    if (key != HM_PF_EMPTY) hm_pf_insert(dst, key, counts[s], first[s]);
}

// occupied slots, compacted in any order (the host sorts by first position, which is unique per key)
__global__ __launch_bounds__(256) void hm_pf_compact_kernel(PfTable t, uint64_t cap, unsigned long long* __restrict__ n_out,
                                                            unsigned long long* __restrict__ keys_out,
                                                            unsigned long long* __restrict__ counts_out,
                                                            unsigned long long* __restrict__ first_out, uint64_t out_cap)
{
    const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= cap) return;
    const unsigned long long key = t.keys[s];
    if (key == HM_PF_EMPTY) return;
    const unsigned long long k = atomicAdd(n_out, 1ull);
    if (k >= out_cap) return;
    keys_out[k] = key;
    counts_out[k] = t.counts[s];
    first_out[k] = t.first[s];
}

struct Table {
    unsigned long long* keys = nullptr;
    unsigned long long* counts = nullptr;
    unsigned long long* first = nullptr;
    int64_t cap = 0;
};

// [0] main distinct  [1] slab distinct  [2] slab pairs  [3] compact count  [4] flags (two ints: slab, main overflow)
constexpr int HM_PF_WORDS = 5;

}  // namespace

struct hm_pairfreq {
    int device = 0;
    int64_t init_cap = 0;
    bool forced = false;                                    // initial capacity given by the caller (test hook)
    Table main, slab;
    unsigned long long* words = nullptr;
    int64_t n_distinct = 0;                                 // occupied slots of the main table
    int64_t n_pairs = 0;
    int64_t slab_recounts = 0;
};

namespace {

void hm_pf_free(Table& t)
{
    for (void* p : {(void*)t.keys, (void*)t.counts, (void*)t.first}) if (p) (void)hipFree(p);
    t = Table{};
}

int hm_pf_alloc(Table& t, int64_t cap, hipStream_t st)
{
    hm_pf_free(t);
    HM_HIP0(hipMalloc(&t.keys, sizeof(unsigned long long) * cap));
    HM_HIP0(hipMalloc(&t.counts, sizeof(unsigned long long) * cap));
    HM_HIP0(hipMalloc(&t.first, sizeof(unsigned long long) * cap));
    t.cap = cap;
    HM_HIP0(hipMemsetAsync(t.keys, 0xFF, sizeof(unsigned long long) * cap, st));
    HM_HIP0(hipMemsetAsync(t.counts, 0, sizeof(unsigned long long) * cap, st));
    HM_HIP0(hipMemsetAsync(t.first, 0xFF, sizeof(unsigned long long) * cap, st));
    return HM_OK;
}

PfTable hm_pf_view(const Table& t, unsigned long long* distinct, int* overflow, bool slab = false)
{
    PfTable v;
    v.keys = t.keys; v.counts = t.counts; v.first = t.first;
    v.distinct = distinct; v.overflow = overflow;
    v.mask = (uint64_t)t.cap - 1;
    v.limit = (unsigned long long)(t.cap / 2);
    v.max_probe = slab ? std::min<uint64_t>(HM_PF_SLAB_PROBES, (uint64_t)t.cap) : (uint64_t)t.cap;
    return v;
}

int64_t hm_pf_pow2(int64_t x)
{
    int64_t c = 4;
    while (c < x) c <<= 1;
    return c;
}

unsigned hm_pf_blocks(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

// main table able to hold `need` distinct keys at load <= 1/2 (rehash of what it holds)
int hm_pf_reserve_main(hm_pairfreq* pf, int64_t need, hipStream_t st)
{
    if (pf->main.cap && need <= pf->main.cap / 2) return HM_OK;
    const int64_t cap = hm_pf_pow2(std::max<int64_t>(2 * need, pf->init_cap));
    Table fresh;
    if (int e = hm_pf_alloc(fresh, cap, st)) { hm_pf_free(fresh); return e; }
    int* flags = reinterpret_cast<int*>(pf->words + 4);
    HM_HIP0(hipMemsetAsync(pf->words, 0, sizeof(unsigned long long), st));
    HM_HIP0(hipMemsetAsync(flags + 1, 0, sizeof(int), st));
    if (pf->main.cap) {
        hipLaunchKernelGGL(hm_pf_merge_kernel, dim3(hm_pf_blocks(pf->main.cap, 256)), dim3(256), 0, st,
                           pf->main.keys, pf->main.counts, pf->main.first, (uint64_t)pf->main.cap,
                           hm_pf_view(fresh, pf->words, flags + 1));
        HM_HIP0(hipGetLastError());
    }
    HM_HIP0(hipStreamSynchronize(st));
    hm_pf_free(pf->main);
    pf->main = fresh;
    return HM_OK;
}

}  // namespace

extern "C" int hm_pairfreq_create(hm_pairfreq** out, int device, int64_t initial_capacity)
{
    if (!out) return hm_fail(nullptr, HM_E_ARG, "hm_pairfreq_create: out is NULL");
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return hm_fail(nullptr, HM_E_ARG, "hm_pairfreq_create: no HIP device available (the counter has no CPU fallback)");
    if (device < 0 || device >= ndev) return hm_fail(nullptr, HM_E_ARG, "hm_pairfreq_create: bad device index");
    if (initial_capacity < 0 || initial_capacity > ((int64_t)1 << 40))
        return hm_fail(nullptr, HM_E_ARG, "hm_pairfreq_create: initial_capacity must lie in [0, 2^40]");
    HM_HIP0(hipSetDevice(device));
    hm_pairfreq* pf = new hm_pairfreq();
    pf->device = device;
    pf->init_cap = hm_pf_pow2(initial_capacity ? initial_capacity : ((int64_t)1 << 16));
    pf->forced = initial_capacity != 0;
    if (hipMalloc(&pf->words, sizeof(unsigned long long) * HM_PF_WORDS) != hipSuccess
        || hipMemset(pf->words, 0, sizeof(unsigned long long) * HM_PF_WORDS) != hipSuccess) {
        if (pf->words) (void)hipFree(pf->words);
        delete pf;
        return hm_fail(nullptr, HM_E_NOMEM, "hm_pairfreq_create: device allocation failed");
    }
    *out = pf;
    return HM_OK;
}

extern "C" int hm_pairfreq_destroy(hm_pairfreq* pf)
{
    if (!pf) return HM_OK;
    (void)hipSetDevice(pf->device);          // every entry point synchronises its stream: nothing is in flight
    hm_pf_free(pf->main);
    hm_pf_free(pf->slab);
    if (pf->words) (void)hipFree(pf->words);
    delete pf;
    return HM_OK;
}

extern "C" int hm_pairfreq_add(hm_pairfreq* pf, const int32_t* sym_dev, const int64_t* offsets_dev, const int32_t* len_dev,
                               int64_t n_lines, int64_t n_positions, int64_t base, void* stream)
{
    if (!pf) return hm_fail(nullptr, HM_E_ARG, "hm_pairfreq_add: NULL counter");
    if (n_lines < 0 || n_positions < 0 || base < 0 || (n_lines > 0 && !offsets_dev) || (n_positions > 0 && !sym_dev))
        return hm_fail(nullptr, HM_E_ARG, "hm_pairfreq_add: NULL pointer or negative size");
    if (n_positions >= ((int64_t)1 << 40) || base > ((int64_t)1 << 62) - n_positions)
        return hm_fail(nullptr, HM_E_ARG, "hm_pairfreq_add: 2^40 positions per slab, flat positions below 2^62");
    if (n_lines == 0 || n_positions < 2) return HM_OK;
    HM_HIP0(hipSetDevice(pf->device));
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* slab_distinct = pf->words + 1;
    unsigned long long* slab_pairs = pf->words + 2;
    int* flags = reinterpret_cast<int*>(pf->words + 4);
    const int64_t bound = hm_pf_pow2(2 * n_positions);     // load <= 1/2 with every position a distinct pair
    // first guess: what earlier slabs needed, and (unless a tiny capacity was forced) one slot per 8 positions, at most 2^25
    int64_t guess = std::max<int64_t>(pf->init_cap, std::max<int64_t>(pf->slab.cap, 2 * pf->n_distinct));
    if (!pf->forced) guess = std::max<int64_t>(guess, std::min<int64_t>(n_positions / 8, (int64_t)1 << 25));
    int64_t cap = std::min(bound, hm_pf_pow2(guess));
    unsigned long long words[HM_PF_WORDS];
    for (;;) {
        if (pf->slab.cap != cap) {
            if (int e = hm_pf_alloc(pf->slab, cap, st)) return e;
        } else {
            HM_HIP0(hipMemsetAsync(pf->slab.keys, 0xFF, sizeof(unsigned long long) * cap, st));
            HM_HIP0(hipMemsetAsync(pf->slab.counts, 0, sizeof(unsigned long long) * cap, st));
            HM_HIP0(hipMemsetAsync(pf->slab.first, 0xFF, sizeof(unsigned long long) * cap, st));
        }
        HM_HIP0(hipMemsetAsync(pf->words + 1, 0, sizeof(unsigned long long) * 2, st));
        HM_HIP0(hipMemsetAsync(flags, 0, sizeof(int), st));
        CountArgs a;
        a.sym = sym_dev; a.off = offsets_dev; a.len = len_dev; a.n_lines = n_lines; a.n = n_positions;
        a.base = (unsigned long long)base; a.pairs = slab_pairs;
        a.t = hm_pf_view(pf->slab, slab_distinct, flags, cap < bound);   // at the bound: probe the whole table
        hipLaunchKernelGGL(hm_pf_count_kernel, dim3(hm_pf_blocks(n_positions, HM_PF_THREADS * HM_PF_ITEMS)),
                           dim3(HM_PF_THREADS), 0, st, a);
        HM_HIP0(hipGetLastError());
        HM_HIP0(hipMemcpyAsync(words, pf->words, sizeof(words), hipMemcpyDeviceToHost, st));
        HM_HIP0(hipStreamSynchronize(st));
        const int* fl = reinterpret_cast<const int*>(words + 4);
        if (!fl[0]) break;
        if (cap >= bound)
            return hm_fail(nullptr, HM_E_STATE, "hm_pairfreq_add: overflow of a table sized for every position (internal error)");
        cap = std::min(bound, 4 * cap);                     // recount the slab into a larger table
        ++pf->slab_recounts;
    }
    const int64_t slab_n = (int64_t)words[1];
    pf->n_pairs += (int64_t)words[2];
    if (pf->n_distinct == 0) {                              // nothing counted yet: the slab table becomes the main table
        std::swap(pf->main, pf->slab);
        pf->n_distinct = slab_n;
        return HM_OK;
    }
    if (int e = hm_pf_reserve_main(pf, pf->n_distinct + slab_n, st)) return e;
    HM_HIP0(hipMemcpyAsync(pf->words, &pf->n_distinct, sizeof(int64_t), hipMemcpyHostToDevice, st));
    HM_HIP0(hipMemsetAsync(flags + 1, 0, sizeof(int), st));
    hipLaunchKernelGGL(hm_pf_merge_kernel, dim3(hm_pf_blocks(cap, 256)), dim3(256), 0, st,
                       pf->slab.keys, pf->slab.counts, pf->slab.first, (uint64_t)cap, hm_pf_view(pf->main, pf->words, flags + 1));
    HM_HIP0(hipGetLastError());
    HM_HIP0(hipMemcpyAsync(words, pf->words, sizeof(words), hipMemcpyDeviceToHost, st));
    HM_HIP0(hipStreamSynchronize(st));
    if (reinterpret_cast<const int*>(words + 4)[1])
        return hm_fail(nullptr, HM_E_STATE, "hm_pairfreq_add: main table overflow (internal error)");
    pf->n_distinct = (int64_t)words[0];
    return HM_OK;
}

extern "C" int hm_pairfreq_read(hm_pairfreq* pf, int64_t* n_distinct, int64_t* n_pairs, int64_t* slab_recounts,
                                uint64_t* keys_dev, uint64_t* counts_dev, int64_t* first_dev, int64_t out_cap, void* stream)
{
    if (!pf) return hm_fail(nullptr, HM_E_ARG, "hm_pairfreq_read: NULL counter");
    if (n_distinct) *n_distinct = pf->n_distinct;
    if (n_pairs) *n_pairs = pf->n_pairs;
    if (slab_recounts) *slab_recounts = pf->slab_recounts;
    if (!keys_dev && !counts_dev && !first_dev) return HM_OK;
    if (!keys_dev || !counts_dev || !first_dev) return hm_fail(nullptr, HM_E_ARG, "hm_pairfreq_read: give all three arrays or none");
    if (out_cap < pf->n_distinct) return hm_fail(nullptr, HM_E_CAPACITY, "hm_pairfreq_read: out_cap below the distinct count");
    if (pf->n_distinct == 0) return HM_OK;
    HM_HIP0(hipSetDevice(pf->device));
    hipStream_t st = (hipStream_t)stream;
    HM_HIP0(hipMemsetAsync(pf->words + 3, 0, sizeof(unsigned long long), st));
    hipLaunchKernelGGL(hm_pf_compact_kernel, dim3(hm_pf_blocks(pf->main.cap, 256)), dim3(256), 0, st,
                       hm_pf_view(pf->main, pf->words, reinterpret_cast<int*>(pf->words + 4) + 1), (uint64_t)pf->main.cap,
                       pf->words + 3, reinterpret_cast<unsigned long long*>(keys_dev),
                       reinterpret_cast<unsigned long long*>(counts_dev), reinterpret_cast<unsigned long long*>(first_dev),
                       (uint64_t)out_cap);
    HM_HIP0(hipGetLastError());
    HM_HIP0(hipStreamSynchronize(st));
    return HM_OK;
}
