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
// Capacity: every slab is counted into a slab table (hm_table.h) of its own; when that overflows, the remaining blocks return
// at once and the host recounts the slab into a table four times larger (hm_count_growing; a table of 2 * positions slots
// cannot overflow).  The first slab's table becomes the counter's main table; a later slab's table is merged into it, after
// the main table has been grown (rehash on the device) to hold the exact number of distinct keys both hold, so the main table
// never overflows.
#include "hm_table.h"

struct hm_pairfreq;

namespace {

constexpr int64_t HM_PF_BIAS = 0x10FFFF + 2;                // -(2 + 0x10FFFF) -> 0
constexpr int HM_PF_BITS = 22;                              // 2^21 + HM_PF_BIAS < 2^22
constexpr unsigned long long HM_PF_FIELD = (1ull << HM_PF_BITS) - 1;   // a key never reaches HM_TABLE_EMPTY
constexpr int HM_PF_THREADS = 256;
constexpr int HM_PF_ITEMS = 32;                             // positions per thread: 8192 per block
constexpr int HM_PF_LDS_SLOTS = 4096;                       // 16 bytes each: 64 KiB
constexpr int HM_PF_LDS_PROBES = 32;

struct PfTable {
    HmTable t;                    // a slab table gives up after HM_TABLE_PROBES probes; the main table, sized to its exact
                                  // key count, probes up to the whole table
    unsigned long long* counts;   // [cap]
    unsigned long long* first;    // [cap] smallest flat position
};

__device__ __forceinline__ void hm_pf_insert(const PfTable& t, unsigned long long key, unsigned long long cnt,
                                             unsigned long long pos)
{
    const int64_t s = hm_table_claim(t.t, hm_mix64(key), key, [key](unsigned long long cur) { return cur == key; });
    if (s < 0) return;
    atomicAdd(&t.counts[s], cnt);
    atomicMin(&t.first[s], pos);
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
        s_key[s] = HM_TABLE_EMPTY;
        s_cnt[s] = 0;
        s_min[s] = 0xFFFFFFFFu;
    }
    if (threadIdx.x == 0) s_pairs = 0;
    __syncthreads();
    if (hm_table_overflowed(a.t.t)) return;                      // this slab is counted again into a larger table

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
        uint32_t h = (uint32_t)hm_mix64(key) & (HM_PF_LDS_SLOTS - 1);
        bool done = false;
        for (int probe = 0; probe < HM_PF_LDS_PROBES; ++probe) {
            const unsigned long long cur = atomicCAS(&s_key[h], HM_TABLE_EMPTY, key);
            if (cur == HM_TABLE_EMPTY || cur == key) {
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
        if (key != HM_TABLE_EMPTY)
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
    if (key != HM_TABLE_EMPTY) hm_pf_insert(dst, key, counts[s], first[s]);
}

struct Table {
    DevBuf<unsigned long long> keys, counts, first;
    int64_t cap() const { return keys.cap; }
};

// [0] main distinct  [1] slab distinct  [2] slab pairs  [3] compact count  [4] flags (two ints: slab, main overflow)
constexpr int HM_PF_WORDS = 5;

}  // namespace

struct hm_pairfreq {
    int device = 0;
    int64_t init_cap = 0;
    bool forced = false;                                    // initial capacity given by the caller (test hook)
    Table main, slab;
    DevBuf<unsigned long long> words;
    int64_t n_distinct = 0;                                 // occupied slots of the main table
    int64_t n_pairs = 0;
    int64_t slab_recounts = 0;
    int* flags() const { return reinterpret_cast<int*>(words.p + 4); }
};

namespace {

// an empty table of `cap` slots
int hm_pf_reset(Table& t, int64_t cap, hipStream_t st)
{
    if (int e = hm_column_reset(t.keys, cap, 0xFF, st)) return e;
    if (int e = hm_column_reset(t.counts, cap, 0, st)) return e;
    return hm_column_reset(t.first, cap, 0xFF, st);
}

PfTable hm_pf_view(const Table& t, unsigned long long* distinct, int* overflow, bool slab = false)
{
    return PfTable{hm_table_view(t.keys.p, t.cap(), distinct, overflow, slab), t.counts.p, t.first.p};
}

int64_t hm_pf_pow2(int64_t x) { return hm_pow2_at_least(x, 4); }

// every occupied slot of `src` into `dst` (the main table, or its successor), whose distinct count and overflow flag come
// back in `words`
int hm_pf_merge(hm_pairfreq* pf, const Table& src, const Table& dst, unsigned long long* words, hipStream_t st)
{
    HM_HIP0(hipMemsetAsync(pf->flags() + 1, 0, sizeof(int), st));
    hipLaunchKernelGGL(hm_pf_merge_kernel, dim3(hm_blocks(src.cap(), 256)), dim3(256), 0, st, src.keys.p, src.counts.p, src.first.p,
                       (uint64_t)src.cap(), hm_pf_view(dst, pf->words.p, pf->flags() + 1));
    HM_HIP0(hipGetLastError());
    HM_HIP0(hipMemcpyAsync(words, pf->words.p, sizeof(unsigned long long) * HM_PF_WORDS, hipMemcpyDeviceToHost, st));
    HM_HIP0(hipStreamSynchronize(st));
    return HM_OK;
}

// main table able to hold `need` distinct keys at load <= 1/2 (rehash of what it holds)
int hm_pf_reserve_main(hm_pairfreq* pf, int64_t need, hipStream_t st)
{
    if (pf->main.cap() && need <= pf->main.cap() / 2) return HM_OK;
    Table fresh;
    if (int e = hm_pf_reset(fresh, hm_pf_pow2(std::max<int64_t>(2 * need, pf->init_cap)), st)) return e;
    HM_HIP0(hipMemsetAsync(pf->words.p, 0, sizeof(unsigned long long), st));
    unsigned long long words[HM_PF_WORDS];
    if (pf->main.cap())
        if (int e = hm_pf_merge(pf, pf->main, fresh, words, st)) return e;
    pf->main = std::move(fresh);
    return HM_OK;
}

}  // namespace

extern "C" int hm_pairfreq_create(hm_pairfreq** out, int device, int64_t initial_capacity)
{
    if (int e = hm_check_create("hm_pairfreq_create", out, device, initial_capacity)) return e;
    HM_HIP0(hipSetDevice(device));
    std::unique_ptr<hm_pairfreq> pf(new hm_pairfreq());
    pf->device = device;
    pf->init_cap = hm_pf_pow2(initial_capacity ? initial_capacity : ((int64_t)1 << 16));
    pf->forced = initial_capacity != 0;
    if (pf->words.alloc(HM_PF_WORDS) != hipSuccess || hipMemset(pf->words.p, 0, sizeof(unsigned long long) * HM_PF_WORDS) != hipSuccess)
        return hm_fail(nullptr, HM_E_NOMEM, "hm_pairfreq_create: device allocation failed");
    *out = pf.release();
    return HM_OK;
}

extern "C" int hm_pairfreq_destroy(hm_pairfreq* pf)
{
    if (!pf) return HM_OK;
    (void)hipSetDevice(pf->device);          // every entry point synchronises its stream: nothing is in flight
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
    const int64_t bound = hm_pf_pow2(2 * n_positions);     // load <= 1/2 with every position a distinct pair
    // first guess: what earlier slabs needed, and (unless a tiny capacity was forced) one slot per 8 positions, at most 2^25
    int64_t guess = std::max<int64_t>(pf->init_cap, std::max<int64_t>(pf->slab.cap(), 2 * pf->n_distinct));
    if (!pf->forced) guess = std::max<int64_t>(guess, std::min<int64_t>(n_positions / 8, (int64_t)1 << 25));
    unsigned long long words[HM_PF_WORDS];
    auto count = [&](int64_t cap, bool* overflow) -> int {
        if (int e = hm_pf_reset(pf->slab, cap, st)) return e;
        HM_HIP0(hipMemsetAsync(pf->words.p + 1, 0, sizeof(unsigned long long) * 2, st));
        HM_HIP0(hipMemsetAsync(pf->flags(), 0, sizeof(int), st));
        CountArgs a;
        a.sym = sym_dev; a.off = offsets_dev; a.len = len_dev; a.n_lines = n_lines; a.n = n_positions;
        a.base = (unsigned long long)base; a.pairs = pf->words.p + 2;
        a.t = hm_pf_view(pf->slab, pf->words.p + 1, pf->flags(), cap < bound);   // at the bound: probe the whole table
        hipLaunchKernelGGL(hm_pf_count_kernel, dim3(hm_blocks(n_positions, HM_PF_THREADS * HM_PF_ITEMS)), dim3(HM_PF_THREADS), 0, st, a);
        HM_HIP0(hipGetLastError());
        HM_HIP0(hipMemcpyAsync(words, pf->words.p, sizeof(words), hipMemcpyDeviceToHost, st));
        HM_HIP0(hipStreamSynchronize(st));
        *overflow = reinterpret_cast<const int*>(words + 4)[0] != 0;
        return HM_OK;
    };
    if (int e = hm_count_growing("hm_pairfreq_add", std::min(bound, hm_pf_pow2(guess)), bound, pf->slab_recounts, count)) return e;
    const int64_t slab_n = (int64_t)words[1];
    pf->n_pairs += (int64_t)words[2];
    if (pf->n_distinct == 0) {                              // nothing counted yet: the slab table becomes the main table
        std::swap(pf->main, pf->slab);
        pf->n_distinct = slab_n;
        return HM_OK;
    }
    if (int e = hm_pf_reserve_main(pf, pf->n_distinct + slab_n, st)) return e;
    HM_HIP0(hipMemcpyAsync(pf->words.p, &pf->n_distinct, sizeof(int64_t), hipMemcpyHostToDevice, st));
    if (int e = hm_pf_merge(pf, pf->slab, pf->main, words, st)) return e;
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
    HM_HIP0(hipMemsetAsync(pf->words.p + 3, 0, sizeof(unsigned long long), st));
    HmColumns<2> cols{{pf->main.counts.p, pf->main.first.p},
                      {reinterpret_cast<unsigned long long*>(counts_dev), reinterpret_cast<unsigned long long*>(first_dev)}};
    hipLaunchKernelGGL(hm_table_compact_kernel<2>, dim3(hm_blocks(pf->main.cap(), 256)), dim3(256), 0, st, pf->main.keys.p, cols,
                       (uint64_t)pf->main.cap(), pf->words.p + 3, reinterpret_cast<unsigned long long*>(keys_dev), (uint64_t)out_cap);
    HM_HIP0(hipGetLastError());
    HM_HIP0(hipStreamSynchronize(st));
    return HM_OK;
}
