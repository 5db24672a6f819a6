// hm_greedy.hip -- greedy longest-match token counts of a corpus sample under "vocabulary + one candidate string", for
// many candidates at once (CompressionAwareTokenizer._compression_aware_scoring, compression_aware_tokenizer.py:91-190,
// and the compression term of EnhancedFastHyperbolicTokenizer, enhanced_fast_hyperbolic_merge.py:849-899).
//
// The reference's rule: at position p take the longest vocabulary entry that is a prefix of text[p:], else the single
// character text[p].  Everything here works on Unicode code points (int32), the positions of Python's str.
//
// State of one matcher (independent of any engine, like hm_tokenize.hip):
//   corpus    cp[N] code points of the representative lines, off[R + 1], mult[R] (int64), line_of[N]
//   vocabulary  every appended string in a host pool; for full builds a device copy and an open-addressing set keyed by
//             (length, 64-bit FNV-1a hash); every hit is verified code point by code point, so nothing is probabilistic
//   lm[N]     length of the longest vocabulary string that starts at p (1 when none: the character fallback)
//   base[R]   greedy token count of every line under the vocabulary
// Strings are only ever appended (rows are never removed), so a new string t only raises lm:
// lm[p] = max(lm[p], |t|) wherever t occurs -- one parallel pass over the corpus per merge, no rebuild.
//
// Scoring K candidates m_c: under vocabulary + {m_c} the walk is  p += max(lm[p], |m_c| if m_c matches at p), so a
// line's count can only differ from base[l] when m_c matches somewhere in it with |m_c| > lm[p].
//   phase 1  one lane per corpus position: mark the (candidate, line) pairs with such an improvement site
//   phase 2  one wave per (line, 64 candidates), lines longest first: marked lanes walk the line, the others take
//            base[l]; lanes of a wave share the line's cache lines.  counts[c][l] (optional) and
//            totals[c] = sum_l mult[l] * count[c][l] (int64 atomics).
#include "hm_table.h"

namespace {

constexpr int HM_GR_DIRECT_MAX = 64;        // appends of at most this many strings update lm directly, more rebuild it
constexpr uint64_t HM_GR_FNV_BASIS = 0xcbf29ce484222325ull;
constexpr uint64_t HM_GR_FNV_PRIME = 0x100000001b3ull;

__host__ __device__ __forceinline__ uint64_t hm_gr_step(uint64_t h, int32_t cp)
{
    return (h ^ (uint64_t)(uint32_t)cp) * HM_GR_FNV_PRIME;
}
__host__ __device__ __forceinline__ uint64_t hm_gr_slot(uint64_t h, int32_t len, uint64_t mask)
{
    return ((h ^ ((uint64_t)(uint32_t)len * 0x9E3779B97F4A7C15ull)) * 0xD6E8FEB86659FD93ull >> 17) & mask;
}

struct SetEntry {               // 16 bytes; len == 0: free
    uint64_t h;
    int32_t len;
    int32_t str;                // index into the pool's offsets
};

// lm of every position from the hashed set: extend the hash one code point at a time and probe the lengths that exist
__global__ __launch_bounds__(256) void hm_greedy_build_kernel(const int32_t* __restrict__ cp, const int32_t* __restrict__ line_of,
                                                               const int64_t* __restrict__ off, int64_t n,
                                                               const SetEntry* __restrict__ set, uint64_t mask,
                                                               const uint8_t* __restrict__ has_len, int32_t max_len,
                                                               const int32_t* __restrict__ pool, const int64_t* __restrict__ pool_off,
                                                               int32_t* __restrict__ lm)
{
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const int64_t rem = off[line_of[p] + 1] - p;
    const int32_t lim = (int32_t)min((int64_t)max_len, rem);
    int32_t best = 1;
    uint64_t h = HM_GR_FNV_BASIS;
    for (int32_t k = 1; k <= lim; ++k) {
        h = hm_gr_step(h, cp[p + k - 1]);
        if (!has_len[k]) continue;
        for (uint64_t s = hm_gr_slot(h, k, mask);; s = (s + 1) & mask) {
            const SetEntry e = set[s];
            if (e.len == 0) break;
            if (e.len != k || e.h != h) continue;
            const int32_t* t = pool + pool_off[e.str];
            int32_t q = 0;
            while (q < k && t[q] == cp[p + q]) ++q;
            if (q == k) { best = k; break; }
        }
    }
    lm[p] = best;
}

// lm[p] = max(lm[p], |t|) for the appended strings t that occur at p (first code point filters)
__global__ __launch_bounds__(256) void hm_greedy_append_kernel(const int32_t* __restrict__ cp, const int32_t* __restrict__ line_of,
                                                                const int64_t* __restrict__ off, int64_t n,
                                                                const int32_t* __restrict__ str, const int64_t* __restrict__ str_off,
                                                                int32_t n_str, int32_t* __restrict__ lm)
{
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const int64_t rem = off[line_of[p] + 1] - p;
    const int32_t c0 = cp[p];
    int32_t best = lm[p];
    for (int32_t s = 0; s < n_str; ++s) {
        const int64_t b = str_off[s];
        const int64_t len = str_off[s + 1] - b;
        if (len <= best || len > rem || str[b] != c0) continue;
        int64_t q = 1;
        while (q < len && str[b + q] == cp[p + q]) ++q;
        if (q == len) best = (int32_t)len;
    }
    lm[p] = best;
}

__global__ __launch_bounds__(64) void hm_greedy_base_kernel(const int64_t* __restrict__ off, const int32_t* __restrict__ lm,
                                                             int64_t n_lines, int32_t* __restrict__ base)
{
    const int64_t l = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= n_lines) return;
    const int64_t end = off[l + 1];
    int32_t count = 0;
    for (int64_t p = off[l]; p < end; p += lm[p]) ++count;
    base[l] = count;
}

struct CountArgs {
    const int32_t* cp;
    const int32_t* line_of;
    const int64_t* off;
    const int64_t* mult;
    const int32_t* lm;
    const int32_t* base;
    const int32_t* order;       // lines, longest first
    int64_t n, n_lines;
    const int32_t* cand;        // candidate code points
    const int64_t* cand_off;    // [k + 1]
    int32_t k;
    int32_t k_waves;            // ceil(k / 64)
    uint8_t* mark;              // [k][n_lines]
    int32_t* counts;            // [k][n_lines] or nullptr
    unsigned long long* totals; // [k]
};

__device__ __forceinline__ bool hm_gr_match(const int32_t* __restrict__ cp, int64_t p, const int32_t* __restrict__ t, int64_t len)
{
    int64_t q = 1;                            // t[0] == cp[p] is checked by the caller
    while (q < len && t[q] == cp[p + q]) ++q;
    return q == len;
}

// phase 1: the candidate loop is uniform across the wave (its operands come through scalar loads)
__global__ __launch_bounds__(256) void hm_greedy_mark_kernel(CountArgs a)
{
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.n) return;
    const int32_t l = a.line_of[p];
    const int64_t rem = a.off[l + 1] - p;
    const int32_t c0 = a.cp[p], have = a.lm[p];
    for (int32_t c = 0; c < a.k; ++c) {
        const int64_t b = a.cand_off[c];
        const int64_t len = a.cand_off[c + 1] - b;
        if (len <= have || len > rem || a.cand[b] != c0) continue;
        if (hm_gr_match(a.cp, p, a.cand + b, len)) a.mark[(int64_t)c * a.n_lines + l] = 1;
    }
}

// phase 2: wave w takes line order[w / k_waves] and candidates 64 * (w % k_waves) + lane
__global__ __launch_bounds__(64) void hm_greedy_walk_kernel(CountArgs a)
{
    const int64_t w = blockIdx.x;
    const int32_t l = a.order[w / a.k_waves];
    const int32_t c = (int32_t)(w % a.k_waves) * 64 + (int32_t)threadIdx.x;
    if (c >= a.k) return;
    const int64_t idx = (int64_t)c * a.n_lines + l;
    int32_t count = a.base[l];
    if (a.mark[idx]) {
        const int64_t b = a.cand_off[c];
        const int64_t len = a.cand_off[c + 1] - b;
        const int32_t* t = a.cand + b;
        const int32_t c0 = t[0];
        const int64_t end = a.off[l + 1];
        count = 0;
        for (int64_t p = a.off[l]; p < end; ++count) {
            int64_t step = a.lm[p];
            if (len > step && len <= end - p && a.cp[p] == c0 && hm_gr_match(a.cp, p, t, len)) step = len;
            p += step;
        }
    }
    if (a.counts) a.counts[idx] = count;
    atomicAdd(a.totals + c, (unsigned long long)(a.mult[l] * (int64_t)count));
}

}  // namespace

struct hm_greedy {
    int device = 0;
    // corpus (device)
    DevBuf<int32_t> cp, line_of, lm, base, order;
    DevBuf<int64_t> off, mult;
    int64_t n = 0, n_lines = 0;
    bool has_corpus = false;
    // vocabulary (host pool; empty strings are kept out: they never match)
    std::vector<int32_t> pool;
    std::vector<int64_t> pool_off{0};
    int32_t max_len = 0;
    // per-call workspaces (grown on demand)
    DevBuf<int32_t> cand;
    DevBuf<int64_t> cand_off;
    DevBuf<uint8_t> mark;
};

namespace {

// strings [s0, s1) of an offsets array: argument checks shared by the entry points
int hm_gr_check_strings(const char* who, const int32_t* cps, const int64_t* offsets, int64_t count)
{
    if (count < 0 || (count > 0 && (!offsets || !cps))) return hm_fail(nullptr, HM_E_ARG, std::string(who) + ": NULL pointer or negative count");
    if (count == 0) return HM_OK;
    if (offsets[0] != 0) return hm_fail(nullptr, HM_E_ARG, std::string(who) + ": offsets[0] must be 0");
    for (int64_t s = 0; s < count; ++s)
        if (offsets[s + 1] < offsets[s] || offsets[s + 1] - offsets[s] > INT32_MAX)
            return hm_fail(nullptr, HM_E_ARG, std::string(who) + ": offsets must be non-decreasing, every string shorter than 2^31");
    if (offsets[count] >= ((int64_t)1 << 31)) return hm_fail(nullptr, HM_E_ARG, std::string(who) + ": 2^31 code points or more");
    return HM_OK;
}

// lm of the whole corpus from the whole pool (hash build), then base
int hm_gr_rebuild(hm_greedy* g, hipStream_t st)
{
    if (!g->has_corpus) return HM_OK;
    const int64_t n_str = (int64_t)g->pool_off.size() - 1;
    if (g->n == 0) {
        // empty lines only: nothing to match, every count is 0
    } else if (n_str == 0) {
        std::vector<int32_t> ones((size_t)g->n, 1);
        HM_HIP0(hipMemcpyAsync(g->lm.p, ones.data(), sizeof(int32_t) * g->n, hipMemcpyHostToDevice, st));
        HM_HIP0(hipStreamSynchronize(st));
    } else {
        int64_t cap = 16;
        while (cap < 2 * n_str) cap <<= 1;
        const uint64_t mask = (uint64_t)cap - 1;
        std::vector<SetEntry> set((size_t)cap, SetEntry{0, 0, 0});
        std::vector<uint8_t> has_len((size_t)g->max_len + 1, 0);
        for (int64_t s = 0; s < n_str; ++s) {
            const int32_t* t = g->pool.data() + g->pool_off[s];
            const int32_t len = (int32_t)(g->pool_off[s + 1] - g->pool_off[s]);
            uint64_t h = HM_GR_FNV_BASIS;
            for (int32_t q = 0; q < len; ++q) h = hm_gr_step(h, t[q]);
            has_len[len] = 1;
            for (uint64_t b = hm_gr_slot(h, len, mask);; b = (b + 1) & mask) {
                SetEntry& e = set[b];
                if (e.len == 0) { e = SetEntry{h, len, (int32_t)s}; break; }
                if (e.len == len && e.h == h && std::equal(t, t + len, g->pool.data() + g->pool_off[e.str])) break;   // duplicate
            }
        }
        DevBuf<SetEntry> d_set;
        DevBuf<uint8_t> d_has;
        DevBuf<int32_t> d_pool;
        DevBuf<int64_t> d_poff;
        HM_HIP0(d_set.alloc(cap));
        HM_HIP0(d_has.alloc((int64_t)has_len.size()));
        HM_HIP0(d_pool.alloc((int64_t)g->pool.size()));
        HM_HIP0(d_poff.alloc((int64_t)g->pool_off.size()));
        HM_HIP0(hipMemcpyAsync(d_set.p, set.data(), sizeof(SetEntry) * cap, hipMemcpyHostToDevice, st));
        HM_HIP0(hipMemcpyAsync(d_has.p, has_len.data(), has_len.size(), hipMemcpyHostToDevice, st));
        if (!g->pool.empty()) HM_HIP0(hipMemcpyAsync(d_pool.p, g->pool.data(), sizeof(int32_t) * g->pool.size(), hipMemcpyHostToDevice, st));
        HM_HIP0(hipMemcpyAsync(d_poff.p, g->pool_off.data(), sizeof(int64_t) * g->pool_off.size(), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(hm_greedy_build_kernel, dim3((unsigned)((g->n + 255) / 256)), dim3(256), 0, st,
                           g->cp.p, g->line_of.p, g->off.p, g->n, d_set.p, mask, d_has.p, g->max_len, d_pool.p, d_poff.p, g->lm.p);
        HM_HIP0(hipGetLastError());
        HM_HIP0(hipStreamSynchronize(st));     // the temporaries die here
    }
    if (g->n_lines) {
        hipLaunchKernelGGL(hm_greedy_base_kernel, dim3((unsigned)((g->n_lines + 63) / 64)), dim3(64), 0, st, g->off.p, g->lm.p, g->n_lines, g->base.p);
        HM_HIP0(hipGetLastError());
    }
    HM_HIP0(hipStreamSynchronize(st));
    return HM_OK;
}

}  // namespace

extern "C" int hm_greedy_create(hm_greedy** out, int device)
{
    if (int e = hm_check_create("hm_greedy_create", out, device)) return e;
    hm_greedy* g = new hm_greedy();
    g->device = device;
    *out = g;
    return HM_OK;
}

extern "C" int hm_greedy_destroy(hm_greedy* g)
{
    if (!g) return HM_OK;
    (void)hipSetDevice(g->device);           // every entry point synchronises its stream: nothing is in flight
    delete g;
    return HM_OK;
}

extern "C" int hm_greedy_set_corpus(hm_greedy* g, const int32_t* cps, const int64_t* offsets, const int64_t* mult,
                                    int64_t n_lines, void* stream)
{
    if (!g) return hm_fail(nullptr, HM_E_ARG, "hm_greedy_set_corpus: NULL matcher");
    if (n_lines >= ((int64_t)1 << 31)) return hm_fail(nullptr, HM_E_ARG, "hm_greedy_set_corpus: 2^31 lines or more");
    if (int st = hm_gr_check_strings("hm_greedy_set_corpus", cps, offsets, n_lines)) return st;
    if (n_lines > 0 && !mult) return hm_fail(nullptr, HM_E_ARG, "hm_greedy_set_corpus: mult is NULL");
    for (int64_t l = 0; l < n_lines; ++l)
        if (mult[l] < 0) return hm_fail(nullptr, HM_E_ARG, "hm_greedy_set_corpus: negative multiplicity");
    HM_HIP0(hipSetDevice(g->device));
    hipStream_t st = (hipStream_t)stream;
    HM_HIP0(hipStreamSynchronize(st));          // earlier counts may still read the old corpus
    g->has_corpus = false;
    const int64_t n = n_lines ? offsets[n_lines] : 0;
    std::vector<int32_t> line_of((size_t)n);
    std::vector<int32_t> order((size_t)n_lines);
    for (int64_t l = 0; l < n_lines; ++l) {
        for (int64_t p = offsets[l]; p < offsets[l + 1]; ++p) line_of[(size_t)p] = (int32_t)l;
        order[(size_t)l] = (int32_t)l;
    }
    std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) {
        return offsets[x + 1] - offsets[x] > offsets[y + 1] - offsets[y];
    });
    HM_HIP0(g->cp.alloc(n));
    HM_HIP0(g->line_of.alloc(n));
    HM_HIP0(g->lm.alloc(n));
    HM_HIP0(g->off.alloc(n_lines + 1));
    HM_HIP0(g->mult.alloc(n_lines));
    HM_HIP0(g->base.alloc(n_lines));
    HM_HIP0(g->order.alloc(n_lines));
    g->n = n;
    g->n_lines = n_lines;
    if (n) {
        HM_HIP0(hipMemcpyAsync(g->cp.p, cps, sizeof(int32_t) * n, hipMemcpyHostToDevice, st));
        HM_HIP0(hipMemcpyAsync(g->line_of.p, line_of.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice, st));
    }
    if (n_lines) {
        HM_HIP0(hipMemcpyAsync(g->off.p, offsets, sizeof(int64_t) * (n_lines + 1), hipMemcpyHostToDevice, st));
        HM_HIP0(hipMemcpyAsync(g->mult.p, mult, sizeof(int64_t) * n_lines, hipMemcpyHostToDevice, st));
        HM_HIP0(hipMemcpyAsync(g->order.p, order.data(), sizeof(int32_t) * n_lines, hipMemcpyHostToDevice, st));
    }
    HM_HIP0(hipStreamSynchronize(st));          // the host staging vectors die here
    g->has_corpus = true;
    return hm_gr_rebuild(g, st);
}

extern "C" int hm_greedy_add_strings(hm_greedy* g, const int32_t* cps, const int64_t* offsets, int64_t n_strings, void* stream)
{
    if (!g) return hm_fail(nullptr, HM_E_ARG, "hm_greedy_add_strings: NULL matcher");
    if (int st = hm_gr_check_strings("hm_greedy_add_strings", cps, offsets, n_strings)) return st;
    if (n_strings == 0) return HM_OK;
    if ((int64_t)g->pool.size() + offsets[n_strings] >= ((int64_t)1 << 31) || (int64_t)g->pool_off.size() + n_strings >= ((int64_t)1 << 31))
        return hm_fail(nullptr, HM_E_ARG, "hm_greedy_add_strings: the vocabulary pool would reach 2^31 code points or strings");
    // host pool: empty strings never match (the reference would loop forever on them)
    std::vector<int64_t> fresh{0};
    const int64_t pool0 = (int64_t)g->pool.size();
    for (int64_t s = 0; s < n_strings; ++s) {
        const int64_t len = offsets[s + 1] - offsets[s];
        if (len == 0) continue;
        g->pool.insert(g->pool.end(), cps + offsets[s], cps + offsets[s + 1]);
        g->pool_off.push_back((int64_t)g->pool.size());
        fresh.push_back((int64_t)g->pool.size() - pool0);
        g->max_len = std::max<int32_t>(g->max_len, (int32_t)len);
    }
    const int64_t n_new = (int64_t)fresh.size() - 1;
    if (!g->has_corpus || g->n == 0 || n_new == 0) return HM_OK;
    HM_HIP0(hipSetDevice(g->device));
    hipStream_t st = (hipStream_t)stream;
    if (n_new > HM_GR_DIRECT_MAX) return hm_gr_rebuild(g, st);
    HM_HIP0(g->cand.grow(fresh.back()));
    HM_HIP0(g->cand_off.grow(n_new + 1));
    HM_HIP0(hipMemcpyAsync(g->cand.p, g->pool.data() + pool0, sizeof(int32_t) * fresh.back(), hipMemcpyHostToDevice, st));
    HM_HIP0(hipMemcpyAsync(g->cand_off.p, fresh.data(), sizeof(int64_t) * fresh.size(), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(hm_greedy_append_kernel, dim3((unsigned)((g->n + 255) / 256)), dim3(256), 0, st,
                       g->cp.p, g->line_of.p, g->off.p, g->n, g->cand.p, g->cand_off.p, (int32_t)n_new, g->lm.p);
    HM_HIP0(hipGetLastError());
    hipLaunchKernelGGL(hm_greedy_base_kernel, dim3((unsigned)((g->n_lines + 63) / 64)), dim3(64), 0, st, g->off.p, g->lm.p, g->n_lines, g->base.p);
    HM_HIP0(hipGetLastError());
    HM_HIP0(hipStreamSynchronize(st));          // `fresh` and the pool may move once this returns
    return HM_OK;
}

extern "C" int hm_greedy_count(hm_greedy* g, const int32_t* cps, const int64_t* offsets, int64_t k,
                               int32_t* counts_dev, int64_t* totals_dev, void* stream)
{
    if (!g) return hm_fail(nullptr, HM_E_ARG, "hm_greedy_count: NULL matcher");
    if (k >= ((int64_t)1 << 31)) return hm_fail(nullptr, HM_E_ARG, "hm_greedy_count: 2^31 candidates or more");
    if (int st = hm_gr_check_strings("hm_greedy_count", cps, offsets, k)) return st;
    if (k > 0 && !totals_dev) return hm_fail(nullptr, HM_E_ARG, "hm_greedy_count: totals_dev is NULL");
    if (!g->has_corpus) return hm_fail(nullptr, HM_E_STATE, "hm_greedy_count: hm_greedy_set_corpus first");
    if (k == 0) return HM_OK;
    HM_HIP0(hipSetDevice(g->device));
    hipStream_t st = (hipStream_t)stream;
    HM_HIP0(hipMemsetAsync(totals_dev, 0, sizeof(int64_t) * k, st));
    if (g->n_lines == 0) return HM_OK;
    HM_HIP0(g->cand.grow(offsets[k]));
    HM_HIP0(g->cand_off.grow(k + 1));
    HM_HIP0(g->mark.grow(k * g->n_lines));
    if (offsets[k]) HM_HIP0(hipMemcpyAsync(g->cand.p, cps, sizeof(int32_t) * offsets[k], hipMemcpyHostToDevice, st));
    HM_HIP0(hipMemcpyAsync(g->cand_off.p, offsets, sizeof(int64_t) * (k + 1), hipMemcpyHostToDevice, st));
    HM_HIP0(hipMemsetAsync(g->mark.p, 0, (size_t)(k * g->n_lines), st));
    CountArgs a;
    a.cp = g->cp.p; a.line_of = g->line_of.p; a.off = g->off.p; a.mult = g->mult.p; a.lm = g->lm.p; a.base = g->base.p; a.order = g->order.p;
    a.n = g->n; a.n_lines = g->n_lines;
    a.cand = g->cand.p; a.cand_off = g->cand_off.p; a.k = (int32_t)k; a.k_waves = (int32_t)((k + 63) / 64);
    a.mark = g->mark.p; a.counts = counts_dev; a.totals = reinterpret_cast<unsigned long long*>(totals_dev);
    if (g->n) {
        hipLaunchKernelGGL(hm_greedy_mark_kernel, dim3((unsigned)((g->n + 255) / 256)), dim3(256), 0, st, a);
        HM_HIP0(hipGetLastError());
    }
    const int64_t waves = g->n_lines * a.k_waves;
    if (waves > 0x7FFFFFFF) return hm_fail(nullptr, HM_E_ARG, "hm_greedy_count: lines x ceil(k / 64) must stay below 2^31");
    hipLaunchKernelGGL(hm_greedy_walk_kernel, dim3((unsigned)waves), dim3(64), 0, st, a);
    HM_HIP0(hipGetLastError());
    HM_HIP0(hipStreamSynchronize(st));          // the caller's host arrays were copied from pageable memory
    return HM_OK;
}

extern "C" int hm_greedy_longest(hm_greedy* g, int32_t* lm_dev, int32_t* base_dev, void* stream)
{
    if (!g) return hm_fail(nullptr, HM_E_ARG, "hm_greedy_longest: NULL matcher");
    if (!g->has_corpus) return hm_fail(nullptr, HM_E_STATE, "hm_greedy_longest: hm_greedy_set_corpus first");
    HM_HIP0(hipSetDevice(g->device));
    hipStream_t st = (hipStream_t)stream;
    if (lm_dev && g->n) HM_HIP0(hipMemcpyAsync(lm_dev, g->lm.p, sizeof(int32_t) * g->n, hipMemcpyDeviceToDevice, st));
    if (base_dev && g->n_lines) HM_HIP0(hipMemcpyAsync(base_dev, g->base.p, sizeof(int32_t) * g->n_lines, hipMemcpyDeviceToDevice, st));
    return HM_OK;
}
