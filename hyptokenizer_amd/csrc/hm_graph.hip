// hm_graph.hip -- shortest-path lengths and connected components of an undirected graph (hierarchy-distortion
// evaluation).  Engine-free like the text kernels; buffers are hm_table.h's DevBuf.
//
// The graph is a symmetric CSR (row_ptr int64[n + 1], col int32[nnz]) checked on the host when it is set: every kernel
// below indexes with values that check has seen.
//
// Bit-parallel multi-source BFS.  Every source of a pass owns one bit; a node carries W 64-bit words in each of three
// arrays `seen`, `frontier`, `next`, node-major: word w of node v is at [v * W + w].  Thread t of a launch owns word
// t = v * W + w, so the lanes of a wave run across the words of a node and a neighbour's row is one coalesced read.
//   pull(L):    next[v] = (OR over u in adj(v) of frontier[u]) & ~seen[v];  seen[v] |= next[v]
//               no atomics on the bit arrays: word (v, w) has one writer, and `frontier` is only read.
//   second(L):  pairs -- every unresolved (source bit, dst) tests its bit in next[dst], writes L, counts `remaining` down;
//               rows  -- every (column node, word), in that order, writes L to the rows of the bits set in next[node].
//               Its thread 0 also keeps the books: stop when pull(L) set no bit, clear the flag of pull(L + 1).
// Both kernels return at once when `stop != 0 || remaining == 0`.  The host enqueues levels in chunks and reads the
// control block between chunks; after at most n levels the frontier is empty.
//
// Pass size: 3 arrays x n nodes x W words x 8 bytes <= HM_GRAPH_BITS_BUDGET (1 GiB), W >= 1; a call with more than
// 64 * W distinct sources runs ceil(S / (64 * W)) passes.  Knob "graph_pass_words" caps W (tests force several passes).
//
// Components: min-label propagation with hooking and pointer jumping.  labels[v] starts at v, only decreases, and is
// always a node of v's component, so concurrent atomicMin updates can only change how fast the fixed point is reached,
// not what it is: every node carries the smallest index of its component.
#include "hm_csr.h"

#define HM_GRAPH_MAX_NODES ((int64_t)1 << 24)
#define HM_GRAPH_BITS_BUDGET ((int64_t)1 << 30)
#define HM_GRAPH_THREADS 256

struct GraphCtl {
    uint32_t remaining;            // pairs mode: unresolved pairs of the pass; rows mode: 1
    uint32_t stop;                 // the frontier ran empty (BFS) / an iteration changed nothing (components)
    uint32_t grew[2];              // by level parity: pull(L) set a bit / prop(i) lowered a label
    uint32_t levels;               // levels (iterations) that did work
    uint32_t overflow;             // rows mode: a level above 32767 reached a column node
    unsigned long long count;      // components: roots
};

struct hm_graph {
    int device = 0;
    HmCsr csr;
    int64_t pass_words_cap = 0;                  // knob graph_pass_words (0: the memory bound alone)
    int64_t chunk_levels = 16;                   // knob graph_chunk_levels
    DevBuf<unsigned long long> d_bits;           // seen | frontier | next, n * W words each
    DevBuf<int32_t> d_idx;                       // staging: seeds, sorted pairs, column nodes
    DevBuf<GraphCtl> d_ctl;
    DevBuf<GraphCtl, true> h_ctl;                // [0] what goes up, [1] what comes back
    int64_t last_levels = 0, last_launches = 0, last_passes = 0, last_words = 0;
};

static std::map<std::string, double> g_graph_knobs;

bool hm_graph_owns_knob(const char* name)
{
    const std::string k = name ? name : "";
    return k == "graph_pass_words" || k == "graph_chunk_levels";
}

// HM_OK: a graph knob, taken; HM_E_ARG: a graph knob, bad value; 1: not a graph knob
int hm_graph_default_knob(const char* name, double v, int clear)
{
    const std::string k = name ? name : "";
    if (clear) { if (k.empty()) g_graph_knobs.clear(); else g_graph_knobs.erase(k); return HM_OK; }
    if (!hm_graph_owns_knob(name)) return 1;
    if (!(v >= 0 && v <= 65536) || (k == "graph_chunk_levels" && v < 1)) return HM_E_ARG;
    g_graph_knobs[k] = v;
    return HM_OK;
}

namespace {

__device__ __forceinline__ bool hm_graph_idle(const GraphCtl* ctl)
{
    return __hip_atomic_load(&ctl->stop, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0
        || __hip_atomic_load(&ctl->remaining, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0;
}

// raise a flag many waves raise: read first, the atomic only when it is still down
__device__ __forceinline__ void hm_graph_raise(uint32_t* flag)
{
    if (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) atomicOr(flag, 1u);
}

// the books of level (iteration) L, kept by one thread of the second kernel: pull(L) / prop(L) has finished
__device__ __forceinline__ void hm_graph_books(GraphCtl* ctl, int64_t L, bool first)
{
    if (!first && ctl->grew[L & 1] == 0) __hip_atomic_store(&ctl->stop, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else ctl->levels += 1;
    ctl->grew[(L + 1) & 1] = 0;
}

__global__ __launch_bounds__(HM_GRAPH_THREADS) void hm_graph_seed_kernel(const int32_t* __restrict__ seeds, int64_t count, int W,
                                                                         unsigned long long* __restrict__ seen,
                                                                         unsigned long long* __restrict__ frontier)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const int64_t at = (int64_t)seeds[i] * W + (i >> 6);
    const unsigned long long bit = 1ull << (i & 63);
    atomicOr(&seen[at], bit);              // a node may be seeded twice (distance_rows with a repeated source)
    atomicOr(&frontier[at], bit);
}

__global__ __launch_bounds__(HM_GRAPH_THREADS) void hm_graph_pull_kernel(const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                                         int64_t total, int W, const unsigned long long* __restrict__ frontier,
                                                                         unsigned long long* __restrict__ seen,
                                                                         unsigned long long* __restrict__ next, GraphCtl* ctl, int64_t L)
{
    if (hm_graph_idle(ctl)) return;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const int64_t v = t / W;
    const int64_t w = t - v * W;
    const int64_t e0 = row_ptr[v], e1 = row_ptr[v + 1];
    unsigned long long acc = 0;
    int64_t e = e0;
    for (; e + 4 <= e1; e += 4) {
        const unsigned long long a0 = frontier[(int64_t)col[e] * W + w], a1 = frontier[(int64_t)col[e + 1] * W + w];
        const unsigned long long a2 = frontier[(int64_t)col[e + 2] * W + w], a3 = frontier[(int64_t)col[e + 3] * W + w];
        acc |= (a0 | a1) | (a2 | a3);
    }
    for (; e < e1; ++e) acc |= frontier[(int64_t)col[e] * W + w];
    const unsigned long long s = seen[t];
    const unsigned long long nx = acc & ~s;
    next[t] = nx;
    if (nx) {
        seen[t] = s | nx;
        hm_graph_raise(&ctl->grew[L & 1]);
    }
}

// pairs mode: entry i of the pass is (slot bit, dst node, index of the caller's pair), sorted by slot
__global__ __launch_bounds__(HM_GRAPH_THREADS) void hm_graph_pairs_kernel(const int32_t* __restrict__ slot, const int32_t* __restrict__ dst,
                                                                          const int32_t* __restrict__ pair, int64_t count, int W,
                                                                          const unsigned long long* __restrict__ cur, int32_t* __restrict__ out,
                                                                          GraphCtl* ctl, int64_t L)
{
    if (hm_graph_idle(ctl)) return;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) hm_graph_books(ctl, L, L == 0);
    bool hit = false;
    if (i < count) {
        const int32_t p = pair[i];
        if (out[p] < 0) {
            const int32_t b = slot[i];
            hit = (cur[(int64_t)dst[i] * W + (b >> 6)] >> (b & 63)) & 1ull;
            if (hit) out[p] = (int32_t)L;
        }
    }
    const unsigned long long m = __ballot(hit);
    if (m != 0 && (threadIdx.x & 63) == (unsigned)(__ffsll((long long)m) - 1)) atomicSub(&ctl->remaining, (uint32_t)__popcll(m));
}

// rows mode: thread t = m * W + w reads word w of column node m -- the node-major order of the bit arrays, so a wave reads
// consecutive words (one row when cols is NULL or sorted) -- and writes level L to out[(row0 + 64 w + b) * ld + m] for every
// bit b set.  The read happens for all M * W words at every level, the stores once per (source, column) over the whole
// BFS, so the order favours the read; the int16 stores of a wave scatter over rows.
__global__ __launch_bounds__(HM_GRAPH_THREADS) void hm_graph_rows_kernel(const int32_t* __restrict__ cols, int64_t M, int W,
                                                                         const unsigned long long* __restrict__ cur, int16_t* __restrict__ out,
                                                                         int64_t row0, int64_t ld, GraphCtl* ctl, int64_t L)
{
    if (hm_graph_idle(ctl)) return;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t == 0) hm_graph_books(ctl, L, L == 0);
    if (t >= M * W) return;
    const int64_t m = t / W;
    const int64_t w = t - m * W;
    const int64_t node = cols ? (int64_t)cols[m] : m;
    unsigned long long bits = cur[node * W + w];
    if (bits == 0) return;
    if (L > 32767) { hm_graph_raise(&ctl->overflow); return; }
    while (bits) {
        const int b = __ffsll((long long)bits) - 1;
        bits &= bits - 1;
        out[(row0 + 64 * w + b) * ld + m] = (int16_t)L;
    }
}

__global__ __launch_bounds__(HM_GRAPH_THREADS) void hm_graph_fill16_kernel(int16_t* __restrict__ out, int64_t rows, int64_t M, int64_t ld)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= rows * M) return;
    const int64_t r = t / M;
    out[r * ld + (t - r * M)] = (int16_t)-1;
}

__global__ __launch_bounds__(HM_GRAPH_THREADS) void hm_graph_iota_kernel(int32_t* __restrict__ labels, int64_t n)
{
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v < n) labels[v] = (int32_t)v;
}

__device__ __forceinline__ int32_t hm_graph_label(const int32_t* labels, int64_t v)
{
    return __hip_atomic_load(&labels[v], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// labels[v] and the label of v's current root both go down to the smallest label among v and its neighbours
__global__ __launch_bounds__(HM_GRAPH_THREADS) void hm_graph_prop_kernel(const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                                         int64_t n, int32_t* labels, GraphCtl* ctl, int64_t it)
{
    if (hm_graph_idle(ctl)) return;
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    const int32_t own = hm_graph_label(labels, v);
    int32_t m = own;
    for (int64_t e = row_ptr[v]; e < row_ptr[v + 1]; ++e) m = min(m, hm_graph_label(labels, col[e]));
    if (m < own) {
        atomicMin(&labels[v], m);
        atomicMin(&labels[own], m);
        hm_graph_raise(&ctl->grew[it & 1]);
    }
}

// pointer jumping: labels[v] <- the root of its chain (labels[x] <= x, so the walk ends)
__global__ __launch_bounds__(HM_GRAPH_THREADS) void hm_graph_jump_kernel(int64_t n, int32_t* labels, GraphCtl* ctl, int64_t it)
{
    if (hm_graph_idle(ctl)) return;
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v == 0) hm_graph_books(ctl, it, false);
    if (v >= n) return;
    int32_t l = hm_graph_label(labels, v);
    for (;;) {
        const int32_t up = hm_graph_label(labels, l);
        if (up >= l) break;
        l = up;
    }
    atomicMin(&labels[v], l);
}

__global__ __launch_bounds__(HM_GRAPH_THREADS) void hm_graph_roots_kernel(int64_t n, const int32_t* __restrict__ labels, GraphCtl* ctl)
{
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool root = v < n && labels[v] == (int32_t)v;
    const unsigned long long m = __ballot(root);
    if (m != 0 && (threadIdx.x & 63) == (unsigned)(__ffsll((long long)m) - 1)) atomicAdd(&ctl->count, (unsigned long long)__popcll(m));
}

int hm_graph_check(hm_graph* g, const char* who, bool need_csr)
{
    if (!g) return hm_fail(nullptr, HM_E_ARG, std::string(who) + ": NULL handle");
    if (need_csr && g->csr.n <= 0) return hm_fail(nullptr, HM_E_STATE, std::string(who) + ": no graph set (hm_graph_set_csr)");
    return HM_OK;
}

// words per node of a pass over `sources` distinct sources: as many as they need, within the memory bound and the knob
int64_t hm_graph_words(const hm_graph* g, int64_t sources)
{
    int64_t W = std::max<int64_t>(1, (sources + 63) / 64);
    W = std::min(W, std::max<int64_t>(1, HM_GRAPH_BITS_BUDGET / (24 * g->csr.n)));
    if (g->pass_words_cap > 0) W = std::min(W, g->pass_words_cap);
    return W;
}

int hm_graph_put_ctl(hm_graph* g, uint32_t remaining, hipStream_t s)
{
    GraphCtl& c = g->h_ctl.p[0];
    memset(&c, 0, sizeof(c));
    c.remaining = remaining;
    HM_HIP0(hipMemcpyAsync(g->d_ctl.p, &c, sizeof(GraphCtl), hipMemcpyHostToDevice, s));
    return HM_OK;
}

int hm_graph_get_ctl(hm_graph* g, hipStream_t s)
{
    HM_HIP0(hipMemcpyAsync(&g->h_ctl.p[1], g->d_ctl.p, sizeof(GraphCtl), hipMemcpyDeviceToHost, s));
    HM_HIP0(hipStreamSynchronize(s));
    return HM_OK;
}

// One pass of the BFS from the `count` seeds at seeds_dev (bit i = seed i), W words per node.  second(cur, L) enqueues
// the second kernel of level L on the array `cur`.  The control block must already be on the device.
template <class Second>
int hm_graph_bfs(hm_graph* g, const int32_t* seeds_dev, int64_t count, int W, hipStream_t s, Second second)
{
    const int64_t total = g->csr.n * W;
    unsigned long long* seen = g->d_bits.p;
    unsigned long long* fr = seen + total;
    unsigned long long* nx = fr + total;
    HM_HIP0(hipMemsetAsync(seen, 0, sizeof(unsigned long long) * (size_t)(2 * total), s));
    hipLaunchKernelGGL(hm_graph_seed_kernel, dim3(hm_blocks(count, HM_GRAPH_THREADS)), dim3(HM_GRAPH_THREADS), 0, s, seeds_dev, count, W, seen, fr);
    second(fr, (int64_t)0);
    g->last_launches += 2;
    for (int64_t L = 1; L <= g->csr.n;) {
        const int64_t end = std::min(g->csr.n, L + g->chunk_levels - 1);
        for (; L <= end; ++L) {
            hipLaunchKernelGGL(hm_graph_pull_kernel, dim3(hm_blocks(total, HM_GRAPH_THREADS)), dim3(HM_GRAPH_THREADS), 0, s, g->csr.row.p,
                               g->csr.col.p, total, W, fr, seen, nx, g->d_ctl.p, L);
            second(nx, L);
            std::swap(fr, nx);
            g->last_launches += 2;
        }
        HM_HIP0(hipGetLastError());
        if (int rc = hm_graph_get_ctl(g, s)) return rc;
        if (g->h_ctl.p[1].stop != 0 || g->h_ctl.p[1].remaining == 0) break;
    }
    g->last_levels = std::max<int64_t>(g->last_levels, g->h_ctl.p[1].levels);
    g->last_passes += 1;
    return HM_OK;
}

void hm_graph_begin(hm_graph* g, int64_t W)
{
    g->last_levels = g->last_launches = g->last_passes = 0;
    g->last_words = W;
}

}  // namespace

extern "C" int hm_graph_create(hm_graph** out, int device)
{
    if (int rc = hm_check_create("hm_graph_create", out, device)) return rc;
    HM_HIP0(hipSetDevice(device));
    std::unique_ptr<hm_graph> g(new hm_graph());
    g->device = device;
    if (g->d_ctl.alloc(1) != hipSuccess || g->h_ctl.alloc(2) != hipSuccess)
        return hm_fail(nullptr, HM_E_NOMEM, "hm_graph_create: allocation failed");
    auto k = g_graph_knobs.find("graph_pass_words");
    if (k != g_graph_knobs.end()) g->pass_words_cap = (int64_t)k->second;
    k = g_graph_knobs.find("graph_chunk_levels");
    if (k != g_graph_knobs.end()) g->chunk_levels = (int64_t)k->second;
    *out = g.release();
    return HM_OK;
}

extern "C" int hm_graph_destroy(hm_graph* g)
{
    if (!g) return HM_OK;
    (void)hipSetDevice(g->device);          // every entry point synchronises its stream: nothing is in flight
    delete g;
    return HM_OK;
}

extern "C" int hm_graph_set_csr(hm_graph* g, const int64_t* row_ptr, const int32_t* col, int64_t n, void* stream)
{
    if (int rc = hm_graph_check(g, "hm_graph_set_csr", false)) return rc;
    if (int rc = hm_csr_check("hm_graph_set_csr", row_ptr, col, n, HM_GRAPH_MAX_NODES, "[1, 2^24]", false)) return rc;
    return hm_csr_set(g->csr, g->device, row_ptr, col, n, (hipStream_t)stream);
}

extern "C" int hm_graph_components(hm_graph* g, int32_t* labels_dev, int64_t* n_components, void* stream)
{
    if (int rc = hm_graph_check(g, "hm_graph_components", true)) return rc;
    if (!labels_dev) return hm_fail(nullptr, HM_E_ARG, "hm_graph_components: labels_dev is NULL");
    HM_HIP0(hipSetDevice(g->device));
    hipStream_t s = (hipStream_t)stream;
    hm_graph_begin(g, 0);
    const dim3 grid(hm_blocks(g->csr.n, HM_GRAPH_THREADS)), block(HM_GRAPH_THREADS);
    if (int rc = hm_graph_put_ctl(g, 1, s)) return rc;
    hipLaunchKernelGGL(hm_graph_iota_kernel, grid, block, 0, s, labels_dev, g->csr.n);
    g->last_launches += 1;
    // an iteration that changes nothing ends the loop; every other one lowers a label, so n + 1 iterations bound it
    for (int64_t it = 0; it <= g->csr.n;) {
        const int64_t end = std::min(g->csr.n, it + 3);
        for (; it <= end; ++it) {
            hipLaunchKernelGGL(hm_graph_prop_kernel, grid, block, 0, s, g->csr.row.p, g->csr.col.p, g->csr.n, labels_dev, g->d_ctl.p, it);
            hipLaunchKernelGGL(hm_graph_jump_kernel, grid, block, 0, s, g->csr.n, labels_dev, g->d_ctl.p, it);
            g->last_launches += 2;
        }
        HM_HIP0(hipGetLastError());
        if (int rc = hm_graph_get_ctl(g, s)) return rc;
        if (g->h_ctl.p[1].stop != 0) break;
    }
    if (g->h_ctl.p[1].stop == 0) return hm_fail(nullptr, HM_E_STATE, "hm_graph_components: no fixed point (internal error)");
    hipLaunchKernelGGL(hm_graph_roots_kernel, grid, block, 0, s, g->csr.n, labels_dev, g->d_ctl.p);
    g->last_launches += 1;
    HM_HIP0(hipGetLastError());
    if (int rc = hm_graph_get_ctl(g, s)) return rc;
    g->last_levels = g->h_ctl.p[1].levels;
    g->last_passes = 1;
    if (n_components) *n_components = (int64_t)g->h_ctl.p[1].count;
    return HM_OK;
}

extern "C" int hm_graph_pair_lengths(hm_graph* g, const int32_t* src, const int32_t* dst, int64_t n_pairs, int32_t* out_dev, void* stream)
{
    if (int rc = hm_graph_check(g, "hm_graph_pair_lengths", true)) return rc;
    if (n_pairs < 0 || n_pairs >= ((int64_t)1 << 31) || (n_pairs > 0 && (!src || !dst || !out_dev)))
        return hm_fail(nullptr, HM_E_ARG, "hm_graph_pair_lengths: bad arguments");
    for (int64_t p = 0; p < n_pairs; ++p)
        if (src[p] < 0 || src[p] >= g->csr.n || dst[p] < 0 || dst[p] >= g->csr.n)
            return hm_fail(nullptr, HM_E_ARG, "hm_graph_pair_lengths: node index out of range");
    hm_graph_begin(g, 0);
    if (n_pairs == 0) return HM_OK;
    HM_HIP0(hipSetDevice(g->device));
    hipStream_t s = (hipStream_t)stream;
    // the distinct sources in ascending order: source k owns bit k % (64 W) of pass k / (64 W)
    std::vector<int32_t> distinct(src, src + n_pairs);
    std::sort(distinct.begin(), distinct.end());
    distinct.erase(std::unique(distinct.begin(), distinct.end()), distinct.end());
    const int64_t S = (int64_t)distinct.size();
    const int64_t W = hm_graph_words(g, S), per_pass = 64 * W;
    g->last_words = W;
    std::vector<int64_t> order(n_pairs), slot_of(n_pairs);
    for (int64_t p = 0; p < n_pairs; ++p) {
        slot_of[p] = std::lower_bound(distinct.begin(), distinct.end(), src[p]) - distinct.begin();
        order[p] = p;
    }
    std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return slot_of[a] < slot_of[b]; });
    // staging: [0, S) seeds, then per sorted pair its bit within the pass, its dst and the caller's index
    std::vector<int32_t> stage((size_t)(S + 3 * n_pairs));
    std::copy(distinct.begin(), distinct.end(), stage.begin());
    int32_t* st_slot = stage.data() + S;
    int32_t* st_dst = st_slot + n_pairs;
    int32_t* st_pair = st_dst + n_pairs;
    for (int64_t i = 0; i < n_pairs; ++i) {
        const int64_t p = order[i];
        st_slot[i] = (int32_t)(slot_of[p] % per_pass);
        st_dst[i] = dst[p];
        st_pair[i] = (int32_t)p;
    }
    HM_HIP0(g->d_idx.grow((int64_t)stage.size()));
    if (g->d_bits.cap < 3 * g->csr.n * W) HM_HIP0(g->d_bits.alloc(3 * g->csr.n * W));      // exactly the bound, never grow()'s doubling
    HM_HIP0(hipMemcpyAsync(g->d_idx.p, stage.data(), sizeof(int32_t) * stage.size(), hipMemcpyHostToDevice, s));
    HM_HIP0(hipMemsetAsync(out_dev, 0xff, sizeof(int32_t) * (size_t)n_pairs, s));
    const int32_t* d_slot = g->d_idx.p + S;
    const int32_t* d_dst = d_slot + n_pairs;
    const int32_t* d_pair = d_dst + n_pairs;
    int64_t lo = 0;
    for (int64_t base = 0; base < S; base += per_pass) {
        const int64_t count = std::min(per_pass, S - base);
        int64_t hi = lo;
        while (hi < n_pairs && slot_of[order[hi]] < base + count) ++hi;
        const int64_t np = hi - lo;
        if (int rc = hm_graph_put_ctl(g, (uint32_t)np, s)) return rc;
        const int rc = hm_graph_bfs(g, g->d_idx.p + base, count, (int)W, s, [&](const unsigned long long* cur, int64_t L) {
            hipLaunchKernelGGL(hm_graph_pairs_kernel, dim3(hm_blocks(np, HM_GRAPH_THREADS)), dim3(HM_GRAPH_THREADS), 0, s, d_slot + lo, d_dst + lo,
                               d_pair + lo, np, (int)W, cur, out_dev, g->d_ctl.p, L);
        });
        if (rc) return rc;
        lo = hi;
    }
    return HM_OK;
}

extern "C" int hm_graph_distance_rows(hm_graph* g, const int32_t* src, int64_t n_src, const int32_t* cols, int64_t n_cols, int16_t* out_dev,
                                      int64_t ld, void* stream)
{
    if (int rc = hm_graph_check(g, "hm_graph_distance_rows", true)) return rc;
    const int64_t M = cols ? n_cols : g->csr.n;
    if (n_src < 0 || n_src >= ((int64_t)1 << 31) || M < 0 || (n_src > 0 && !src) || ld < M || (n_src > 0 && M > 0 && !out_dev))
        return hm_fail(nullptr, HM_E_ARG, "hm_graph_distance_rows: bad arguments");
    for (int64_t k = 0; k < n_src; ++k)
        if (src[k] < 0 || src[k] >= g->csr.n) return hm_fail(nullptr, HM_E_ARG, "hm_graph_distance_rows: source index out of range");
    for (int64_t m = 0; cols && m < M; ++m)
        if (cols[m] < 0 || cols[m] >= g->csr.n) return hm_fail(nullptr, HM_E_ARG, "hm_graph_distance_rows: column index out of range");
    hm_graph_begin(g, 0);
    if (n_src == 0 || M == 0) return HM_OK;
    HM_HIP0(hipSetDevice(g->device));
    hipStream_t s = (hipStream_t)stream;
    const int64_t W = hm_graph_words(g, n_src), per_pass = 64 * W;
    g->last_words = W;
    HM_HIP0(g->d_idx.grow(n_src + (cols ? M : 0)));
    if (g->d_bits.cap < 3 * g->csr.n * W) HM_HIP0(g->d_bits.alloc(3 * g->csr.n * W));      // exactly the bound, never grow()'s doubling
    HM_HIP0(hipMemcpyAsync(g->d_idx.p, src, sizeof(int32_t) * (size_t)n_src, hipMemcpyHostToDevice, s));
    if (cols) HM_HIP0(hipMemcpyAsync(g->d_idx.p + n_src, cols, sizeof(int32_t) * (size_t)M, hipMemcpyHostToDevice, s));
    const int32_t* d_cols = cols ? g->d_idx.p + n_src : nullptr;
    hipLaunchKernelGGL(hm_graph_fill16_kernel, dim3(hm_blocks(n_src * M, HM_GRAPH_THREADS)), dim3(HM_GRAPH_THREADS), 0, s, out_dev, n_src, M, ld);
    g->last_launches += 1;
    for (int64_t base = 0; base < n_src; base += per_pass) {
        const int64_t count = std::min(per_pass, n_src - base);
        if (int rc = hm_graph_put_ctl(g, 1, s)) return rc;
        const int rc = hm_graph_bfs(g, g->d_idx.p + base, count, (int)W, s, [&](const unsigned long long* cur, int64_t L) {
            hipLaunchKernelGGL(hm_graph_rows_kernel, dim3(hm_blocks(M * W, HM_GRAPH_THREADS)), dim3(HM_GRAPH_THREADS), 0, s, d_cols, M, (int)W, cur,
                               out_dev, base, ld, g->d_ctl.p, L);
        });
        if (rc) return rc;
        if (g->h_ctl.p[1].overflow != 0)
            return hm_fail(nullptr, HM_E_CAPACITY, "hm_graph_distance_rows: a path longer than 32767 edges does not fit int16");
    }
    return HM_OK;
}

extern "C" int hm_graph_last_stats(const hm_graph* g, int64_t* levels, int64_t* launches, int64_t* passes, int64_t* words)
{
    if (!g) return hm_fail(nullptr, HM_E_ARG, "hm_graph_last_stats: NULL handle");
    if (levels) *levels = g->last_levels;
    if (launches) *launches = g->last_launches;
    if (passes) *passes = g->last_passes;
    if (words) *words = g->last_words;
    return HM_OK;
}
