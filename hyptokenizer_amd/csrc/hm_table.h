// hm_table.h -- what the text-side translation units (hm_greedy, hm_pairfreq, hm_ngram, hm_classmin) share: an owning
// device buffer, the argument checks of the create functions, and the 64-bit counting table of the two counters (one
// probe on the device, one compaction kernel, one recount-on-overflow loop on the host).  DESIGN.md section 5.9.
//
// The table: open addressing over 64-bit keys, linear probing, ~0 = free slot.  A key is claimed by a CAS into a free
// slot; `distinct` counts the claimed slots and the load is capped at one half.  Crossing the cap, or a probe sequence
// longer than max_probe, raises `*overflow`: from then on the table takes no new key, its contents are void, and the host
// counts again into a table four times larger.  A table with at least twice as many slots as there are insertions
// cannot overflow, so the loop ends.  Payload columns (counts, first positions) belong to the caller.
#pragma once
#include "hm_common.h"

#include <memory>

// ---- owning buffer: device memory, or pinned host memory (PINNED) ----
template <class T, bool PINNED = false>
struct DevBuf {
    T* p = nullptr;
    int64_t cap = 0;                                        // elements asked for (at least one is allocated)

    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept
    {
        if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
        return *this;
    }
    ~DevBuf() { release(); }

    void release()
    {
        if (p) (void)(PINNED ? hipHostFree(p) : hipFree(p));
        p = nullptr;
        cap = 0;
    }
    hipError_t alloc(int64_t n)                             // exactly n elements; what the buffer held is gone
    {
        release();
        const size_t bytes = sizeof(T) * (size_t)std::max<int64_t>(n, 1);
        const hipError_t st = PINNED ? hipHostMalloc(reinterpret_cast<void**>(&p), bytes, hipHostMallocDefault)
                                     : hipMalloc(reinterpret_cast<void**>(&p), bytes);
        if (st != hipSuccess) p = nullptr;
        else cap = n;
        return st;
    }
    hipError_t grow(int64_t need)                           // room for `need` elements; contents are NOT kept
    {
        return need <= cap ? hipSuccess : alloc(std::max<int64_t>(need, 2 * cap));
    }
};

// ---- argument checks and capacity arithmetic of the create functions ----
inline int hm_check_device(const char* who, int device)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return hm_fail(nullptr, HM_E_ARG, std::string(who) + ": no HIP device available (there is no CPU fallback)");
    if (device < 0 || device >= ndev) return hm_fail(nullptr, HM_E_ARG, std::string(who) + ": bad device index");
    return HM_OK;
}

// what a create function checks first: the out pointer (cleared), the device, a counter's initial table capacity
template <class H>
int hm_check_create(const char* who, H** out, int device, int64_t initial_capacity = 0)
{
    if (!out) return hm_fail(nullptr, HM_E_ARG, std::string(who) + ": out is NULL");
    *out = nullptr;
    if (int e = hm_check_device(who, device)) return e;
    if (initial_capacity < 0 || initial_capacity > ((int64_t)1 << 40))
        return hm_fail(nullptr, HM_E_ARG, std::string(who) + ": initial_capacity must lie in [0, 2^40]");
    return HM_OK;
}

inline int64_t hm_pow2_at_least(int64_t x, int64_t floor)   // floor: a power of two
{
    int64_t c = floor;
    while (c < x) c <<= 1;
    return c;
}

// ---- the counting table ----
constexpr unsigned long long HM_TABLE_EMPTY = ~0ull;
constexpr uint64_t HM_TABLE_PROBES = 4096;                  // a table below the bound that needs more is counted again, larger

__host__ __device__ __forceinline__ uint64_t hm_mix64(uint64_t k)
{
    k ^= k >> 31;
    k *= 0x7fb5d329728ea185ull;
    k ^= k >> 27;
    k *= 0x81dadef4bc2dd44dull;
    k ^= k >> 33;
    return k;
}

struct HmTable {
    unsigned long long* keys;       // [mask + 1], HM_TABLE_EMPTY when free
    unsigned long long* distinct;   // claimed slots
    int* overflow;                  // raised when more than `limit` slots were claimed or a probe sequence ran out
    uint64_t mask;
    unsigned long long limit;       // (mask + 1) / 2
    uint64_t max_probe;
};

// `capped`: give up after HM_TABLE_PROBES probes (a table that may still be counted again); otherwise probe the whole table
inline HmTable hm_table_view(unsigned long long* keys, int64_t cap, unsigned long long* distinct, int* overflow, bool capped)
{
    HmTable t;
    t.keys = keys; t.distinct = distinct; t.overflow = overflow;
    t.mask = (uint64_t)cap - 1;
    t.limit = (unsigned long long)(cap / 2);
    t.max_probe = capped ? std::min<uint64_t>(HM_TABLE_PROBES, (uint64_t)cap) : (uint64_t)cap;
    return t;
}

__device__ __forceinline__ bool hm_table_overflowed(const HmTable& t)
{
    return __hip_atomic_load(t.overflow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
}

// Slot of the caller's key, probing from h0: `key` is what a free slot is claimed with, same(cur) says whether an occupied
// slot holds it (the n-gram table stores references and compares what they point to).  *fresh (optional) is set when this
// call claimed the slot.  -1, with the overflow flag raised, when the table takes no (further) key.
template <class Same>
__device__ __forceinline__ int64_t hm_table_claim(const HmTable& t, uint64_t h0, unsigned long long key, Same same, bool* fresh = nullptr)
{
    uint64_t slot = h0 & t.mask;
    for (uint64_t probe = 0; probe < t.max_probe; ++probe, slot = (slot + 1) & t.mask) {
        unsigned long long cur = __hip_atomic_load(&t.keys[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == HM_TABLE_EMPTY) {
            if (hm_table_overflowed(t)) return -1;
            cur = atomicCAS(&t.keys[slot], HM_TABLE_EMPTY, key);
            if (cur == HM_TABLE_EMPTY) {
                if (fresh) *fresh = true;
                if (atomicAdd(t.distinct, 1ull) >= t.limit) { atomicOr(t.overflow, 1); return -1; }
                return (int64_t)slot;
            }
        }
        if (same(cur)) return (int64_t)slot;
    }
    atomicOr(t.overflow, 1);
    return -1;
}

// occupied slots and their COLS payload columns, compacted in any order; *n_out counts them (it may pass out_cap)
template <int COLS>
struct HmColumns {
    const unsigned long long* in[COLS];
    unsigned long long* out[COLS];
};

template <int COLS>
__global__ __launch_bounds__(256) void hm_table_compact_kernel(const unsigned long long* __restrict__ keys, HmColumns<COLS> c, uint64_t cap,
                                                               unsigned long long* __restrict__ n_out,
                                                               unsigned long long* __restrict__ keys_out, uint64_t out_cap)
{
    const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= cap) return;
    const unsigned long long key = keys[s];
    if (key == HM_TABLE_EMPTY) return;
    const unsigned long long k = atomicAdd(n_out, 1ull);
    if (k >= out_cap) return;
    keys_out[k] = key;
#pragma unroll
    for (int q = 0; q < COLS; ++q) c.out[q][k] = c.in[q][s];
}

inline unsigned hm_blocks(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

// one column of a table: `cap` words with every byte `fill` (0xFF: free keys, no position yet; 0: counts); the memory is
// kept when the size does not change
inline int hm_column_reset(DevBuf<unsigned long long>& col, int64_t cap, int fill, hipStream_t st)
{
    if (col.cap != cap) HM_HIP0(col.alloc(cap));
    HM_HIP0(hipMemsetAsync(col.p, fill, sizeof(unsigned long long) * (size_t)cap, st));
    return HM_OK;
}

// The recount loop.  count(cap, &overflow) sizes or resets the caller's tables for `cap` slots, runs the count and reports
// the overflow flag it read back; while it is set the count is repeated with four times the slots, `bound` at most (the
// size that cannot overflow).
template <class Count>
int hm_count_growing(const char* who, int64_t cap, int64_t bound, int64_t& recounts, Count count)
{
    for (;;) {
        bool overflow = false;
        if (int e = count(cap, &overflow)) return e;
        if (!overflow) return HM_OK;
        if (cap >= bound)
            return hm_fail(nullptr, HM_E_STATE, std::string(who) + ": overflow of a table sized for every occurrence (internal error)");
        cap = std::min(bound, 4 * cap);
        ++recounts;
    }
}
