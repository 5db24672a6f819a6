// hm_tokstats.hip -- the integer counts behind the corpus metrics of a tokenizer, over a token stream that is already on
// the device (scripts/compare_tokenizers.py: benchmark_hyperbolic_tokenizer :146-221, evaluate_linguistic_quality
// :224-289, evaluate_compression_efficiency :292-329; scripts/benchmark_efficiency.py:58-94 covers the same ground).
//
// Input: the output of hm_tokenize_batch -- tok[], offsets[n + 1], len[n]; line l holds tok[offsets[l] .. offsets[l] +
// len[l]), the slots behind it up to offsets[l + 1] are never read as tokens.  What the metrics need of a token are four
// flags and its length, one 32-bit word per symbol (attr[], layout in include/hypmerge.h); a negative symbol -(2 + cp)
// is one character, whose flags come from a bitmap of re's \w over the code space.
//
// Work is parallel over token POSITIONS: a tile is HM_TS_TILE consecutive positions, four per lane (one 16-byte load),
// and a block walks a contiguous range of tiles with its counts in registers.  The first / last flags of the neighbouring
// positions come from the neighbouring lanes (the two lanes at a wave's ends look their neighbour up themselves).  A lane
// finds the line of its first position by bisection once per block and by galloping from the previous tile's line after
// that, so one long line is shared by as many lanes as it has positions / 4.  Five 64-bit sums per lane -> wave (shuffles)
// -> block (LDS) -> one atomic add per counter and block.  Integer sums: the result does not depend on the launch geometry.
// The optional per-line counts are flushed whenever a lane's line changes (a wave that lies inside ONE line adds once).
#include "hm_common.h"

namespace {

constexpr int HM_TS_THREADS = 256;
constexpr int HM_TS_PER_LANE = 4;
constexpr int HM_TS_TILE = HM_TS_THREADS * HM_TS_PER_LANE;    // HM_TOKSTATS_TILE of the header
constexpr int HM_TS_BLOCKS_PER_CU = 4;
constexpr uint32_t HM_TS_NONWORD = HM_TOKSTATS_NONWORD, HM_TS_MORPH = HM_TOKSTATS_MORPHEME, HM_TS_FIRST = HM_TOKSTATS_FIRST_WORD,
                   HM_TS_LAST = HM_TOKSTATS_LAST_WORD;
static_assert(HM_TS_TILE == HM_TOKSTATS_TILE, "tile size of the header");

struct TsArgs {
    const int32_t* tok;
    const int64_t* off;           // [n_lines + 1]
    const int32_t* len;           // [n_lines]
    int64_t n_lines;
    int64_t n;                    // positions
    const uint32_t* attr;         // [n_sym]
    int64_t n_sym;
    const uint32_t* wordmap;      // 0x110000 bits
    unsigned long long* totals;   // [HM_TOKSTATS_COUNTERS]
    unsigned long long* lines;    // [n_lines][HM_TOKSTATS_COUNTERS] or nullptr
    int64_t n_tiles, tiles_per_block;
    int vec;                      // tok is 16-byte aligned
};

// attribute word of one symbol; anything that is neither a table symbol nor a code point counts as an empty token
__device__ __forceinline__ uint32_t hm_ts_attr(const TsArgs& a, int32_t s)
{
    if (s >= 0) return (int64_t)s < a.n_sym ? a.attr[s] : 0u;
    const uint32_t cp = (uint32_t)(-(int64_t)s - 2);
    if (s == -1 || cp >= 0x110000u) return 0u;
    const uint32_t w = (a.wordmap[cp >> 5] >> (cp & 31)) & 1u;
    return (1u << HM_TOKSTATS_LEN_SHIFT) | (w ? (HM_TS_FIRST | HM_TS_LAST) : HM_TS_NONWORD);
}

// line l with off[l] <= q < off[l + 1] (empty lines skipped), searched upwards from `lo` (off[lo] <= q)
__device__ __forceinline__ int64_t hm_ts_line(const int64_t* __restrict__ off, int64_t n_lines, int64_t lo, int64_t q)
{
    int64_t step = 1, hi = lo + 1;
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

struct Counts {
    unsigned long long c[HM_TOKSTATS_COUNTERS];
    __device__ __forceinline__ void clear()
    {
#pragma unroll
        for (int k = 0; k < HM_TOKSTATS_COUNTERS; ++k) c[k] = 0;
    }
    __device__ __forceinline__ bool any() const { return c[0] != 0; }       // every counted token adds to c[0]
};

__device__ __forceinline__ unsigned long long hm_ts_wave_sum(unsigned long long v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ void hm_ts_flush_line(unsigned long long* lines, int64_t line, const Counts& c)
{
    unsigned long long* row = lines + line * HM_TOKSTATS_COUNTERS;
#pragma unroll
    for (int k = 0; k < HM_TOKSTATS_COUNTERS; ++k)
        if (c.c[k]) atomicAdd(&row[k], c.c[k]);
}

__global__ __launch_bounds__(HM_TS_THREADS) void hm_tokstats_kernel(TsArgs a)
{
    __shared__ unsigned long long s_part[HM_TS_THREADS / 64][HM_TOKSTATS_COUNTERS];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t t0 = (int64_t)blockIdx.x * a.tiles_per_block;
    const int64_t t1 = min(t0 + a.tiles_per_block, a.n_tiles);
    Counts tot, cur;              // the block's share, and the share of the line this lane is in (per-line output only)
    tot.clear();
    cur.clear();
    int64_t line = -1, line_begin = 0, line_next = 0, line_len = 0;   // the lane's current line: [line_begin, line_next), len tokens
    int64_t cur_line = -1;

    for (int64_t t = t0; t < t1; ++t) {
        const int64_t q0 = t * HM_TS_TILE + (int64_t)threadIdx.x * HM_TS_PER_LANE;
        int32_t s[HM_TS_PER_LANE];
        if (a.vec && q0 + HM_TS_PER_LANE <= a.n) {
            const int4 v = *reinterpret_cast<const int4*>(a.tok + q0);
            s[0] = v.x; s[1] = v.y; s[2] = v.z; s[3] = v.w;
        } else {
#pragma unroll
            for (int k = 0; k < HM_TS_PER_LANE; ++k) s[k] = q0 + k < a.n ? a.tok[q0 + k] : -1;
        }
        uint32_t at[HM_TS_PER_LANE];
#pragma unroll
        for (int k = 0; k < HM_TS_PER_LANE; ++k) at[k] = hm_ts_attr(a, s[k]);
        // the neighbours of this lane's run: position q0 - 1 (lane - 1's last) and q0 + 4 (lane + 1's first).  All 64 lanes
        // shuffle; the lanes at the wave's ends read their neighbour from memory.  Neither value is used unless that
        // position is a token of the same line (checked below), so what a slot behind a line's end holds never counts.
        uint32_t before = __shfl_up(at[HM_TS_PER_LANE - 1], 1, 64);
        uint32_t after = __shfl_down(at[0], 1, 64);
        if (lane == 0) before = q0 > 0 && q0 - 1 < a.n ? hm_ts_attr(a, a.tok[q0 - 1]) : 0u;
        if (lane == 63) after = q0 + HM_TS_PER_LANE < a.n ? hm_ts_attr(a, a.tok[q0 + HM_TS_PER_LANE]) : 0u;

#pragma unroll
        for (int k = 0; k < HM_TS_PER_LANE; ++k) {
            const int64_t q = q0 + k;
            if (q >= a.n) break;
            if (line < 0 || q >= line_next) {
                int64_t lo = 0;
                if (line >= 0) lo = min(line + 1, a.n_lines - 1);      // (the clamp matters only for offsets that end below n)
                else {                                      // first position of this lane: bisection over all lines
                    int64_t hi = a.n_lines;
                    while (hi - lo > 1) {
                        const int64_t mid = lo + (hi - lo) / 2;
                        if (a.off[mid] <= q) lo = mid;
                        else hi = mid;
                    }
                }
                line = hm_ts_line(a.off, a.n_lines, lo, q);
                line_begin = a.off[line];
                line_next = a.off[line + 1];
                line_len = min((int64_t)max(a.len[line], 0), line_next - line_begin);   // a tokenised line is never longer than its input
            }
            const int64_t i = q - line_begin;
            if (i < 0 || i >= line_len) continue;           // a slot behind the line's tokens (or inconsistent offsets)
            const uint32_t me = at[k];
            const uint32_t prev = k == 0 ? before : at[k > 0 ? k - 1 : 0];
            const uint32_t next = k == HM_TS_PER_LANE - 1 ? after : at[k < HM_TS_PER_LANE - 1 ? k + 1 : 0];
            const bool sub = (i > 0 && (prev & HM_TS_LAST) && (me & HM_TS_FIRST)) ||
                             (i < line_len - 1 && (me & HM_TS_LAST) && (next & HM_TS_FIRST));
            if (a.lines && line != cur_line) {
                if (cur.any()) {
                    hm_ts_flush_line(a.lines, cur_line, cur);
#pragma unroll
                    for (int c = 0; c < HM_TOKSTATS_COUNTERS; ++c) tot.c[c] += cur.c[c];
                }
                cur.clear();
                cur_line = line;
            }
            Counts& c = a.lines ? cur : tot;
            c.c[0] += 1;
            c.c[1] += me >> HM_TOKSTATS_LEN_SHIFT;
            c.c[2] += (me & HM_TS_NONWORD) ? 1 : 0;
            c.c[3] += (me & HM_TS_MORPH) ? 1 : 0;
            c.c[4] += sub ? 1 : 0;
        }
        if (a.lines) {
            // end of the tile: what the lane holds for its line goes out.  A wave whose lanes all sit in one line (a long
            // line) adds once per counter instead of 64 times
            const int64_t first = __shfl(cur_line, 0, 64);
            const bool uniform = __all(cur_line == first) && first >= 0;
#pragma unroll
            for (int k = 0; k < HM_TOKSTATS_COUNTERS; ++k) tot.c[k] += cur.c[k];
            if (uniform) {
#pragma unroll
                for (int k = 0; k < HM_TOKSTATS_COUNTERS; ++k) {
                    const unsigned long long v = hm_ts_wave_sum(cur.c[k]);
                    if (lane == 0 && v) atomicAdd(&a.lines[first * HM_TOKSTATS_COUNTERS + k], v);
                }
            } else if (cur.any()) {
                hm_ts_flush_line(a.lines, cur_line, cur);
            }
            cur.clear();
        }
    }

#pragma unroll
    for (int k = 0; k < HM_TOKSTATS_COUNTERS; ++k) {
        const unsigned long long v = hm_ts_wave_sum(tot.c[k]);
        if (lane == 0) s_part[wv][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < HM_TOKSTATS_COUNTERS) {
        unsigned long long v = 0;
#pragma unroll
        for (int w = 0; w < HM_TS_THREADS / 64; ++w) v += s_part[w][threadIdx.x];
        if (v) atomicAdd(&a.totals[threadIdx.x], v);
    }
}

}  // namespace

extern "C" int hm_tokstats(const int32_t* tok_dev, const int64_t* offsets_dev, const int32_t* len_dev, int64_t n_lines,
                           int64_t n_positions, const uint32_t* attr_dev, int64_t n_sym, const uint32_t* wordmap_dev,
                           uint64_t* totals_dev, uint64_t* line_counts_dev, int64_t max_blocks, void* stream)
{
    if (n_lines < 0 || n_positions < 0 || n_sym < 0 || max_blocks < 0)
        return hm_fail(nullptr, HM_E_ARG, "hm_tokstats: negative size");
    if (!totals_dev || !wordmap_dev || (n_sym > 0 && !attr_dev) || (n_lines > 0 && (!offsets_dev || !len_dev)) ||
        (n_positions > 0 && !tok_dev))
        return hm_fail(nullptr, HM_E_ARG, "hm_tokstats: NULL pointer");
    if (n_positions > 0 && n_lines == 0) return hm_fail(nullptr, HM_E_ARG, "hm_tokstats: positions without lines");
    if (n_sym > ((int64_t)1 << 21)) return hm_fail(nullptr, HM_E_ARG, "hm_tokstats: at most 2^21 symbols");
    if (n_positions >= ((int64_t)1 << 40)) return hm_fail(nullptr, HM_E_ARG, "hm_tokstats: 2^40 positions per call");
    hipStream_t st = (hipStream_t)stream;
    HM_HIP0(hipMemsetAsync(totals_dev, 0, sizeof(uint64_t) * HM_TOKSTATS_COUNTERS, st));
    if (line_counts_dev && n_lines)
        HM_HIP0(hipMemsetAsync(line_counts_dev, 0, sizeof(uint64_t) * HM_TOKSTATS_COUNTERS * (size_t)n_lines, st));
    if (n_positions == 0) return HM_OK;
    TsArgs a;
    a.tok = tok_dev; a.off = offsets_dev; a.len = len_dev; a.n_lines = n_lines; a.n = n_positions;
    a.attr = attr_dev; a.n_sym = n_sym; a.wordmap = wordmap_dev;
    a.totals = reinterpret_cast<unsigned long long*>(totals_dev);
    a.lines = reinterpret_cast<unsigned long long*>(line_counts_dev);
    a.n_tiles = (n_positions + HM_TS_TILE - 1) / HM_TS_TILE;
    a.vec = ((uintptr_t)tok_dev & 15) == 0;
    int64_t blocks = max_blocks;
    if (blocks == 0) {
        int dev = 0, cus = 0;
        HM_HIP0(hipGetDevice(&dev));
        HM_HIP0(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
        blocks = (int64_t)std::max(cus, 1) * HM_TS_BLOCKS_PER_CU;
    }
    blocks = std::min(blocks, a.n_tiles);
    a.tiles_per_block = (a.n_tiles + blocks - 1) / blocks;
    blocks = (a.n_tiles + a.tiles_per_block - 1) / a.tiles_per_block;
    hipLaunchKernelGGL(hm_tokstats_kernel, dim3((unsigned)blocks), dim3(HM_TS_THREADS), 0, st, a);
    HM_HIP0(hipGetLastError());
    return HM_OK;
}
