// hm_gromov_plan.h -- host-side planning of the Gromov-delta walk (hm_gromov.hip): argument checks, the tile
// list of the upper triangle, the workspace size.  No HIP: tests/gromov_plan_driver.cpp compiles it with a host compiler
// alone; the kernels decode their tile with hm_gr_tile_of, so the function is usable on both sides.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define HM_GR_HD __host__ __device__
#else
#define HM_GR_HD
#endif

#define HM_GR_TILE 128             // edge of an output tile (i-tile x j-tile of one base point)
#define HM_GR_KCHUNK 32            // k positions staged per round
#define HM_GR_MAX_N 32768          // B = D(i,w) + D(j,w) - D(i,j) of int16 distances fits 16 unsigned bits; n^2 records never overflow
#define HM_GR_REC_BYTES 16         // one workspace record per (base, tile): {value, i, j, spare}, 32 bits each

// what the checks below return; the entry points turn them into HM_E_ARG with these words
enum HmGromovArg { HM_GR_ARG_OK = 0, HM_GR_ARG_NULL = 1, HM_GR_ARG_N = 2, HM_GR_ARG_LD = 3, HM_GR_ARG_BASES = 4 };

inline const char* hm_gr_arg_text(int what)
{
    switch (what) {
    case HM_GR_ARG_NULL: return "NULL pointer";
    case HM_GR_ARG_N: return "n must lie in 1..32768";
    case HM_GR_ARG_LD: return "ld must be at least n";
    case HM_GR_ARG_BASES: return "n_base must lie in 0..n";
    default: return "";
    }
}

// tiles along one edge and in the upper triangle (diagonal included)
HM_GR_HD inline int64_t hm_gr_edge_tiles(int64_t n) { return (n + HM_GR_TILE - 1) / HM_GR_TILE; }
HM_GR_HD inline int64_t hm_gr_tiles(int64_t n)
{
    const int64_t nt = hm_gr_edge_tiles(n);
    return nt * (nt + 1) / 2;
}
// tiles before tile row ti: rows 0 .. ti - 1 hold nt, nt - 1, ... tiles
HM_GR_HD inline int64_t hm_gr_row_start(int64_t nt, int64_t ti) { return ti * nt - ti * (ti - 1) / 2; }
// tile t of the list (row-major over the upper triangle) -> (ti, tj), ti <= tj.  A halving search over hm_gr_row_start:
// integers only, the same on host and device.
HM_GR_HD inline void hm_gr_tile_of(int64_t nt, int64_t t, int* ti_out, int* tj_out)
{
    int64_t lo = 0, hi = nt;                                   // the last row whose start is <= t
    while (hi - lo > 1) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (hm_gr_row_start(nt, mid) <= t) lo = mid;
        else hi = mid;
    }
    *ti_out = (int)lo;
    *tj_out = (int)(lo + (t - hm_gr_row_start(nt, lo)));
}

// bytes of workspace a call needs (0 for a call that launches nothing, -1 for sizes the entry points refuse)
inline int64_t hm_gr_workspace_bytes(int64_t n, int64_t n_base)
{
    if (n < 1 || n > HM_GR_MAX_N || n_base < 0 || n_base > n) return -1;
    return n_base * hm_gr_tiles(n) * HM_GR_REC_BYTES;
}

// the checks every entry point makes before it touches the device
inline int hm_gr_check_args(const void* d, int64_t n, int64_t ld, const void* base, int64_t n_base, const void* value_out,
                            const void* witness_out, const void* workspace)
{
    if (!d || !base || !value_out || !witness_out || !workspace) return HM_GR_ARG_NULL;
    if (n < 1 || n > HM_GR_MAX_N) return HM_GR_ARG_N;
    if (ld < n) return HM_GR_ARG_LD;
    if (n_base < 0 || n_base > n) return HM_GR_ARG_BASES;
    return HM_GR_ARG_OK;
}
