// hm_csr.h -- a graph on the device as a CSR (row_ptr int64[n + 1], col int32[nnz]), its host-side check and its upload:
// what hm_graph.hip and hm_negsample.hip share.  Their kernels index with values the check has seen.
#pragma once
#include "hm_table.h"

struct HmCsr {
    int64_t n = 0, nnz = 0;                                 // n == 0: no graph set
    DevBuf<int64_t> row;
    DevBuf<int32_t> col;
};

// The caller's host CSR: n in [1, max_nodes] (`limit_text` is that interval in the message), row_ptr from 0 without a
// decrease, nnz below 2^31, col in [0, n) and, with `sorted_unique`, every row ascending without repeats.  One walk in row
// order, so the first offending entry decides the message.
inline int hm_csr_check(const char* who, const int64_t* row_ptr, const int32_t* col, int64_t n, int64_t max_nodes, const char* limit_text,
                        bool sorted_unique)
{
    const std::string w(who);
    if (!row_ptr || n < 1 || n > max_nodes) return hm_fail(nullptr, HM_E_ARG, w + ": n must lie in " + limit_text);
    if (row_ptr[0] != 0) return hm_fail(nullptr, HM_E_ARG, w + ": row_ptr[0] must be 0");
    for (int64_t v = 0; v < n; ++v)
        if (row_ptr[v + 1] < row_ptr[v] || row_ptr[v + 1] >= ((int64_t)1 << 31))
            return hm_fail(nullptr, HM_E_ARG, w + ": row_ptr must not decrease and nnz must stay below 2^31");
    if (row_ptr[n] > 0 && !col) return hm_fail(nullptr, HM_E_ARG, w + ": col is NULL");
    for (int64_t v = 0; v < n; ++v)
        for (int64_t e = row_ptr[v]; e < row_ptr[v + 1]; ++e) {
            if (col[e] < 0 || (int64_t)col[e] >= n) return hm_fail(nullptr, HM_E_ARG, w + ": column index out of range");
            if (sorted_unique && e > row_ptr[v] && col[e] <= col[e - 1])
                return hm_fail(nullptr, HM_E_ARG, w + ": a row must be sorted and free of repeats");
        }
    return HM_OK;
}

// Upload a checked CSR.  n goes to 0 first, so a failed upload leaves "no graph set".
inline int hm_csr_set(HmCsr& g, int device, const int64_t* row_ptr, const int32_t* col, int64_t n, hipStream_t s)
{
    const int64_t nnz = row_ptr[n];
    HM_HIP0(hipSetDevice(device));
    g.n = 0;
    HM_HIP0(g.row.alloc(n + 1));
    HM_HIP0(g.col.alloc(nnz));
    HM_HIP0(hipMemcpyAsync(g.row.p, row_ptr, sizeof(int64_t) * (size_t)(n + 1), hipMemcpyHostToDevice, s));
    if (nnz > 0) HM_HIP0(hipMemcpyAsync(g.col.p, col, sizeof(int32_t) * (size_t)nnz, hipMemcpyHostToDevice, s));
    HM_HIP0(hipStreamSynchronize(s));                       // pageable caller memory
    g.n = n;
    g.nnz = nnz;
    return HM_OK;
}
