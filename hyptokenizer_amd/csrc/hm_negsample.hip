// hm_negsample.hip -- reproducible negative sampling for graph embedding: for every (anchor, positive) pair
// K node indices drawn uniformly from [0, V), never the anchor and never a neighbour of the anchor.
//
// The graph is a symmetric CSR whose rows are sorted and free of repeats (checked on the host when it is set), so
// adjacency is a binary search in the anchor's row.  Randomness is Philox4x32-10 (Salmon et al., SC 2011): key = the 64-bit
// seed, counter = (sample b, slot k, attempt t, step), candidate = (uint64(r) * V) >> 32 from the first output word r.  A
// slot is a pure function of (seed, step, b, k, anchor): no state, no dependence on the launch geometry.  A rejected
// candidate is redrawn with the next t; after max_tries rejections the slot is -1, the loss kernels' mask.
#include "hm_csr.h"

#define HM_NS_THREADS 256
#define HM_NS_MAX_NODES (((int64_t)1 << 31) - 1)

struct hm_negsample {
    int device = 0;
    HmCsr csr;
};

namespace {

__device__ __forceinline__ uint32_t hm_ns_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1)
{
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c0;
}

// thread (b, j): column j of out row b.  j < 2 copies the pair, j >= 2 draws slot k = j - 2
__global__ __launch_bounds__(HM_NS_THREADS) void hm_ns_kernel(const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col, int64_t V,
                                                              const int64_t* __restrict__ pairs, int64_t B, int64_t K, uint32_t k0, uint32_t k1,
                                                              uint32_t step, int max_tries, int64_t* __restrict__ out)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t W = 2 + K;
    if (t >= B * W) return;
    const int64_t b = t / W, j = t - b * W;
    if (j < 2) { out[t] = pairs[2 * b + j]; return; }
    const int64_t anchor = pairs[2 * b];
    int64_t res = -1;
    if (anchor >= 0 && anchor < V) {
        const int64_t e0 = row_ptr[anchor], e1 = row_ptr[anchor + 1];
        for (int a = 0; a < max_tries; ++a) {
            const uint32_t r = hm_ns_philox((uint32_t)b, (uint32_t)(j - 2), (uint32_t)a, step, k0, k1);
            const int64_t cand = (int64_t)(((uint64_t)r * (uint64_t)V) >> 32);
            if (cand == anchor) continue;
            int64_t lo = e0, hi = e1;                         // first entry of the row that is >= cand
            while (lo < hi) {
                const int64_t mid = lo + ((hi - lo) >> 1);
                if ((int64_t)col[mid] < cand) lo = mid + 1;
                else hi = mid;
            }
            if (lo < e1 && (int64_t)col[lo] == cand) continue;
            res = cand;
            break;
        }
    }
    out[t] = res;
}

}  // namespace

extern "C" int hm_negsample_create(hm_negsample** out, int device)
{
    if (int rc = hm_check_create("hm_negsample_create", out, device)) return rc;
    std::unique_ptr<hm_negsample> g(new hm_negsample());
    g->device = device;
    *out = g.release();
    return HM_OK;
}

extern "C" int hm_negsample_destroy(hm_negsample* g)
{
    if (!g) return HM_OK;
    (void)hipSetDevice(g->device);
    delete g;
    return HM_OK;
}

// The host-side checks of hm_negsample_set_csr, apart from the handle: what the kernel's indexing relies on.
extern "C" int hm_negsample_check_csr(const int64_t* row_ptr, const int32_t* col, int64_t n)
{
    return hm_csr_check("hm_negsample_set_csr", row_ptr, col, n, HM_NS_MAX_NODES, "[1, 2^31)", true);
}

extern "C" int hm_negsample_set_csr(hm_negsample* g, const int64_t* row_ptr, const int32_t* col, int64_t n, void* stream)
{
    if (!g) return hm_fail(nullptr, HM_E_ARG, "hm_negsample_set_csr: NULL handle");
    if (int rc = hm_negsample_check_csr(row_ptr, col, n)) return rc;
    return hm_csr_set(g->csr, g->device, row_ptr, col, n, (hipStream_t)stream);
}

extern "C" int hm_negsample_sample(hm_negsample* g, const int64_t* pairs_dev, int64_t n_pairs, int64_t k, uint64_t seed, int64_t step,
                                   int max_tries, int64_t* out_dev, void* stream)
{
    if (!g) return hm_fail(nullptr, HM_E_ARG, "hm_negsample_sample: NULL handle");
    if (n_pairs < 0 || n_pairs > ((int64_t)1 << 31) || k < 0 || k > ((int64_t)1 << 20) || step < 0 || step >= ((int64_t)1 << 32) ||
        max_tries < 1 || max_tries > 65536 || (n_pairs + 1) * (k + 2) > ((int64_t)1 << 38) || (n_pairs > 0 && (!pairs_dev || !out_dev)))
        return hm_fail(nullptr, HM_E_ARG, "hm_negsample_sample: bad arguments");
    if (g->csr.n <= 0) return hm_fail(nullptr, HM_E_STATE, "hm_negsample_sample: no graph set (hm_negsample_set_csr)");
    if (n_pairs == 0) return HM_OK;
    HM_HIP0(hipSetDevice(g->device));
    const int64_t total = n_pairs * (2 + k);
    hipLaunchKernelGGL(hm_ns_kernel, dim3(hm_blocks(total, HM_NS_THREADS)), dim3(HM_NS_THREADS), 0, (hipStream_t)stream, g->csr.row.p, g->csr.col.p,
                       g->csr.n, pairs_dev, n_pairs, k, (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)step, max_tries, out_dev);
    HM_HIP0(hipGetLastError());
    return HM_OK;
}
