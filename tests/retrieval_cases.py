"""CPU truth and input builders shared by the retrieval tests (test_retrieval_golden.py without a GPU,
test_gpu_retrieval.py with one) and by the golden generator.

The truth works on a distance matrix ``D`` (numpy fp32), in the tests always the unchanged oracle's
``oracle.hm_oracle.batch_distance``: the project's canonical fp32 distance.

  ranks_truth(D)  ->  (rank_t2i, rank_i2t), with NaN ordered as torch.sort orders it (greater than every number, equal
                      to NaN):
                        rank_t2i[i] = #{ j : D[i,j] <  D[i,i] } + #{ j < i : D[i,j] == D[i,i] }
                        rank_i2t[j] = #{ i : D[i,j] <  D[j,j] } + #{ i < j : D[i,j] == D[j,j] }
  recall_truth(D, k_values)  ->  the reference's dictionary: pair i is retrieved at k iff its rank is < k
  knn_truth(D, k, exclude_self)  ->  (distances [Q, k] fp32, indices [Q, k] int64): np.lexsort((index, distance)) per row
                      with the NaNs dropped, padded with (+inf, -1)
"""
from __future__ import annotations

import numpy as np

SIGN_MODE = {"reference": 0, "lorentz": 1}


def _less_equal(row: np.ndarray, pivot) -> tuple:
    """Element-wise (row < pivot, row == pivot) under torch.sort's order of NaN."""
    rn = np.isnan(row)
    if np.isnan(pivot):
        return ~rn, rn
    with np.errstate(invalid="ignore"):
        return (row < pivot) & ~rn, (row == pivot) & ~rn


def _ranks_rows(D: np.ndarray) -> np.ndarray:
    n = D.shape[0]
    out = np.empty(n, np.int32)
    for i in range(n):
        lt, eq = _less_equal(D[i], D[i, i])
        out[i] = int(lt.sum()) + int(eq[:i].sum())
    return out


def ranks_truth(D: np.ndarray):
    D = np.asarray(D, np.float32)
    assert D.ndim == 2 and D.shape[0] == D.shape[1]
    return _ranks_rows(D), _ranks_rows(np.ascontiguousarray(D.T))


def recall_from_ranks(rank_t2i, rank_i2t, k_values) -> dict:
    n = len(rank_t2i)
    out = {}
    for name, rk in (("text2image", rank_t2i), ("image2text", rank_i2t)):
        for k in k_values:
            out[f"r@{k}_{name}"] = int((np.asarray(rk) < k).sum()) / n
    return out


def recall_truth(D: np.ndarray, k_values) -> dict:
    return recall_from_ranks(*ranks_truth(D), k_values)


def knn_truth(D: np.ndarray, k: int, exclude_self: bool = False):
    D = np.asarray(D, np.float32)
    nq, nk = D.shape
    dist = np.full((nq, k), np.inf, np.float32)
    idx = np.full((nq, k), -1, np.int64)
    for i in range(nq):
        keep = ~np.isnan(D[i])
        if exclude_self and i < nk:
            keep[i] = False
        cand = np.nonzero(keep)[0]
        order = cand[np.lexsort((cand, D[i, cand]))][:k]
        dist[i, :len(order)] = D[i, order]
        idx[i, :len(order)] = order
    return dist, idx


# ---- input builders ----------------------------------------------------------------------------------------------------
def project(x: np.ndarray) -> np.ndarray:
    """Rows onto the unit hyperboloid: x0 = sqrt(1 + |x_spatial|^2), in fp32."""
    x = np.array(x, np.float32)
    x[:, 0] = np.sqrt(np.float32(1.0) + (x[:, 1:] * x[:, 1:]).sum(-1, dtype=np.float32))
    return x


def points(rs: np.random.RandomState, n: int, d: int, scale: float) -> np.ndarray:
    return project(rs.randn(n, d + 1).astype(np.float32) * np.float32(scale))


def pairs(rs: np.random.RandomState, n: int, d: int, scale: float, noise: float):
    """(a, b) with b = project(a + noise): matched pairs, the shape of a retrieval validation set."""
    a = points(rs, n, d, scale)
    b = project(a + rs.randn(n, d + 1).astype(np.float32) * np.float32(noise))
    return a, b


def special_pairs(rs: np.random.RandomState, n: int, d: int, scale: float = 1.0, noise: float = 0.7):
    """Pairs with duplicated rows in both operands (exact ties), one row of NaN and rows off the hyperboloid (u < 1 under
    "lorentz": clamped to distance 0, massive ties), as far as n allows."""
    a, b = pairs(rs, n, d, scale, noise)
    if n >= 8:
        a[5] = a[2]; b[5] = b[2]                       # duplicates in both operands
        a[n - 1] = a[0]                                # a duplicate in one operand only
        b[3, 0] = np.nan                               # a key row of NaN ...
        a[6, -1] = np.nan                              # ... and a query row of NaN
        off = max(2, n // 8)
        a[n // 2:n // 2 + off] = rs.randn(off, d + 1).astype(np.float32) * np.float32(0.2)      # time-like part too small
        b[n // 2 + 1:n // 2 + 1 + off] = rs.randn(off, d + 1).astype(np.float32) * np.float32(0.2)
    elif n >= 2:
        b[1] = b[0]
    return a, b
