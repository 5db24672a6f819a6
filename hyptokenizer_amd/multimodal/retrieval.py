"""Hyperbolic retrieval metrics and exact k-NN as fused HIP kernels.

``compute_recall_at_k`` has the reference's name, arguments and result (``scripts/train_retrieval.py:176-229``), which fills
a B x B matrix by B^2 calls of ``distance(...).item()`` and runs ``torch.topk`` per row and per column.  Here one walk over
the pair tiles counts, for every matched pair, how many candidates come before it (``retrieval_ranks``); the matrix is never
stored.  ``hyperbolic_knn`` is the per-query search the reference's FAISS branch asked for (``index.search(q, k)``,
``tokenizer/hyperbolic_merge.py:217``, ``tokenizer/fast_hyperbolic_merge.py:302-304``), exact and in the project's canonical
fp32 distance.

Conventions of ``contrastive_loss.py``: tensors must live on a HIP device (there is no CPU fallback), rows are taken as
fp32, ``sign_convention=`` and its default are those of ``embedding.lorentz_model``.  Nothing here is differentiable:
results are detached.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import torch

from .. import _lib
from ..embedding import lorentz_model as _lm
from ..engine import MAX_TABLE_ROWS, _f, _ptr, _require_cuda, _rows2d, _stream_of
from .contrastive_loss import MAX_BATCH, MAX_D1, _check_pair

MAX_K = 128


def _ld(t: torch.Tensor) -> int:
    return t.stride(0) if t.shape[0] > 1 else t.shape[1]


def _check_batch(text: torch.Tensor, image: torch.Tensor, what: str) -> None:
    _check_pair(text, image, what)
    if not 1 <= text.shape[0] <= MAX_BATCH:
        raise ValueError(f"{what}: batch size must lie in [1, {MAX_BATCH}], got {text.shape[0]}")


def _same_device(a: torch.Tensor, b: torch.Tensor, what: str) -> None:
    if a.device != b.device:
        raise ValueError(f"{what}: both operands must live on the same device, got {a.device} and {b.device}")


def set_rank_layout(layout: int) -> None:
    """Test / tuning hook (results never depend on it): the tile layout of the rank kernel from now on, process-wide.
    0 = the default, 1 = A and B rows in LDS, 2 = A rows in registers and B rows as 16-byte LDS broadcasts."""
    _lib.check(_lib.load().hm_debug_retrieval_layout(int(layout)))


def _ranks(text: torch.Tensor, image: torch.Tensor, sign_mode: int) -> torch.Tensor:
    _require_cuda(text, image)
    _same_device(text, image, "retrieval_ranks")
    L = _lib.load()
    zt, zi = _rows2d(text), _rows2d(image)
    n, d1 = zt.shape
    out = torch.empty((2, n), dtype=torch.int32, device=zt.device)
    with torch.cuda.device(zt.device):
        _lib.check(L.hm_retrieval_ranks(_ptr(zt), _ptr(zi), n, _ld(zt), _ld(zi), d1, int(sign_mode), _ptr(out[0]), _ptr(out[1]),
                                        _stream_of(zt)))
    return out


def retrieval_ranks(text_embeddings: torch.Tensor, image_embeddings: torch.Tensor, *,
                    sign_convention: Optional[str] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(rank_t2i, rank_i2t)``, two int32 device tensors of length B.  With ``D[i, j] = distance(text[i], image[j])``
    (``c = 1``, the bits ``batch_distance`` returns)::

        rank_t2i[i] = #{ j : D[i,j] <  D[i,i] }  +  #{ j < i : D[i,j] == D[i,i] }
        rank_i2t[j] = #{ i : D[i,j] <  D[j,j] }  +  #{ i < j : D[i,j] == D[j,j] }

    Pair i counts as retrieved at k iff its rank is ``< k``.  NaN sorts as torch sorts it: greater than every number, equal
    to NaN."""
    _check_batch(text_embeddings, image_embeddings, "retrieval_ranks")
    out = _ranks(text_embeddings, image_embeddings, _lm._sign(sign_convention))
    return out[0], out[1]


def compute_recall_at_k(text_embeddings: torch.Tensor, image_embeddings: torch.Tensor, k_values: Sequence[int] = (1, 5, 10), *,
                        sign_convention: Optional[str] = None) -> Dict[str, float]:
    """Reference ``scripts/train_retrieval.py:176-229``: ``r@{k}_text2image`` for every k, then ``r@{k}_image2text`` for
    every k, each ``correct / batch_size`` as a Python float.  ``k > B`` (where the reference's ``torch.topk`` raises) is a
    ``ValueError``."""
    _check_batch(text_embeddings, image_embeddings, "compute_recall_at_k")
    n = text_embeddings.shape[0]
    ks: List[int] = [int(k) for k in k_values]
    for k in ks:
        if k > n:
            raise ValueError(f"compute_recall_at_k: k = {k} exceeds the batch size B = {n}")
        if k < 0:
            raise ValueError(f"compute_recall_at_k: k must not be negative, got {k}")
    ranks = _ranks(text_embeddings, image_embeddings, _lm._sign(sign_convention))
    if ks:
        kk = torch.tensor(ks, dtype=torch.int32, device=ranks.device)
        correct = (ranks[:, None, :] < kk[None, :, None]).sum(-1).cpu().tolist()        # [direction][k]
    else:
        correct = [[], []]
    results: Dict[str, float] = {}
    for row, name in ((0, "text2image"), (1, "image2text")):
        for k, c in zip(ks, correct[row]):
            results[f"r@{k}_{name}"] = int(c) / n
    return results


def hyperbolic_knn(queries: torch.Tensor, keys: torch.Tensor, k: int, c: float = 1.0, *, sign_convention: Optional[str] = None,
                   exclude_self: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """The k nearest keys of every query: ``(distances [Q, k] fp32, indices [Q, k] int64)``, each row ordered by
    ``(distance, key index)`` ascending -- the k smallest entries of that row of ``batch_distance(queries, keys, c)`` with
    the same bits.  NaN distances are never selected; a row with fewer than k selectable keys is padded with index -1 and
    distance ``+inf``.  ``exclude_self=True`` skips key i for query i (a table against itself)."""
    if queries.dim() != 2 or keys.dim() != 2 or queries.shape[1] != keys.shape[1]:
        raise ValueError(f"hyperbolic_knn: expected queries (Q, d+1) and keys (N, d+1), got {tuple(queries.shape)} and {tuple(keys.shape)}")
    nq, d1 = queries.shape
    nk = keys.shape[0]
    if not 2 <= d1 <= MAX_D1:
        raise ValueError(f"hyperbolic_knn: d+1 must lie in [2, {MAX_D1}], got {d1}")
    if not (1 <= nq <= MAX_TABLE_ROWS and 1 <= nk <= MAX_TABLE_ROWS):
        raise ValueError(f"hyperbolic_knn: Q and N must lie in [1, {MAX_TABLE_ROWS}], got {nq} and {nk}")
    k = int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError(f"hyperbolic_knn: k must lie in [1, {MAX_K}], got {k}")
    if k > nk:
        raise ValueError(f"hyperbolic_knn: k = {k} exceeds the number of keys N = {nk}")
    if not c > 0:
        raise ValueError(f"hyperbolic_knn: c must be positive, got {c}")
    _require_cuda(queries, keys)
    _same_device(queries, keys, "hyperbolic_knn")
    L = _lib.load()
    qq, kk = _rows2d(queries), _rows2d(keys)
    dist = torch.empty((nq, k), dtype=torch.float32, device=qq.device)
    idx = torch.empty((nq, k), dtype=torch.int32, device=qq.device)
    with torch.cuda.device(qq.device):
        _lib.check(L.hm_knn(_ptr(qq), nq, _ptr(kk), nk, _ld(qq), _ld(kk), d1, _f(c), _lm._sign(sign_convention), k,
                            1 if exclude_self else 0, _ptr(dist), _ptr(idx), _stream_of(qq)))
    return dist, idx.long()
