"""Gromov delta-hyperbolicity of a graph metric or of a table's distances -- "is this data hyperbolic at all, and which
curvature fits it" -- as one fused HIP walk over the (max, min) semiring (``hm_gromov_delta_*``).

For a base point ``w`` the Gromov product is ``(i|j)_w = (d(i,w) + d(j,w) - d(i,j)) / 2`` and

    delta_w = max_{i,j,k} [ min((i|k)_w, (k|j)_w) - (i|j)_w ]

The maximum of ``delta_w`` over all ``w`` is the four-point delta; a tree has ``delta = 0``.  ``delta_rel = 2 delta / diam``
compares data sets (Khrulkov et al., "Hyperbolic Image Embeddings", CVPR 2020).  Only the upper triangle of the distance matrix
is read: ``D(i,j) = dist[min(i,j), max(i,j)]``, the diagonal as it is given.

* int16 distances (a graph metric, ``GraphPaths.distance_rows``): the kernel works on ``B = 2 (i|j)_w``, an integer, and
  returns the exact integer ``2 delta_w``.  Precondition: ``0 <= dist <= 32767`` and the triangle inequality (a connected
  sample: ``-1``, "no path", is not a distance).
* float32 distances (``lorentz_model.batch_distance``): ``A = 0.5f * ((D(i,w) + D(j,w)) - D(i,j)) + 0.0f`` in exactly this
  order, ``delta_w = max_{i<=j} fl(max_k min(A(i,k), A(k,j)) - A(i,j))``: the bits of a float32 restatement in numpy.
  Precondition: every entry is finite.

The witness of a base is ``(i, j, k)``: among the maximising pairs the smallest ``i``, then the smallest ``j >= i``, then the
smallest ``k`` that attains the inner maximum.  The cost is O(n^3) per base point; no ``[n, n]`` product matrix and no
``[chunk, n, n]`` temporary exists.  There is no CPU fallback: off a HIP device the functions raise ``HypMergeUnavailable``.
Nothing here is differentiable.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple, Union

import numpy as np
import torch

from .. import _lib
from ..engine import _ptr, _require_cuda, _stream_of
from ..graph import select_nodes
from ..graph_paths import GraphPaths
from . import lorentz_model

MAX_POINTS = 32768
#: workspace of one kernel call; a call with more bases than fit is split (the results do not depend on the split)
_WORKSPACE_BUDGET = 256 << 20


@dataclass
class GromovDelta:
    """What ``gromov_delta`` returns."""
    delta: float                        # max over the evaluated bases; for int16 input the kernel's integer divided by 2
    per_base: torch.Tensor              # the kernel's raw values, on the device: int32 2 delta_w (int16 input) or float32 delta_w
    witness: Tuple[int, int, int, int]  # (x, y, z, w): the maximiser (i, j, k) of the maximising base w (the first such base)
    diameter: float                     # the largest entry of the upper triangle
    delta_rel: float                    # 2 delta / diameter; nan for diameter 0
    n: int
    base_positions: Optional[np.ndarray] = None   # int32: the evaluated bases, positions in the matrix, in the order of per_base
    n_used: Optional[int] = None        # graph_hyperbolicity / embedding_hyperbolicity: points that entered the matrix
    nodes_used: Optional[np.ndarray] = None       # ... and which: node indices / table rows in matrix order


def set_kernel_form(form: int) -> None:
    """Test / tuning hook (results never depend on it): the path int16 input takes from now on, process-wide.  0 = the
    default, 1 = 32-bit integer min / max, 2 = packed 16-bit min / max."""
    _lib.check(_lib.load().hm_debug_gromov_form(int(form)))


def _base_positions(base_points, n: int) -> np.ndarray:
    if base_points is None:
        return np.zeros(1, np.int32)
    if isinstance(base_points, str):
        if base_points != "all":
            raise ValueError(f"gromov_delta: base_points must be None, a sequence of positions or 'all', got {base_points!r}")
        return np.arange(n, dtype=np.int32)
    if isinstance(base_points, torch.Tensor):
        base_points = base_points.detach().cpu().numpy()
    a = np.asarray(base_points)
    if a.size == 0:
        raise ValueError("gromov_delta: base_points is empty")
    if not np.issubdtype(a.dtype, np.integer):
        raise ValueError("gromov_delta: base_points must hold integer positions")
    a = a.astype(np.int64).reshape(-1)
    if a.min() < 0 or a.max() >= n:
        raise ValueError(f"gromov_delta: base_points names a position outside [0, {n})")
    return np.ascontiguousarray(a.astype(np.int32))


def gromov_delta(dist: torch.Tensor, base_points: Union[None, str, Sequence[int], torch.Tensor] = None) -> GromovDelta:
    """Gromov delta of the square distance matrix ``dist`` (int16 or float32 on a HIP device, unit stride along its rows; other
    integer types are converted to int16 after a range check, float64 is refused) for the base points ``base_points``:
    ``None`` = position 0, a sequence of positions, or ``"all"`` = all n, the exact four-point delta at O(n^4) cost.

    One synchronising read brings the values and witnesses to the host.  Two calls return the same bits."""
    if not isinstance(dist, torch.Tensor) or dist.dim() != 2 or dist.shape[0] != dist.shape[1]:
        raise ValueError("gromov_delta: dist must be a square matrix")
    n = int(dist.shape[0])
    if not 1 <= n <= MAX_POINTS:
        raise ValueError(f"gromov_delta: dist must have between 1 and {MAX_POINTS} rows, got {n}")
    if dist.dtype == torch.float64:
        raise ValueError("gromov_delta: float64 distances are refused (the walk is float32: convert, and own the rounding)")
    if dist.dtype not in (torch.int16, torch.float32, torch.int8, torch.uint8, torch.int32, torch.int64):
        raise ValueError(f"gromov_delta: dist must be int16 or float32 (or another integer type), got {dist.dtype}")
    bases = _base_positions(base_points, n)
    _require_cuda(dist)
    d = dist.detach()
    if d.dtype not in (torch.int16, torch.float32):
        if int(d.min()) < 0 or int(d.max()) > 32767:
            raise ValueError("gromov_delta: integer distances must lie in 0..32767")
        d = d.to(torch.int16)
    if d.stride(1) != 1 or (n > 1 and d.stride(0) < n):
        d = d.contiguous()
    ld = int(d.stride(0)) if n > 1 else n
    dev = d.device
    is_int = d.dtype == torch.int16
    L = _lib.load()
    fn = L.hm_gromov_delta_i16 if is_int else L.hm_gromov_delta_f32
    per_call = max(1, min(n, _WORKSPACE_BUDGET // int(L.hm_gromov_workspace_bytes(n, 1))))
    workspace = torch.empty(int(L.hm_gromov_workspace_bytes(n, min(per_call, bases.size))), dtype=torch.uint8, device=dev)
    base_dev = torch.from_numpy(bases).to(dev)
    per_base = torch.empty(bases.size, dtype=torch.int32 if is_int else torch.float32, device=dev)
    witness = torch.empty((bases.size, 3), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        for b0 in range(0, bases.size, per_call):
            b1 = min(b0 + per_call, bases.size)
            _lib.check(fn(_ptr(d), n, ld, _ptr(base_dev[b0:b1]), b1 - b0, _ptr(per_base[b0:b1]), _ptr(witness[b0:b1]), _ptr(workspace),
                          _stream_of(d)))
    diameter = float(torch.triu(d).max())
    values = per_base.cpu().numpy()
    at = int(np.argmax(values))                                  # the first maximising base
    delta = float(values[at]) / 2.0 if is_int else float(values[at])
    i, j, k = (int(v) for v in witness[at].tolist())
    delta_rel = 2.0 * delta / diameter if diameter != 0.0 else float("nan")
    return GromovDelta(delta=delta, per_base=per_base, witness=(i, j, k, int(bases[at])), diameter=diameter, delta_rel=delta_rel, n=n,
                       base_positions=bases)


def _draw(rng: np.random.Generator, population: np.ndarray, count: int) -> np.ndarray:
    """``count`` distinct members of ``population`` (all of it when it has no more), in ascending order of position."""
    if count >= population.size:
        return population
    return population[np.sort(rng.choice(population.size, size=count, replace=False))]


def _bases_of(base_points, n_used: int, rng: np.random.Generator):
    if isinstance(base_points, (int, np.integer)) and not isinstance(base_points, bool):
        if base_points < 1:
            raise ValueError("base_points must be at least 1")
        return _draw(rng, np.arange(n_used, dtype=np.int64), int(base_points))
    return base_points


def graph_hyperbolicity(graph_or_paths, nodes=None, num_samples: int = 2048, base_points: Union[int, str, Sequence[int], None] = 8,
                        seed: int = 0) -> GromovDelta:
    """Gromov delta of the shortest-path metric of a graph, on a sample of its nodes.

    ``graph_or_paths`` is a ``GraphPaths`` or what its constructor accepts.  From ``nodes`` (node indices; omitted: every node)
    ``num_samples`` are drawn without replacement under ``numpy.random.default_rng(seed)`` (all of them when there are no
    more).  A metric needs a connected sample: of the sampled nodes those of the component that holds most of them are kept
    (``components()``; a tie goes to the smallest label) and ``n_used`` reports how many.  An int ``base_points`` means that
    many base points, drawn from the kept sample with the same generator; anything else goes to ``gromov_delta`` as positions
    in the kept sample.  ``delta`` is exact for the sample and the bases, in units of half an edge."""
    paths = graph_or_paths if isinstance(graph_or_paths, GraphPaths) else GraphPaths(graph_or_paths)
    rng = np.random.default_rng(seed)
    pool = np.arange(paths.n, dtype=np.int64) if nodes is None else paths.graph.select(nodes, "graph_hyperbolicity")
    if pool.size == 0 or num_samples < 1:
        raise ValueError("graph_hyperbolicity: nothing to sample")
    sample = _draw(rng, pool, min(int(num_samples), MAX_POINTS))
    labels = paths.components().cpu().numpy()[sample]
    names, counts = np.unique(labels, return_counts=True)       # ascending labels: argmax takes the smallest on a tie
    kept = sample[labels == names[int(np.argmax(counts))]]
    bases = _bases_of(base_points, kept.size, rng)
    out = gromov_delta(paths.distance_rows(kept, kept), bases)
    out.n_used, out.nodes_used = int(kept.size), kept
    return out


def embedding_hyperbolicity(table: torch.Tensor, nodes=None, num_samples: int = 2048,
                            base_points: Union[int, str, Sequence[int], None] = 8, seed: int = 0, c: float = 1.0,
                            sign_convention: str = "lorentz") -> GromovDelta:
    """Gromov delta of the distances ``lorentz_model.batch_distance(rows, rows, c)`` of a sample of the table's rows.

    The sample is drawn as in ``graph_hyperbolicity`` (same ``nodes``, ``num_samples`` and ``seed``: the same rows, as long as
    none is dropped).  Rows with a non-finite entry are dropped and ``n_used`` reports how many remain.  Only the ``"lorentz"``
    sign is served."""
    if sign_convention != "lorentz":
        raise ValueError(f"embedding_hyperbolicity: sign_convention must be 'lorentz', got {sign_convention!r}")
    if not isinstance(table, torch.Tensor) or table.dim() != 2 or table.dtype != torch.float32:
        raise ValueError("embedding_hyperbolicity: the table must be a float32 matrix [V, d + 1]")
    v = int(table.shape[0])
    rng = np.random.default_rng(seed)
    pool = np.arange(v, dtype=np.int64) if nodes is None else select_nodes(nodes, v, "embedding_hyperbolicity", what="row")
    if pool.size == 0 or num_samples < 1:
        raise ValueError("embedding_hyperbolicity: nothing to sample")
    _require_cuda(table)
    sample = _draw(rng, pool, min(int(num_samples), MAX_POINTS))
    rows = table.detach()[torch.from_numpy(sample).to(table.device)]
    finite = torch.isfinite(rows).all(dim=1)
    sample = sample[finite.cpu().numpy()]
    rows = rows[finite].contiguous()
    if rows.shape[0] == 0:
        raise ValueError("embedding_hyperbolicity: no finite row in the sample")
    bases = _bases_of(base_points, int(rows.shape[0]), rng)
    out = gromov_delta(lorentz_model.batch_distance(rows, rows, float(c), sign_convention="lorentz"), bases)
    out.n_used, out.nodes_used = int(rows.shape[0]), sample
    return out


def curvature_estimate(delta_rel: float, delta_unit: float = 0.144) -> float:
    """The rule of thumb of Khrulkov et al. ("Hyperbolic Image Embeddings", CVPR 2020, section 5): ``c = (delta_unit /
    delta_rel)^2``, the curvature at which a space with the relative delta of the Poincare disk (their estimate: 0.144) would
    have the data's ``delta_rel``; ``inf`` for ``delta_rel = 0`` (a tree fits every curvature).  The constant is theirs and is
    not measured here."""
    delta_rel = float(delta_rel)
    if math.isnan(delta_rel) or delta_rel < 0.0:
        raise ValueError(f"curvature_estimate: delta_rel must be a number >= 0, got {delta_rel}")
    if delta_rel == 0.0:
        return float("inf")
    return (float(delta_unit) / delta_rel) ** 2
