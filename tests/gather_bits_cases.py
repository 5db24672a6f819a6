"""Cases, seeded inputs and the C-ABI runner of the gathered-row bit fixture (tests/golden/g17_gather_kernel_bits.*), shared
by tests/golden/make_golden_gather_bits.py and tests/test_gpu_gather_kernel_bits.py.

The fixture pins the bits of the two kernel families that gather Lorentz rows by index on the lane groups of
csrc/hm_rowgroup.h: the graph edge loss (hm_edge_loss_fwd / _bwd) and Lorentz-centroid pooling
(hm_centroid_fwd / _bwd), each in both of its work decompositions (form 0: a lane group per row, form 1: a
wave per row), which differ in the order of their sums.  Like tests/row_bits_cases.py it is a covering design, not a cross
product: every width runs every batch size somewhere, and each property the kernels branch on appears at a 16-lane and at
a 32-lane width.  Every output buffer is pre-filled with the sentinel of row_bits_cases, so that "written exactly once,
everywhere" is part of what is compared.  ``cases()`` is the list; ``inputs(case)`` builds the seeded inputs on the CPU;
``run(case, inp, L)`` calls the library and returns {array name: float32 or int64 array}.
"""
from __future__ import annotations

import zlib

import numpy as np
import torch

import riemannian_cases as RC
from pooling_cases import LENGTHS, SLACK
from row_bits_cases import DEV, FILL, _buf, _rows, key  # noqa: F401  (key is re-exported)

V = 40                                                         # rows of the seeded tables
SCALES = (1e-3, 1.0, 6.0)                                      # spatial norm of row i is about SCALES[i % 3]
WIDTHS = (2, 5, 17, 65, 66, 129)                               # d1: the d < 8 sum, both sides of the 16 / 32-lane switch
COO_FILL = -7

# ---- the case list ------------------------------------------------------------------------------------------------------
# edge loss: d1 -> (B, K) pairs; K = 50 at B = 3 makes a group walk more partners than it has lanes
EL_SHAPES = {
    2: ((37, 5), (3, 50), (1, 0), (1, 1)),
    5: ((37, 5), (3, 50), (1, 1), (3, 0)),
    17: ((37, 5), (3, 50), (1, 0)),
    65: ((37, 0), (3, 5), (1, 50)),
    66: ((3, 50), (1, 5)),
    129: ((37, 0), (3, 5), (1, 1)),
}
EL_EXTRA = (
    dict(d1=17, B=3, K=5, pad=3),                              # ld = d1 + 3
    dict(d1=65, B=3, K=1, c=0.7),
    dict(d1=66, B=3, K=5, outside=1),                          # indices outside [0, V) in every role, a partner that is its anchor
)
# pooling: n bags whose lengths and slack are LENGTHS / SLACK from position ``rot`` on; L / W / G: with lengths, weights,
# grad_weights
PL_SHAPES = (
    dict(d1=2, n=37, rot=0, L=1, W=1, G=1),
    dict(d1=2, n=1, rot=0, L=1, W=0, G=0),                     # one empty bag: T = 0
    dict(d1=5, n=37, rot=0, L=1, W=0, G=0),
    dict(d1=5, n=3, rot=0, L=1, W=1, G=1),
    dict(d1=17, n=37, rot=0, L=0, W=1, G=1),
    dict(d1=17, n=3, rot=5, L=1, W=1, G=0, pad=3, off=1),      # ld = d1 + 3, the base 4 bytes past alignment
    dict(d1=65, n=3, rot=5, L=1, W=1, G=1),
    dict(d1=65, n=1, rot=7, L=0, W=0, G=0),
    dict(d1=66, n=3, rot=5, L=1, W=0, G=1),
    dict(d1=66, n=1, rot=2, L=1, W=1, G=0, spacelike=1),       # weights (1, -1): q <= 0
    dict(d1=129, n=3, rot=5, L=0, W=1, G=0, outside=1),        # ids outside [0, V)
    dict(d1=129, n=1, rot=4, L=1, W=0, G=1),
)


def cases() -> list:
    out = []
    for form in (0, 1):
        for d1, shapes in EL_SHAPES.items():
            for b, k in shapes:
                out.append(dict(fam="edge", d1=d1, B=b, K=k, form=form))
        for extra in EL_EXTRA:
            out.append(dict(fam="edge", form=form, **extra))
    for form in (0, 1):
        for shape in PL_SHAPES:
            out.append(dict(fam="pool", form=form, **shape))
    for k, c in enumerate(out):
        c["stem"] = "_".join([c["fam"]] + [f"{q}{c[q]}" for q in ("d1", "B", "K", "n", "rot", "L", "W", "G", "pad", "off", "c",
                                                                   "outside", "spacelike") if q in c])
        c["name"] = f"{k:03d}_{c['stem']}_form{c['form']}"
    return out


# ---- seeded inputs (CPU) --------------------------------------------------------------------------------------------------
def _seed(case) -> int:
    """From the stem: both forms of a case take the same inputs."""
    return zlib.crc32(case["stem"].encode()) & 0x7FFFFFFF


def _table(d1: int, gen) -> torch.Tensor:
    d = d1 - 1
    scale = torch.tensor([SCALES[i % len(SCALES)] for i in range(V)], dtype=torch.float64)[:, None]
    return RC.lift(torch.randn(V, d, generator=gen, dtype=torch.float64) * (scale / np.sqrt(d))).float()


def bag_shape(n: int, rot: int):
    """(lengths, spans) of n bags from position ``rot`` of LENGTHS / SLACK on."""
    lens = [LENGTHS[(rot + i) % len(LENGTHS)] for i in range(n)]
    return lens, [lens[i] + SLACK[(rot + i) % len(SLACK)] for i in range(n)]


def index_and_upstream(case, gen) -> dict:
    """The index [B, 2 + K] and the upstream gradient [B] of a loss on an index (tests/cone_bits_cases.py draws them too)."""
    b, k = case["B"], case["K"]
    idx = torch.randint(0, V, (b, 2 + k), generator=gen, dtype=torch.int64)
    idx[:, 1] = (idx[:, 0] + 1 + torch.randint(0, V - 1, (b,), generator=gen)) % V
    if k >= 5:
        idx[::3, 4] = -1
    if k >= 2 and b >= 3:
        idx[1, 2] = idx[1, 0]                                   # a negative that is its anchor
        idx[2, 3] = idx[2, 2]                                   # a repeated negative
    if case.get("outside"):
        idx[0, 2], idx[0, 3], idx[0, 5] = -1, V + 2, idx[0, 0]
        idx[1, 0] = V                                           # the anchor outside: the sample is skipped
        idx[2, 1] = -5                                          # the positive outside: the sample is skipped
    return {"index": idx, "g": (0.5 + torch.rand(b, generator=gen, dtype=torch.float64)).float()}


def inputs(case) -> dict:
    gen = torch.Generator().manual_seed(_seed(case))
    x = _table(case["d1"], gen)
    if case["fam"] == "edge":
        return {"x": x, **index_and_upstream(case, gen)}
    n = case["n"]
    lens, span = bag_shape(n, case["rot"])
    offsets = torch.zeros(n + 1, dtype=torch.int64)
    offsets[1:] = torch.cumsum(torch.tensor(span, dtype=torch.int64), 0)
    t = int(offsets[-1])
    ids = torch.randint(0, V, (t,), generator=gen, dtype=torch.int64)
    for i in range(n):
        b0 = int(offsets[i])
        if lens[i] == 3:
            ids[b0 + 1] = -1
        if lens[i] == 7:
            ids[b0 + 1] = ids[b0 + 3] = ids[b0]
        if case.get("outside") and lens[i] >= 16:
            ids[b0], ids[b0 + 5], ids[b0 + lens[i] - 1] = V, -3, V + 5
    weights = (0.25 + torch.rand(t, generator=gen, dtype=torch.float64)).float()
    if case.get("spacelike"):
        ids[0], ids[1] = 1, 2                                   # two rows of norm about 1 and 6: s = x_1 - x_2 is spacelike
        weights[0], weights[1] = 1.0, -1.0
    inp = {"x": x, "ids": ids, "offsets": offsets, "g": torch.randn(n, case["d1"], generator=gen, dtype=torch.float64).float()}
    if case["L"]:
        inp["lengths"] = torch.tensor(lens, dtype=torch.int32)
    if case["W"]:
        inp["weights"] = weights
    return inp


def input_digest(inp: dict) -> int:
    h = 0
    for k in sorted(inp):
        h = zlib.crc32(np.ascontiguousarray(inp[k].numpy()).tobytes(), h)
    return h


# ---- the runner ---------------------------------------------------------------------------------------------------------
def run(case, inp, L) -> dict:
    """Sets the case's form for the calls it makes; the caller restores the defaults (``restore_forms``)."""
    from hyptokenizer_amd import _lib
    from hyptokenizer_amd.engine import _ptr as P
    ck = _lib.check
    d1, pad, off = case["d1"], case.get("pad", 0), case.get("off", 0)
    x = _buf(inp["x"], pad, off)
    F = lambda *s: torch.full(s, FILL, device=DEV)                                 # noqa: E731
    dev = lambda q: inp[q].to(DEV) if q in inp else None                           # noqa: E731
    if case["fam"] == "edge":
        b, k, c = case["B"], case["K"], float(np.float32(case.get("c", 1.0)))
        index, g = dev("index"), dev("g")
        loss, w, val = F(b), F(b, 1 + k), F(b * (2 + k), d1)
        coo = torch.full((b * (2 + k),), COO_FILL, dtype=torch.int64, device=DEV)
        ck(L.hm_debug_edge_loss_form(case["form"]))
        ck(L.hm_edge_loss_fwd(P(x), d1 + pad, V, d1, P(index), b, k, c, P(loss), P(w), None))
        ck(L.hm_edge_loss_bwd(P(x), d1 + pad, V, d1, P(index), b, k, c, P(w), P(g), P(val), P(coo), None))
        res = {"loss": loss, "weights": w, "values": val, "coo": coo}
    else:
        n = case["n"]
        ids, offsets, lengths, weights, g = dev("ids"), dev("offsets"), dev("lengths"), dev("weights"), dev("g")
        t = ids.numel()
        mu, inv, val = F(n, d1), F(n), F(t, d1)
        gw = F(t) if case["G"] else None
        coo = torch.full((t,), COO_FILL, dtype=torch.int64, device=DEV)
        ck(L.hm_debug_centroid_form(case["form"]))
        ck(L.hm_centroid_fwd(P(x), d1 + pad, V, d1, P(ids), t, P(offsets), P(lengths), P(weights), n, P(mu), P(inv), None))
        ck(L.hm_centroid_bwd(P(x), d1 + pad, V, d1, P(ids), t, P(offsets), P(lengths), P(weights), n, P(mu), P(inv), P(g), P(val),
                             P(coo), P(gw), None))
        res = {"mu": mu, "inv_nu": inv, "values": val, "coo": coo}
        if gw is not None:
            res["grad_weights"] = gw
    torch.cuda.synchronize()
    assert np.array_equal(_rows(x, d1), inp["x"].numpy())                          # the table and its padding were not written
    return {q: a.cpu().numpy() for q, a in res.items()}


def restore_forms(L) -> None:
    from hyptokenizer_amd import _lib
    _lib.check(L.hm_debug_edge_loss_form(1))
    _lib.check(L.hm_debug_centroid_form(-1))


def stored(a: np.ndarray) -> np.ndarray:
    """What the fixture holds of an output: int64 COO indices as they are, fp32 as a uint32 view."""
    if a.dtype == np.int64:
        return np.ascontiguousarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
