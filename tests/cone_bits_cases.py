"""Cases, seeded inputs and the C-ABI runner of the cone-kernel bit fixture (tests/golden/g18_cone_kernel_bits.*), shared by
tests/golden/make_golden_cone_bits.py and tests/test_gpu_cone_kernel_bits.py.

The fixture pins the bits of hm_cone_loss_fwd / _bwd, whose arithmetic is order-sensitive on purpose, in
both work decompositions (form 0: a lane group per sample, form 1: a wave per sample) and both apex roles.  It is the cone
family's counterpart of tests/gather_bits_cases.py and shares its conventions: a covering design, not a cross product --
every width runs every batch size, each property the kernels branch on appears at a 16-lane and at a 32-lane width -- and
every output buffer pre-filled with the sentinel, so that "written exactly once, everywhere" is part of what is compared.
The index and the upstream gradient are drawn as the edge family's are; the tables are the ray tables of
tests/cones_cases.py (on the random tables of gather_bits_cases no hinge of a negative is ever active and the fixture would
pin zeros), width 2 a line of its own.  ``cases()`` is the list; ``inputs(case)`` builds the seeded inputs on the CPU;
``run(case, inp, L)`` calls the library and returns {array name: float32 or int64 array}.
"""
from __future__ import annotations

import zlib

import numpy as np
import torch

import cones_cases as CC
from gather_bits_cases import COO_FILL, V, WIDTHS, index_and_upstream, input_digest, stored  # noqa: F401  (re-exported)
from riemannian_cases import lift
from row_bits_cases import DEV, FILL, _buf, _rows, key  # noqa: F401

assert V == CC.V
APERTURE_K = CC.APERTURE_K
MARGINS = CC.MARGINS
LINE_SEED = 11                                                 # width 2 has no entry in cones_cases.TABLE_SEEDS

# d1 -> (B, K, margin); K = 50 at B = 3 makes a group walk more partners than it has lanes
SHAPES = {
    2: ((37, 5, 0.5), (3, 50, 0.01), (1, 0, 0.01), (1, 1, 0.5)),
    5: ((37, 5, 0.01), (3, 50, 0.5), (1, 1, 0.01), (3, 0, 0.5)),
    17: ((37, 5, 0.5), (3, 50, 0.01), (1, 0, 0.5)),
    65: ((37, 0, 0.01), (3, 5, 0.5), (1, 50, 0.5)),
    66: ((37, 1, 0.5), (3, 50, 0.5), (1, 5, 0.01)),
    129: ((37, 0, 0.5), (3, 5, 0.5), (1, 1, 0.01)),
}
EXTRA = (
    dict(d1=17, B=3, K=5, margin=0.5, pad=3),                  # ld = d1 + 3
    dict(d1=66, B=3, K=5, margin=0.5, outside=1),              # indices outside [0, V) in every role, a partner that is its anchor
)


def cases() -> list:
    shapes = [dict(d1=d1, B=b, K=k, margin=m) for d1, rows in SHAPES.items() for b, k, m in rows] + [dict(e) for e in EXTRA]
    out = []
    for form in (0, 1):
        for role in (0, 1):
            for shape in shapes:
                out.append(dict(fam="cone", form=form, role=role, **shape))
    for k, c in enumerate(out):
        c["stem"] = "_".join(["cone"] + [f"{q}{c[q]}" for q in ("d1", "B", "K", "margin", "pad", "outside") if q in c])
        c["name"] = f"{k:03d}_{c['stem']}_role{c['role']}_form{c['form']}"
    return out


# ---- seeded inputs (CPU) --------------------------------------------------------------------------------------------------
def line_table(seed: int = LINE_SEED) -> torch.Tensor:
    """Width 2: cones_cases.ray_table has no normal to tilt along there.  Row i lies at signed distance +-RADII[(i // 4) % 4]
    from the origin, scaled by a seeded factor in [0.8, 1.2]; every fourth row sits within 2 K / S_MAX, where the aperture
    is clamped as well."""
    gen = torch.Generator().manual_seed(7000 * 2 + seed)
    sign = torch.where(torch.rand(V, generator=gen, dtype=torch.float64) < 0.5, -1.0, 1.0)
    radius = torch.tensor([CC.RADII[(i // 4) % 4] for i in range(V)], dtype=torch.float64)
    radius[::4] = 0.15
    return lift((sign * radius * (0.8 + 0.4 * torch.rand(V, generator=gen, dtype=torch.float64)))[:, None]).float()


def table(d1: int) -> torch.Tensor:
    return line_table() if d1 == 2 else CC.ray_table(d1)


def inputs(case) -> dict:
    """From the stem: both forms and both roles of a case take the same inputs."""
    gen = torch.Generator().manual_seed(zlib.crc32(case["stem"].encode()) & 0x7FFFFFFF)
    return {"x": table(case["d1"]), **index_and_upstream(case, gen)}


# ---- the runner ---------------------------------------------------------------------------------------------------------
def run(case, inp, L) -> dict:
    """Sets the case's form for the calls it makes; the caller restores the default (``restore_forms``)."""
    from hyptokenizer_amd import _lib
    from hyptokenizer_amd.engine import _ptr as P
    ck = _lib.check
    d1, pad, b, k, role = case["d1"], case.get("pad", 0), case["B"], case["K"], case["role"]
    ap, margin = float(np.float32(APERTURE_K)), float(np.float32(case["margin"]))
    x = _buf(inp["x"], pad, 0)
    F = lambda *s: torch.full(s, FILL, device=DEV)                                 # noqa: E731
    index, g = inp["index"].to(DEV), inp["g"].to(DEV)
    loss, w, val = F(b), F(b, 1 + k, 4), F(b * (2 + k), d1)
    coo = torch.full((b * (2 + k),), COO_FILL, dtype=torch.int64, device=DEV)
    ck(L.hm_debug_cone_loss_form(case["form"]))
    ck(L.hm_cone_loss_fwd(P(x), d1 + pad, V, d1, P(index), b, k, ap, margin, role, P(loss), P(w), None))
    ck(L.hm_cone_loss_bwd(P(x), d1 + pad, V, d1, P(index), b, k, ap, margin, role, P(w), P(g), P(val), P(coo), None))
    torch.cuda.synchronize()
    assert np.array_equal(_rows(x, d1), inp["x"].numpy())                          # the table and its padding were not written
    return {q: a.cpu().numpy() for q, a in {"loss": loss, "weights": w, "values": val, "coo": coo}.items()}


def restore_forms(L) -> None:
    from hyptokenizer_amd import _lib
    _lib.check(L.hm_debug_cone_loss_form(1))
