"""Cases, seeded inputs and the C-ABI runner of the row-kernel bit fixture (tests/golden/g16_row_kernel_bits.*), shared by
tests/golden/make_golden_row_bits.py and tests/test_gpu_row_kernel_bits.py.

The fixture pins the bits of the kernels built on csrc/hm_rowgroup.h (Poincare ball, Riemannian steps), of the Lorentz row
primitives of csrc/hm_lorentz.hip and of the two engine kernels that share their scalars (midpoint, table projection).  The
cases are a covering design, not a cross product (the fixture has to stay small): every entry point runs at every small
width, and each large width carries a rotating subset such that every group size, both access forms, part-filled blocks and
every kernel template appear at a large width as well.  ``cases()`` is the list; ``inputs(case)`` builds the seeded fp32
inputs on the CPU; ``run(case, inp, L)`` calls the library and returns {array name: float32 array}.
"""
from __future__ import annotations

import zlib

import numpy as np
import torch

import riemannian_cases as RC

DEV = "cuda:0"
FILL = 777.0

# ---- the case list ------------------------------------------------------------------------------------------------------
PB_OPS = ("mobius_add", "distance", "scalar_mul", "exp_map_zero", "log_map_zero", "l2p", "p2l")
PB_SMALL, PB_LARGE = (1, 3, 4), (64, 65, 127, 128)
PB_FULL_AT = {"mobius_add": 64, "l2p": 65, "scalar_mul": 127, "exp_map_zero": 128}     # the large width run at b = 37
RO_SETTINGS = {
    "sgd": ("sgd", dict(lr=0.1), 0),
    "sgd_mom": ("sgd", dict(lr=0.1, momentum=0.9), 0),
    "sgd_nesterov_damp": ("sgd", dict(lr=0.1, momentum=0.9, dampening=0.1, nesterov=1), 0),
    "adam_t1": ("adam", dict(lr=0.05, beta1=0.9, beta2=0.999, eps=1e-8), 1),
    "adam_t3": ("adam", dict(lr=0.05, beta1=0.9, beta2=0.999, eps=1e-8), 3),
    "adam_t10": ("adam", dict(lr=0.05, beta1=0.9, beta2=0.999, eps=1e-8), 10),
}
RO_WIDTHS = {2: tuple(RO_SETTINGS), 5: tuple(RO_SETTINGS), 65: ("sgd", "sgd_nesterov_damp", "adam_t10"), 66: ("adam_t1",),
             129: ("sgd", "sgd_nesterov_damp")}
LZ_OPS = ("minkowski", "distance", "log_map", "exp_map", "project")
LZ_SIGNED = ("minkowski", "distance", "log_map")              # the others take no sign mode
LZ_LARGE = {101: (("log_map", 1),), 129: (("exp_map", 0), ("project", 0))}


def cases() -> list:
    out = []
    for k, op in enumerate(PB_OPS):
        for d in PB_SMALL:
            out.append(dict(fam="poincare", op=op, d=d, b=37, c=(1.0, 0.7)[(k + d) % 2]))
        for d in PB_LARGE:
            full = PB_FULL_AT.get(op) == d
            out.append(dict(fam="poincare", op=op, d=d, b=37 if full else 1, c=(1.0, 0.7)[(k + (d & 1)) % 2]))
    out.append(dict(fam="poincare", op="mobius_add", d=1, b=1, c=1.0))
    out.append(dict(fam="poincare", op="p2l", d=4, b=37, c=0.7, standard=1))
    out.append(dict(fam="poincare", op="distance", d=64, b=37, c=0.7, pad=3))                  # leading dimensions d + 3
    out.append(dict(fam="poincare", op="log_map_zero", d=64, b=37, c=1.0, off=1))              # bases 4 bytes past alignment
    for d1, settings in RO_WIDTHS.items():
        for s in settings:
            out.append(dict(fam="riemann", setting=s, d1=d1, n=37))
    out.append(dict(fam="riemann", setting="sgd_mom", d1=66, n=37, pads=[3, 1, 5]))            # a leading dimension per operand
    out.append(dict(fam="riemann", setting="adam_t3", d1=65, n=11, table=37, indexed=1))       # 11 rows of a 37-row table
    for d1 in (2, 9, 33):
        for k, op in enumerate(LZ_OPS):
            for sign in ((0, 1) if op in LZ_SIGNED and d1 < 33 else ((k + 1) % 2,)):
                out.append(dict(fam="lorentz", op=op, d1=d1, b=37, sign=sign))
    for k, op in enumerate(LZ_OPS):
        out.append(dict(fam="lorentz", op=op, d1=2, b=300, sign=k % 2))                        # 300 rows cross the 128-thread block
    out.append(dict(fam="lorentz", op="log_map", d1=9, b=300, sign=1))
    for d1, ops in LZ_LARGE.items():
        for op, sign in ops:
            out.append(dict(fam="lorentz", op=op, d1=d1, b=37, sign=sign))
    for sign in (0, 1):
        out.append(dict(fam="lorentz", op="batch_distance", d1=33, b=37, b2=41, sign=sign))
    out.append(dict(fam="engine", op="midpoint", d1=33, b=5, rows=70))
    out.append(dict(fam="engine", op="project_table", d1=33, rows=70))
    for k, c in enumerate(out):
        c["name"] = "_".join([f"{k:03d}", c["fam"], c.get("op", c.get("setting"))] + [f"{q}{c[q]}" for q in ("d", "d1", "b", "n") if q in c])
    return out


# ---- seeded inputs (CPU, fp32) ----------------------------------------------------------------------------------------------
ZERO_ROW, EDGE_ROW = 5, 9                                     # Poincare: the zero vector; a row at norm >= 1 / sqrt(c)
SAME_ROW, NEAR_ROWS, TINY_ROW = 3, (6, 7), 8                  # Lorentz: y == x; two rows 1e-3 around a common point; |v| < 1e-4
ZERO_G_ROW, NAN_G_ROW = 11, 20                                # Riemannian: a zero gradient row and a NaN gradient row


def _seed(case) -> int:
    return zlib.crc32(case["name"].encode()) & 0x7FFFFFFF


def ball(n, d, c, gen, cap=0.9, lo=0.05):
    v = torch.randn(n, d, generator=gen)
    v = v / v.norm(dim=-1, keepdim=True)
    return (v * (lo + (cap - lo) * torch.rand(n, 1, generator=gen)) / np.sqrt(c)).float()


def _hyperboloid(n, d1, gen, scale=0.7):
    return RC.lift(torch.randn(n, d1 - 1, generator=gen, dtype=torch.float64) * (scale / np.sqrt(d1 - 1))).float()


def inputs(case) -> dict:
    gen = torch.Generator().manual_seed(_seed(case))
    fam = case["fam"]
    if fam == "poincare":
        b, d, c, op = case["b"], case["d"], case["c"], case["op"]
        x, y = ball(b, d, c, gen), ball(b, d, c, gen)
        if b > EDGE_ROW:
            x[ZERO_ROW] = 0.0
            x[EDGE_ROW] = x[EDGE_ROW] / x[EDGE_ROW].norm() * (1.001 / np.sqrt(c))
        inp = {"x": x}
        if op == "l2p":
            inp["x"] = RC.lift(x.double() * 3.0).float()
        if op in ("mobius_add", "distance"):
            inp["y"] = y
        if op == "scalar_mul":
            inp["r"] = (torch.rand(b, generator=gen) + 0.5).float()
        gw = 1 if op == "distance" else d + 1 if op == "p2l" else d
        inp["g"] = torch.randn(b, gw, generator=gen)
        return inp
    if fam == "riemann":
        rows = case.get("table", case["n"])
        x, gs, m, v = RC.inputs(rows, case["d1"], 0.3, _seed(case))
        g = gs[0].clone()
        inp = {"x": x, "m": m, "v": v}
        if case.get("indexed"):
            idx = torch.randperm(rows, generator=gen)[: case["n"]].clone()
            idx[2], idx[7] = -1, rows + 3                       # outside the table: skipped, never written
            inp["rows"] = idx.to(torch.int64)
            g = g[: case["n"]].clone()
        elif case["d1"] == 5:
            g[ZERO_G_ROW] = 0.0
            g[NAN_G_ROW, 2] = float("nan")
        inp["g"] = g
        return inp
    if fam == "lorentz":
        b, d1 = case["b"], case["d1"]
        x, y = _hyperboloid(b, d1, gen), _hyperboloid(case.get("b2", b), d1, gen)
        if case["op"] != "batch_distance":
            y[SAME_ROW] = x[SAME_ROW]
            p = torch.randn(d1 - 1, generator=gen, dtype=torch.float64) * 0.5
            for r in NEAR_ROWS:
                for t in (x, y):
                    t[r] = RC.lift(p + 1.0e-3 * torch.randn(d1 - 1, generator=gen, dtype=torch.float64)).float()
        v = RC.rgrad(x.double(), torch.randn(b, d1, generator=gen, dtype=torch.float64)).float()
        v[TINY_ROW] = v[TINY_ROW] / v[TINY_ROW, 1:].norm().clamp(min=1e-30) * 3.0e-5
        gshape = {"minkowski": (b,), "distance": (b,), "batch_distance": (b, case.get("b2", b))}.get(case["op"], (b, d1))
        return {"x": x, "y": y, "v": v, "g": torch.randn(*gshape, generator=gen)}
    table = _hyperboloid(case["rows"], case["d1"], gen)
    inp = {"table": table}
    if case["op"] == "midpoint":
        inp["I"] = torch.randint(0, case["rows"], (case["b"],), generator=gen).to(torch.int32)
        inp["J"] = torch.randint(0, case["rows"], (case["b"],), generator=gen).to(torch.int32)
        inp["W"] = torch.rand(case["b"], generator=gen)
    else:
        table[:, 0] = 1.0                                       # off the hyperboloid: the projection has something to do
    return inp


def input_digest(inp: dict) -> int:
    h = 0
    for k in sorted(inp):
        h = zlib.crc32(np.ascontiguousarray(inp[k].numpy()).tobytes(), h)
    return h


# ---- the runner ------------------------------------------------------------------------------------------------------------------
def _buf(a: torch.Tensor, pad: int = 0, off: int = 0) -> torch.Tensor:
    """[n, w] rows -> a device view with leading dimension w + pad, starting ``off`` floats past an aligned base."""
    a = a.reshape(a.shape[0], -1)
    n, w = a.shape
    store = torch.full((off + n * (w + pad),), FILL, device=DEV)
    view = store[off:].view(n, w + pad)
    view[:, :w] = a.to(DEV)
    assert view.data_ptr() % 16 == 4 * off
    return view


def _rows(view: torch.Tensor, w: int) -> np.ndarray:
    assert bool((view[:, w:] == FILL).all())                    # the padding was not written
    return view[:, :w].cpu().numpy()


def run(case, inp, L) -> dict:
    from hyptokenizer_amd import _lib
    from hyptokenizer_amd.engine import MergeEngine, _ptr
    P, ck = _ptr, _lib.check
    fam = case["fam"]
    if fam == "poincare":
        b, d, c, op = case["b"], case["d"], float(np.float32(case["c"])), case["op"]
        pad, off = case.get("pad", 0), case.get("off", 0)
        B = lambda a: _buf(a, pad, off)                                            # noqa: E731
        Z = lambda w: _buf(torch.zeros(b, w), pad, off)                            # noqa: E731
        x, g = B(inp["x"]), B(inp["g"])
        if op in ("mobius_add", "distance"):
            y, gx, gy = B(inp["y"]), Z(d), Z(d)
            if op == "mobius_add":
                o = Z(d)
                ck(L.hm_rows_mobius_add(P(x), P(y), b, d + pad, d, c, P(o), d + pad, None))
                ck(L.hm_rows_mobius_add_bwd(P(x), P(y), P(g), d + pad, b, d + pad, d, c, P(gx), P(gy), d + pad, None))
                return {"out": _rows(o, d), "gx": _rows(gx, d), "gy": _rows(gy, d)}
            o, g = torch.zeros(b, device=DEV), inp["g"].reshape(-1).to(DEV)
            ck(L.hm_rows_poincare_distance(P(x), P(y), b, d + pad, d, c, P(o), None))
            ck(L.hm_rows_poincare_distance_bwd(P(x), P(y), P(g), b, d + pad, d, c, P(gx), P(gy), d + pad, None))
            return {"out": o.cpu().numpy(), "gx": _rows(gx, d), "gy": _rows(gy, d)}
        if op == "scalar_mul":
            r, gr, o, gx = inp["r"].to(DEV), torch.zeros(b, device=DEV), Z(d), Z(d)
            ck(L.hm_rows_mobius_scalar_mul(P(r), P(x), b, d + pad, d, c, P(o), d + pad, None))
            ck(L.hm_rows_mobius_scalar_mul_bwd(P(r), P(x), P(g), d + pad, b, d + pad, d, c, P(gr), P(gx), d + pad, None))
            return {"out": _rows(o, d), "gr": gr.cpu().numpy(), "gx": _rows(gx, d)}
        if op in ("exp_map_zero", "log_map_zero"):
            fwd, bwd = getattr(L, "hm_rows_" + op), getattr(L, "hm_rows_" + op + "_bwd")
            o, gx = Z(d), Z(d)
            ck(fwd(P(x), b, d + pad, d, c, P(o), d + pad, None))
            ck(bwd(P(x), P(g), d + pad, b, d + pad, d, c, P(gx), d + pad, None))
            return {"out": _rows(o, d), "gx": _rows(gx, d)}
        if op == "l2p":
            o, gx = Z(d), Z(d + 1)
            ck(L.hm_rows_lorentz_to_poincare(P(x), b, d + 1 + pad, d, c, P(o), d + pad, None))
            ck(L.hm_rows_lorentz_to_poincare_bwd(P(x), P(g), d + pad, b, d + 1 + pad, d, c, P(gx), d + 1 + pad, None))
            return {"out": _rows(o, d), "gx": _rows(gx, d + 1)}
        o, gx, std = Z(d + 1), Z(d), case.get("standard", 0)
        ck(L.hm_rows_poincare_to_lorentz(P(x), b, d + pad, d, c, std, P(o), d + 1 + pad, None))
        ck(L.hm_rows_poincare_to_lorentz_bwd(P(x), P(g), d + 1 + pad, b, d + pad, d, c, std, P(gx), d + pad, None))
        return {"out": _rows(o, d + 1), "gx": _rows(gx, d)}
    if fam == "riemann":
        opt, kw, t = RO_SETTINGS[case["setting"]]
        d1, n, pads = case["d1"], case["n"], case.get("pads", [0, 0, 0])
        table = case.get("table", n)
        x, g, m = _buf(inp["x"], pads[0]), _buf(inp["g"], pads[1]), _buf(inp["m"], pads[2])
        v = inp["v"].to(DEV).clone()
        rows = inp["rows"].to(DEV) if "rows" in inp else None
        if opt == "sgd":
            mu = kw.get("momentum", 0.0)
            ck(L.hm_rsgd_step(P(x), d1 + pads[0], P(g), d1 + pads[1], P(m) if mu else None, d1 + pads[2], P(rows), n, table, d1,
                              kw["lr"], mu, kw.get("dampening", 0.0), kw.get("nesterov", 0), None))
            res = {"x": _rows(x, d1)}
            if mu:
                res["m"] = _rows(m, d1)
        else:
            bc1, bc2 = RC.bias_corrections(kw["beta1"], kw["beta2"], t)
            ck(L.hm_radam_step(P(x), d1 + pads[0], P(g), d1 + pads[1], P(m), d1 + pads[2], P(v), P(rows), n, table, d1, kw["lr"],
                               kw["beta1"], kw["beta2"], kw["eps"], bc1, bc2, None))
            res = {"x": _rows(x, d1), "m": _rows(m, d1), "v": v.cpu().numpy()}
        assert bool((g[:, d1:] == FILL).all())
        return res
    if fam == "lorentz":
        b, d1, sign, op = case["b"], case["d1"], case["sign"], case["op"]
        x, y, v, g = (inp[k].to(DEV).contiguous() for k in ("x", "y", "v", "g"))
        Z = lambda *s: torch.zeros(*s, device=DEV)                                 # noqa: E731
        if op == "batch_distance":
            b2 = case["b2"]
            o, gx, gy = Z(b, b2), Z(b, d1), Z(b2, d1)
            ck(L.hm_batch_distance(P(x), b, P(y), b2, d1, d1, d1, 1.0, sign, P(o), None))
            ck(L.hm_batch_distance_bwd(P(x), b, P(y), b2, d1, d1, d1, 1.0, sign, P(g), b2, P(gx), P(gy), d1, None))
            return {"out": o.cpu().numpy(), "gx": gx.cpu().numpy(), "gy": gy.cpu().numpy()}
        o, gx, gy = (Z(b) if op in ("minkowski", "distance") else Z(b, d1)), Z(b, d1), Z(b, d1)
        if op == "minkowski":
            ck(L.hm_rows_minkowski(P(x), P(y), b, d1, d1, sign, P(o), None))
            ck(L.hm_rows_minkowski_bwd(P(x), P(y), P(g), b, d1, d1, sign, P(gx), P(gy), d1, None))
        elif op == "distance":
            ck(L.hm_rows_distance(P(x), P(y), b, d1, d1, 1.0, sign, P(o), None))
            ck(L.hm_rows_distance_bwd(P(x), P(y), P(g), b, d1, d1, 1.0, sign, P(gx), P(gy), d1, None))
        elif op == "log_map":
            ck(L.hm_rows_log_map(P(x), P(y), b, d1, d1, sign, P(o), d1, None))
            ck(L.hm_rows_log_map_bwd(P(x), P(y), P(g), d1, b, d1, d1, sign, P(gx), P(gy), d1, None))
        elif op == "exp_map":
            ck(L.hm_rows_exp_map(P(x), P(v), b, d1, d1, P(o), d1, None))
            ck(L.hm_rows_exp_map_bwd(P(x), P(v), P(g), d1, b, d1, d1, P(gx), P(gy), d1, None))
        else:
            c = float(np.float32(0.7))
            ck(L.hm_rows_project(P(x), b, d1, d1, c, P(o), d1, None))
            ck(L.hm_rows_project_bwd(P(x), P(g), d1, b, d1, d1, c, P(gx), d1, None))
            return {"out": o.cpu().numpy(), "gx": gx.cpu().numpy()}
        return {"out": o.cpu().numpy(), "gx": gx.cpu().numpy(), "gy": gy.cpu().numpy()}
    rows, d1 = case["rows"], case["d1"]
    table = inp["table"].to(DEV).contiguous()
    eng = MergeEngine(rows, d1, "lorentz", torch.device(DEV))
    eng.set_table(table, rows)
    if case["op"] == "midpoint":
        return {"out": eng.midpoint(inp["I"].numpy(), inp["J"].numpy(), inp["W"].numpy(), 1.0).cpu().numpy()}
    eng.project_table(table, rows, 1.0)
    return {"table": table.cpu().numpy()}


def key(case, q: str) -> str:
    return f"{case['name']}__{q}"
