#!/usr/bin/env python
"""Generate tests/golden/g12_retrieval_{reference,lorentz}.{npz,json} by running the REFERENCE's ``compute_recall_at_k``
(``scripts/train_retrieval.py:176-229``) on the CPU.

Like its siblings it runs only where the reference is present (it is executed, never copied) and applies the sign patch of
make_golden.py to ``embedding.lorentz_model.minkowski_dot``:
  reference : the module exactly as shipped (every distance is 0.0)
  lorentz   : ``minkowski_dot`` negated
``scripts/train_retrieval.py`` cannot be imported as shipped (it imports ``ViTFeatureExtractor``, ``datasets`` and the
``multimodal`` package whose relative import is broken): its source is read at generation time, stub
modules stand in for ``transformers``, ``datasets``, ``multimodal`` and ``multimodal.contrastive_loss``, and the module is
executed from memory (make_golden_autograd.load_losses does the same for the losses).

Per mode the npz holds, for every case ``<name>``: the fp32 inputs ``<name>__text`` and ``<name>__image`` and the
reference's six (or 2 x len(k_values)) recalls ``<name>__recall`` as float64 in the order of its dictionary.  The json
lists the cases with their k_values, the recalls by key, and ``min_gap_rows`` / ``min_gap_cols``: the smallest
``|D[i,j] - D[i,i]|`` over j != i (rows) and ``|D[i,j] - D[j,j]|`` over i != j (columns) of the reference's own distance
matrix.  Parity is bit-level, so the gaps are information, not a tolerance.

The generator asserts, for every case, that the index-stable rank rule of tests/retrieval_cases.py applied to the
reference's OWN distance matrix (captured from its ``torch.topk`` calls) reproduces the reference's numbers, and that R@1
under "lorentz" lies strictly between 0 and 1.  A tie case that ``torch.topk`` breaks otherwise would be dropped from the
goldens and named under ``dropped`` in the json.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_retrieval.py [reference|lorentz|all]
"""
from __future__ import annotations

import json
import os
import sys
import types
import warnings

REF = "/root/reference"
if not os.path.isdir(REF):
    sys.exit("make_golden_retrieval.py: /root/reference is not present; golden vectors can only be regenerated "
             "in the build container.")

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, REF)
warnings.filterwarnings("ignore")

import numpy as np  # noqa: E402
import torch  # noqa: E402

import embedding.lorentz_model as L  # noqa: E402  (reference)

import retrieval_cases as RC  # noqa: E402  (ours: the rank rule and the input builders)

_ORIG = L.minkowski_dot

#: (name, B, d, k_values, spatial scale, duplicated rows)
CASES = (
    ("B10_d1", 10, 1, [1, 5, 10], 1.0, False),
    ("B12_d8", 12, 8, [1, 5, 10], 1.0, False),
    ("B40_d8_k13", 40, 8, [1, 3], 1.0, False),
    ("B40_d64", 40, 64, [1, 5, 10], 0.3, False),
    ("B40_d8_ties", 40, 8, [1, 5, 10], 1.0, True),
    ("B200_d8", 200, 8, [1, 5, 10], 1.0, False),
    ("B200_d128_k13", 200, 128, [1, 3], 0.2, False),
    ("B500_d64", 500, 64, [1, 5, 10], 0.3, False),
)
NOISES = (0.5, 0.7, 1.0, 2.0, 0.25, 4.0)


def set_mode(mode: str) -> None:
    if mode == "reference":
        L.minkowski_dot = _ORIG
    elif mode == "lorentz":
        L.minkowski_dot = lambda a, b: -_ORIG(a, b)
    else:
        raise ValueError(mode)


def load_script():
    """The reference's training script, executed from its source with stand-ins for what it cannot import here."""
    def stub(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        return m

    stubs = {
        "transformers": stub("transformers", ViTFeatureExtractor=object, ViTModel=object, BertModel=object, BertTokenizer=object),
        "datasets": stub("datasets", load_dataset=None),
        "multimodal": stub("multimodal"),
        "multimodal.contrastive_loss": stub("multimodal.contrastive_loss", hyperbolic_contrastive_loss=None,
                                            MultimodalHyperbolicModel=object),
    }
    saved = {k: sys.modules.get(k) for k in stubs}
    sys.modules.update(stubs)
    try:
        path = os.path.join(REF, "scripts", "train_retrieval.py")
        mod = types.ModuleType("reference_train_retrieval")
        mod.__file__ = path
        exec(compile(open(path).read(), path, "exec"), mod.__dict__)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return mod


def run_reference(script, text: np.ndarray, image: np.ndarray, k_values):
    """(recall dictionary, the reference's own distance matrix as it stood when torch.topk read it)."""
    seen = {}
    real = torch.topk

    def spy(inp, *a, **kw):
        if "D" not in seen:
            base = inp._base if inp._base is not None else inp
            seen["D"] = base.detach().clone().numpy()
        return real(inp, *a, **kw)

    torch.topk = spy
    try:
        with torch.no_grad():
            res = script.compute_recall_at_k(torch.from_numpy(text), torch.from_numpy(image), list(k_values))
    finally:
        torch.topk = real
    return res, seen["D"]


def min_gaps(D: np.ndarray):
    n = D.shape[0]
    diag = np.diag(D).astype(np.float64)
    off = ~np.eye(n, dtype=bool)
    rows = np.abs(D.astype(np.float64) - diag[:, None])[off].min() if n > 1 else 0.0
    cols = np.abs(D.astype(np.float64) - diag[None, :])[off].min() if n > 1 else 0.0
    return float(rows), float(cols)


def build_inputs(name, n, d, scale, ties):
    """The same inputs in both modes: the noise is the first of NOISES that puts the "lorentz" R@1 (by the rank rule on the
    float64 Lorentz distance) well inside (0, 1)."""
    for noise in NOISES:
        rs = np.random.RandomState(abs(hash_name(name)) % (2 ** 31))
        a, b = RC.pairs(rs, n, d, scale, noise)
        if ties:
            a[7] = a[3]; b[7] = b[3]                                       # the same pair twice: exact ties in rows and columns
            a[n - 1] = a[3]; b[n - 1] = b[3]
        x, y = a.astype(np.float64), b.astype(np.float64)
        u = x[:, None, 0] * y[None, :, 0] - (x[:, None, 1:] * y[None, :, 1:]).sum(-1)
        r1 = RC.recall_truth(np.arccosh(np.maximum(u, 1.0)).astype(np.float32), [1])
        if all(0.15 < v < 0.85 for v in r1.values()):
            return a, b, noise
    raise AssertionError(f"no noise level puts R@1 of {name} inside (0, 1)")


def hash_name(name: str) -> int:
    h = 2166136261
    for ch in name.encode():
        h = ((h ^ ch) * 16777619) & 0xFFFFFFFF
    return h


def generate(mode: str) -> None:
    set_mode(mode)
    script = load_script()
    arrays, cases, dropped = {}, [], []
    for name, n, d, k_values, scale, ties in CASES:
        a, b, noise = build_inputs(name, n, d, scale, ties)
        res, D = run_reference(script, a, b, k_values)
        keys = [f"r@{k}_text2image" for k in k_values] + [f"r@{k}_image2text" for k in k_values]
        assert list(res.keys()) == keys, (name, list(res.keys()))
        rule = RC.recall_truth(D, k_values)
        reproduces = all(rule[k] == res[k] for k in keys)
        if not reproduces:
            assert ties, (name, rule, res)                                  # only a tie case may disagree with torch.topk
            dropped.append({"name": name, "reason": "torch.topk breaks this case's exact ties otherwise than by index",
                            "reference": res, "rule": rule})
            continue
        if mode == "lorentz":
            assert 0.0 < res["r@1_text2image"] < 1.0 and 0.0 < res["r@1_image2text"] < 1.0, (name, res)
        else:
            assert all(res[f"r@{k}_{s}"] == min(k, n) / n for k in k_values for s in ("text2image", "image2text")), (name, res)
        gr, gc = min_gaps(D)
        arrays[f"{name}__text"] = a
        arrays[f"{name}__image"] = b
        arrays[f"{name}__recall"] = np.array([res[k] for k in keys], np.float64)
        cases.append({"name": name, "B": n, "d": d, "k_values": list(k_values), "scale": scale, "noise": noise, "ties": bool(ties),
                      "recall": {k: res[k] for k in keys}, "min_gap_rows": gr, "min_gap_cols": gc})
        print(f"{mode}: {name}: {res}  gaps {gr:.3g} / {gc:.3g}", flush=True)
    np.savez_compressed(os.path.join(HERE, f"g12_retrieval_{mode}.npz"), **arrays)
    with open(os.path.join(HERE, f"g12_retrieval_{mode}.json"), "w") as f:
        json.dump({"mode": mode, "cases": cases, "dropped": dropped}, f, indent=1)
    print(f"{mode}: {len(cases)} cases, dropped: {[c['name'] for c in dropped]}")


if __name__ == "__main__":
    which = sys.argv[1] if len(sys.argv) > 1 else "all"
    for m in (("reference", "lorentz") if which == "all" else (which,)):
        generate(m)
