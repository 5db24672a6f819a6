#!/usr/bin/env python
"""Generate tests/golden/g18_cone_kernel_bits.{npz,json}: the raw bits of every output of the entailment-cone kernels
(hm_cone_loss_fwd, hm_cone_loss_bwd) for the cases of tests/cone_bits_cases.py (fp32 as uint32, int64 COO indices as they
are), recorded from the library this process loads.

The fixture was recorded ONCE, with the library built from the commit before the cone loss and the edge loss moved onto the
shared index-loss layer of csrc/hm_index_loss.h (selected with HYPMERGE_LIB), and pins those bits, in both work
decompositions and both apex roles, for every later build.  It is not regenerated to make
tests/test_gpu_cone_kernel_bits.py pass: a difference there means a kernel changed its arithmetic or the order of a sum.
Adding cases needs a build of a commit whose bits are trusted.

The json lists the cases with the crc32 of their seeded inputs (the test rebuilds the inputs and checks it first) and the
names of their outputs.  Needs a GPU.

Usage:  HYPMERGE_LIB=/path/to/trusted/libhypmerge.so python tests/golden/make_golden_cone_bits.py [--out-dir DIR]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np  # noqa: E402

import cone_bits_cases as CB  # noqa: E402

STEM = "g18_cone_kernel_bits"


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=HERE)
    args = ap.parse_args()
    from hyptokenizer_amd import _lib
    L = _lib.load()
    arrays, meta = {}, []
    try:
        for case in CB.cases():
            inp = CB.inputs(case)
            res = CB.run(case, inp, L)
            for q, a in res.items():
                arrays[CB.key(case, q)] = CB.stored(a)
            meta.append(dict(case, inputs_crc32=CB.input_digest(inp), outputs=sorted(res),
                             nonfinite=bool(any(not np.isfinite(a).all() for a in res.values()))))
    finally:
        CB.restore_forms(L)
    os.makedirs(args.out_dir, exist_ok=True)
    np.savez_compressed(os.path.join(args.out_dir, STEM + ".npz"), **arrays)
    with open(os.path.join(args.out_dir, STEM + ".json"), "w") as f:
        json.dump({"library": os.path.basename(_lib.LIB_PATH), "cases": meta}, f, indent=1)
    size = os.path.getsize(os.path.join(args.out_dir, STEM + ".npz"))
    print(f"{len(meta)} cases, {len(arrays)} arrays, {size} bytes")


if __name__ == "__main__":
    main()
