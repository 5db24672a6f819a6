#!/usr/bin/env python
"""Generate tests/golden/g17_gather_kernel_bits.{npz,json}: the raw bits of every output of the edge-loss and
centroid-pooling kernels for the cases of tests/gather_bits_cases.py (fp32 as uint32, int64 COO indices as they are),
recorded from the library this process loads.

The fixture was recorded ONCE, with the library built from the commit before the two families moved onto the shared
Lorentz-row and gathered-walk layer of csrc/hm_rowgroup.h (selected with HYPMERGE_LIB), and pins those bits, in both work
decompositions of either family, for every later build.  It is not regenerated to make
tests/test_gpu_gather_kernel_bits.py pass: a difference there means a kernel changed its arithmetic or the order of a sum.
Adding cases needs a build of a commit whose bits are trusted.

The json lists the cases with the crc32 of their seeded inputs (the test rebuilds the inputs and checks it first) and the
names of their outputs.  Needs a GPU.

Usage:  HYPMERGE_LIB=/path/to/trusted/libhypmerge.so python tests/golden/make_golden_gather_bits.py [--out-dir DIR]
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

import gather_bits_cases as GB  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=HERE)
    args = ap.parse_args()
    from hyptokenizer_amd import _lib
    L = _lib.load()
    arrays, meta = {}, []
    try:
        for case in GB.cases():
            inp = GB.inputs(case)
            res = GB.run(case, inp, L)
            for q, a in res.items():
                arrays[GB.key(case, q)] = GB.stored(a)
            meta.append(dict(case, inputs_crc32=GB.input_digest(inp), outputs=sorted(res),
                             nonfinite=bool(any(not np.isfinite(a).all() for a in res.values()))))
    finally:
        GB.restore_forms(L)
    os.makedirs(args.out_dir, exist_ok=True)
    np.savez_compressed(os.path.join(args.out_dir, "g17_gather_kernel_bits.npz"), **arrays)
    with open(os.path.join(args.out_dir, "g17_gather_kernel_bits.json"), "w") as f:
        json.dump({"library": os.path.basename(_lib.LIB_PATH), "cases": meta}, f, indent=1)
    size = os.path.getsize(os.path.join(args.out_dir, "g17_gather_kernel_bits.npz"))
    print(f"{len(meta)} cases, {len(arrays)} arrays, {size} bytes")


if __name__ == "__main__":
    main()
