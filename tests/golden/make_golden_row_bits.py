#!/usr/bin/env python
"""Generate tests/golden/g16_row_kernel_bits.{npz,json}: the raw fp32 bits (as uint32) of every output of the row kernels
for the cases of tests/row_bits_cases.py, recorded from the library this process loads.

The fixture was recorded ONCE, with the library built from the commit before the kernels moved onto csrc/hm_rowgroup.h and
csrc/hm_lorentz.hip (selected with HYPMERGE_LIB), and pins those bits for every later build.  It is not regenerated to
make tests/test_gpu_row_kernel_bits.py pass: a difference there means a kernel changed its arithmetic.  Adding cases needs a
build of a commit whose bits are trusted.

The json lists the cases with the crc32 of their seeded inputs (the test rebuilds the inputs and checks it first) and the
names of their outputs.  Needs a GPU.

Usage:  HYPMERGE_LIB=/path/to/trusted/libhypmerge.so python tests/golden/make_golden_row_bits.py [--out-dir DIR]
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
import torch  # noqa: E402

import row_bits_cases as BC  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=HERE)
    args = ap.parse_args()
    from hyptokenizer_amd import _lib
    L = _lib.load()
    arrays, meta = {}, []
    for case in BC.cases():
        inp = BC.inputs(case)
        res = BC.run(case, inp, L)
        torch.cuda.synchronize()
        for q, a in res.items():
            arrays[BC.key(case, q)] = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
        meta.append(dict(case, inputs_crc32=BC.input_digest(inp), outputs=sorted(res),
                         nonfinite=bool(any(not np.isfinite(a).all() for a in res.values()))))
    os.makedirs(args.out_dir, exist_ok=True)
    np.savez_compressed(os.path.join(args.out_dir, "g16_row_kernel_bits.npz"), **arrays)
    with open(os.path.join(args.out_dir, "g16_row_kernel_bits.json"), "w") as f:
        json.dump({"library": os.path.basename(_lib.LIB_PATH), "cases": meta}, f, indent=1)
    size = os.path.getsize(os.path.join(args.out_dir, "g16_row_kernel_bits.npz"))
    print(f"{len(meta)} cases, {len(arrays)} arrays, {size} bytes")


if __name__ == "__main__":
    main()
