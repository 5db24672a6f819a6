"""Gromov hyperbolicity, the part that needs no GPU: the entry points exist and refuse bad arguments before a device is
touched, the host-side plan (tile list, workspace size, argument checks) holds under a sanitizer in a stand-alone program, the
Python layer raises what it documents, and the truth of tests/hyperbolicity_cases.py, maximised over all base points, equals a
brute-force four-point delta."""
import ctypes as C
import inspect
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import hyperbolicity_cases as HC

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SYMBOLS = ("hm_gromov_delta_i16", "hm_gromov_delta_f32", "hm_gromov_workspace_bytes", "hm_debug_gromov_form")


# ---- 1. the C ABI ------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_listed():
    from hyptokenizer_amd import _lib
    L = _lib.load()
    with open(os.path.join(ROOT, "include", "hypmerge.h")) as f:
        header = f.read()
    for name in SYMBOLS:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(L, name)
    assert L.hm_abi_version() == 3


@pytest.mark.parametrize("entry", ["hm_gromov_delta_i16", "hm_gromov_delta_f32"])
def test_bad_arguments_are_refused_without_a_device(entry):
    from hyptokenizer_amd import _lib
    L = _lib.load()
    E = _lib.HM_E_ARG
    P = C.c_void_p(4096)                                        # never dereferenced: every call below fails or launches nothing

    def call(d=P, n=100, ld=100, base=P, n_base=3, value=P, witness=P, workspace=P):
        return getattr(L, entry)(d, n, ld, base, n_base, value, witness, workspace, None)

    for name in ("d", "base", "value", "witness", "workspace"):
        assert call(**{name: None}) == E, name
    assert call(n=0) == E and call(n=-1) == E and call(n=32769, ld=40000) == E
    assert call(ld=99) == E
    assert call(n_base=-1) == E and call(n_base=101) == E
    assert entry.encode() in L.hm_last_error(None)
    assert call(n_base=0) == _lib.HM_OK and call(n=32768, ld=32768, n_base=0) == _lib.HM_OK and call(n=1, ld=1, n_base=0) == _lib.HM_OK


def test_form_hook_and_workspace_size():
    from hyptokenizer_amd import _lib
    L = _lib.load()
    assert L.hm_debug_gromov_form(-1) == _lib.HM_E_ARG and L.hm_debug_gromov_form(3) == _lib.HM_E_ARG
    assert b"hm_debug_gromov_form" in L.hm_last_error(None)
    for form in (1, 2, 0):
        assert L.hm_debug_gromov_form(form) == _lib.HM_OK
    T = HC.TILE
    for n, nb in ((1, 1), (T, 3), (T + 1, 3), (2 * T + 3, 1), (32768, 8)):
        nt = -(-n // T)
        assert L.hm_gromov_workspace_bytes(n, nb) == 16 * nb * nt * (nt + 1) // 2
    assert L.hm_gromov_workspace_bytes(300, 0) == 0
    for n, nb in ((0, 0), (32769, 1), (5, 6), (5, -1)):
        assert L.hm_gromov_workspace_bytes(n, nb) == -1


# ---- 2. the host-side plan, stand-alone under a sanitizer ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("gromov_plan") / "gromov_plan_driver")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", os.path.join(HERE, "gromov_plan_driver.cpp"), "-o", exe]
    if subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True).returncode != 0:
        subprocess.run(base, check=True, capture_output=True)        # a compiler without the sanitizer runtimes
    return exe


def test_plan_lists_every_tile_of_the_upper_triangle_once(driver):
    T = HC.TILE
    sizes = [1, 2, T - 1, T, T + 1, 2 * T, 2 * T + 3, 5 * T + 1, 4096, 32767, 32768]
    out = subprocess.run([driver] + [str(n) for n in sizes], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout[-400:], out.stderr[-2000:])
    lines = out.stdout.split("\n")
    for n, line in zip(sizes, lines):
        nt = -(-n // T)
        assert [int(v) for v in line.split()] == [n, nt, nt * (nt + 1) // 2, 16 * n * nt * (nt + 1) // 2, 0], line
    args = [ln.split(" ", 2)[1] for ln in lines if ln.startswith("arg ")]
    #       ok   NULL x 5 .............  n = 0, n = 32769, the largest, ld < n, n_base < 0, n_base > n, n_base = 0
    assert args == ["0", "1", "1", "1", "1", "1", "2", "2", "0", "3", "4", "4", "0"]
    assert [ln for ln in lines if ln.startswith("ws ")] == ["ws -1 -1 %d 0" % (16 * 32768 * 256 * 257 // 2)]


# ---- 3. the Python layer -----------------------------------------------------------------------------------------------------
def test_python_layer_raises_what_it_documents():
    from hyptokenizer_amd.embedding import curvature_estimate, embedding_hyperbolicity, gromov_delta
    from hyptokenizer_amd.engine import HypMergeUnavailable
    d = torch.from_numpy(HC.bfs_all_pairs(*HC.cycle(8)))
    x = torch.zeros(9, 4)
    bad = [lambda: gromov_delta(d.double()),                                     # float64 is refused
           lambda: gromov_delta(d.float().half()),
           lambda: gromov_delta(d[:, :5]),                                        # not square
           lambda: gromov_delta(d.reshape(-1)),
           lambda: gromov_delta(torch.zeros((0, 0), dtype=torch.int16)),
           lambda: gromov_delta(d, "every"),
           lambda: gromov_delta(d, []),
           lambda: gromov_delta(d, [0, 8]),                                       # a position out of range
           lambda: gromov_delta(d, [-1]),
           lambda: gromov_delta(d, [0.5]),
           lambda: embedding_hyperbolicity(x, sign_convention="reference"),
           lambda: embedding_hyperbolicity(x.double()),
           lambda: embedding_hyperbolicity(x, nodes=[0, 9]),
           lambda: embedding_hyperbolicity(x, nodes=[1, 1]),
           lambda: embedding_hyperbolicity(x, num_samples=0),
           lambda: curvature_estimate(-0.1),
           lambda: curvature_estimate(float("nan"))]
    for k, fn in enumerate(bad):
        with pytest.raises(ValueError):
            fn()
            pytest.fail(f"case {k} raised nothing")
    for fn in (lambda: gromov_delta(d), lambda: gromov_delta(d.float(), "all"), lambda: gromov_delta(d.long(), [1, 2]),
               lambda: embedding_hyperbolicity(x)):
        with pytest.raises(HypMergeUnavailable):                  # valid arguments on the CPU: there is no fallback
            fn()
    assert curvature_estimate(0.0) == math.inf
    assert curvature_estimate(0.144) == 1.0 and curvature_estimate(0.288) == 0.25
    assert curvature_estimate(0.5, delta_unit=1.0) == 4.0
    doc = inspect.getdoc(curvature_estimate)
    assert "Khrulkov" in doc and "not measured here" in doc


def test_cli_has_the_flag_off_by_default():
    from hyptokenizer_amd.scripts import train_graph_embeddings as T
    for fn in (T.main, T.train_graph_embeddings):
        assert inspect.signature(fn).parameters["eval_hyperbolicity"].default == 0


# ---- 4. the truth itself -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(HC.GRAPHS))
def test_truth_over_all_bases_is_the_four_point_delta(name):
    build, want = HC.GRAPHS[name]
    n, edges = build()
    D = HC.bfs_all_pairs(n, edges)
    assert (D >= 0).all() and np.array_equal(D, D.T)
    values, wit = HC.truth_i16(D, range(n))
    brute = HC.four_point_twice_delta(D)
    assert int(values.max()) == brute
    if want is not None:
        assert brute == want
    # every witness attains its value, and by the documented products
    for w, (v, (i, j, k)) in enumerate(zip(values, wit)):
        B = D[:, w][:, None].astype(int) + D[:, w][None, :] - D
        assert i <= j and min(B[i, k], B[k, j]) - B[i, j] == v


def test_truth_f32_agrees_with_the_integer_truth_on_small_integers():
    # distances that are small integers: every float32 step is exact, so delta_w is half the integer value, witnesses equal
    n, edges = HC.GRAPHS["random24"][0]()
    D = HC.bfs_all_pairs(n, edges)
    vi, wi = HC.truth_i16(D, range(n))
    vf, wf = HC.truth_f32(D.astype(np.float32), range(n))
    assert vf.dtype == np.float32 and np.array_equal(vf, vi.astype(np.float32) / 2) and np.array_equal(wi, wf)


def test_truth_reads_the_upper_triangle_only_and_breaks_ties_as_documented():
    D = HC.bfs_all_pairs(*HC.cycle(9)).astype(np.int16)
    junk = D.copy()
    junk[np.tril_indices(9, -1)] = 77
    assert all(np.array_equal(a, b) for a, b in zip(HC.truth_i16(D, [0, 4]), HC.truth_i16(junk, [0, 4])))
    # all-zero distances: every pair and every k tie at 0 -> (0, 0, 0)
    v, wit = HC.truth_i16(np.zeros((5, 5), np.int16), [2])
    assert v.tolist() == [0] and wit.tolist() == [[0, 0, 0]]
    # the extreme metrics of the GPU tests stay inside the packed path's range
    Dc = HC.cycle_metric(40).astype(np.int64)
    assert Dc.max() == 32767 and max((Dc[:, w][:, None] + Dc[:, w][None, :] - Dc).max() for w in range(40)) == 65534
    assert HC.truth_i16(HC.line_metric(40), [0, 7, 39])[0].tolist() == [0, 0, 0]
