"""Fused retrieval on the GPU: ``retrieval_ranks`` / ``compute_recall_at_k`` / ``hyperbolic_knn`` against the CPU truth of
tests/retrieval_cases.py on the oracle's canonical distances and against the goldens recorded from the reference (g12).
Every comparison is exact: ranks and indices as integers, distances by their bits, recalls as Python floats."""
import json
import os

import numpy as np
import pytest
import torch

import retrieval_cases as RC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = ("reference", "lorentz")


def R():
    from hyptokenizer_amd.multimodal import retrieval
    return retrieval


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check_ranks(oracle, a, b, mode, ta=None, tb=None):
    D = oracle.batch_distance(a, b, 1.0, RC.SIGN_MODE[mode])
    want_r, want_c = RC.ranks_truth(D)
    ta = torch.from_numpy(a).to(DEV) if ta is None else ta
    tb = torch.from_numpy(b).to(DEV) if tb is None else tb
    got_r, got_c = R().retrieval_ranks(ta, tb, sign_convention=mode)
    assert got_r.dtype == torch.int32 and got_c.dtype == torch.int32 and got_r.is_cuda
    assert np.array_equal(got_r.cpu().numpy(), want_r), (mode, a.shape, np.nonzero(got_r.cpu().numpy() != want_r)[0][:8])
    assert np.array_equal(got_c.cpu().numpy(), want_c), (mode, a.shape, np.nonzero(got_c.cpu().numpy() != want_c)[0][:8])
    return D


def check_knn(oracle, q, keys, k, c, mode, exclude_self=False):
    D = oracle.batch_distance(q, keys, c, RC.SIGN_MODE[mode])
    want_d, want_i = RC.knn_truth(D, k, exclude_self)
    got_d, got_i = R().hyperbolic_knn(torch.from_numpy(q).to(DEV), torch.from_numpy(keys).to(DEV), k, c, sign_convention=mode,
                                      exclude_self=exclude_self)
    assert got_d.dtype == torch.float32 and got_i.dtype == torch.int64 and got_d.shape == got_i.shape == (q.shape[0], k)
    gi, gd = got_i.cpu().numpy(), got_d.cpu().numpy()
    assert np.array_equal(gi, want_i), (mode, k, c, np.argwhere(gi != want_i)[:8])
    assert np.array_equal(bits(gd), bits(want_d)), (mode, k, c)
    return want_i


# ---- 1. ranks and recall on the goldens ---------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_goldens_ranks_and_recall(oracle, golden_dir, mode):
    meta = json.load(open(os.path.join(golden_dir, f"g12_retrieval_{mode}.json")))
    z = np.load(os.path.join(golden_dir, f"g12_retrieval_{mode}.npz"))
    assert meta["cases"]
    for c in meta["cases"]:
        a, b = z[f"{c['name']}__text"], z[f"{c['name']}__image"]
        check_ranks(oracle, a, b, mode)
        got = R().compute_recall_at_k(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV), c["k_values"], sign_convention=mode)
        assert list(got.keys()) == list(c["recall"].keys())
        for key, want in c["recall"].items():
            assert isinstance(got[key], float) and got[key] == want, (c["name"], key, got[key], want)
    a, b = z[f"{meta['cases'][0]['name']}__text"], z[f"{meta['cases'][0]['name']}__image"]
    ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    with torch.no_grad():
        default = R().compute_recall_at_k(ta.requires_grad_(), tb, sign_convention=mode)        # default k_values, no autograd
    assert list(default.keys()) == [f"r@{k}_{s}" for s in ("text2image", "image2text") for k in (1, 5, 10)]


# ---- 2. ranks on seeded tables ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_ranks_equal_the_truth_on_seeded_tables(oracle, mode):
    seen = 0
    for n in (1, 2, 63, 64, 65, 1000, 4097):
        for d1 in (2, 9, 65, 129):
            rs = np.random.RandomState(1000 * n + d1)
            a, b = RC.special_pairs(rs, n, d1 - 1, scale=0.5 if d1 > 9 else 1.0, noise=0.7)
            D = check_ranks(oracle, a, b, mode)
            if mode == "lorentz" and n >= 63:
                assert np.isnan(D).any() and (D == 0).sum() > n // 8                             # the special rows are in play
            seen += 1
    assert seen == 28


@pytest.mark.parametrize("mode", MODES)
def test_ranks_of_non_contiguous_inputs(oracle, mode):
    rs = np.random.RandomState(5)
    a, b = RC.special_pairs(rs, 300, 16)
    wide_a = torch.full((300, 40), 7.0, device=DEV)
    wide_a[:, 3:20] = torch.from_numpy(a).to(DEV)
    cols_b = torch.from_numpy(np.ascontiguousarray(b.T)).to(DEV).t()                            # column-major
    assert not wide_a[:, 3:20].is_contiguous() and not cols_b.is_contiguous()
    check_ranks(oracle, a, b, mode, wide_a[:, 3:20], cols_b)
    check_ranks(oracle, a[::2], b[::2], mode, wide_a[::2, 3:20], cols_b[::2])
    check_ranks(oracle, a, b, mode, torch.from_numpy(a).to(DEV).double(), torch.from_numpy(b).to(DEV))


@pytest.mark.parametrize("mode", MODES)
def test_both_rank_layouts_equal_the_truth(oracle, mode):
    """Layout 1 (A and B rows in LDS) and layout 2 (A rows in registers, B as 16-byte LDS broadcasts) against the same truth,
    on every column class of the register kernel and on both sides of each class boundary."""
    try:
        for layout in (1, 2):
            R().set_rank_layout(layout)
            for n, d1 in ((65, 8), (200, 9), (130, 16), (700, 17), (300, 33), (129, 34), (1000, 65), (257, 66), (300, 100),
                          (513, 128), (1000, 129)):
                rs = np.random.RandomState(77 * n + d1)
                a, b = RC.special_pairs(rs, n, d1 - 1, scale=0.5 if d1 > 9 else 1.0, noise=0.7)
                check_ranks(oracle, a, b, mode)
    finally:
        R().set_rank_layout(0)
    with pytest.raises(Exception):
        R().set_rank_layout(3)


@pytest.mark.parametrize("mode", MODES)
def test_both_rank_layouts_on_one_partial_block_and_on_strided_inputs(oracle, mode):
    """A single block with dead owner rows (n = 1, 63) in every column class of the register layout; layout 2 asked of rows
    narrower than 9 columns (they take the LDS layout); the strided and column-major inputs under both layouts."""
    try:
        for layout in (1, 2):
            R().set_rank_layout(layout)
            for n, d1 in ((1, 9), (63, 9), (1, 33), (63, 33), (1, 129), (63, 129), (64, 8)):
                rs = np.random.RandomState(91 * n + d1)
                a, b = RC.special_pairs(rs, n, d1 - 1, scale=0.5 if d1 > 9 else 1.0, noise=0.7)
                check_ranks(oracle, a, b, mode)
            test_ranks_of_non_contiguous_inputs(oracle, mode)
    finally:
        R().set_rank_layout(0)


# ---- 3. k-NN -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_knn_equals_the_truth(oracle, mode):
    rs = np.random.RandomState(11)
    q = RC.points(rs, 70, 32, 0.5)
    keys = RC.points(rs, 333, 32, 0.5)
    keys[100] = keys[7]; keys[200] = keys[7]; keys[201] = keys[8]                                # duplicated key rows
    keys[50, 4] = np.nan                                                                         # a NaN key row
    q[3] = keys[7]                                                                               # distance 0 to three keys
    for k in (1, 10, 100, 128):
        for c in (0.5, 1.0, 2.0):
            check_knn(oracle, q, keys, k, c, mode)
    check_knn(oracle, q, keys[:50], 50, 1.0, mode)                                               # k = N
    table = RC.points(rs, 200, 8, 1.0)
    table[150] = table[20]
    for k in (1, 10, 100, 128):
        idx = check_knn(oracle, table, table, k, 1.0, mode, exclude_self=True)
        assert not (idx == np.arange(200)[:, None]).any()
    check_knn(oracle, table, table, 10, 0.5, mode, exclude_self=False)
    check_knn(oracle, table[:65], table[:129], 128, 1.0, mode, exclude_self=True)                # k = N - 1 selectable


@pytest.mark.parametrize("mode", MODES)
def test_knn_at_the_largest_lds_configuration_and_on_strided_inputs(oracle, mode):
    rs = np.random.RandomState(13)
    q = RC.points(rs, 150, 128, 0.3)                                                             # d1 = 129, Q > 64
    keys = RC.points(rs, 400, 128, 0.3)
    keys[300] = keys[5]
    keys[9, 77] = np.nan
    check_knn(oracle, q, keys, 128, 1.0, mode)                                                   # k = 128: 148 736 B of dynamic LDS
    check_knn(oracle, q, keys, 127, 2.0, mode)
    q2, k2 = RC.points(rs, 90, 99, 0.3), RC.points(rs, 260, 99, 0.3)                             # d1 = 100
    check_knn(oracle, q2, k2, 100, 0.5, mode)
    wide = torch.full((260, 140), 3.0, device=DEV)                                               # row stride 140 > d1
    wide[:, 20:120] = torch.from_numpy(k2).to(DEV)
    cols = torch.from_numpy(np.ascontiguousarray(q2.T)).to(DEV).t()                              # column-major queries
    assert not wide[:, 20:120].is_contiguous() and not cols.is_contiguous()
    D = oracle.batch_distance(q2, k2, 1.0, RC.SIGN_MODE[mode])
    want_d, want_i = RC.knn_truth(D, 10)
    got_d, got_i = R().hyperbolic_knn(cols, wide[:, 20:120], 10, sign_convention=mode)
    assert np.array_equal(got_i.cpu().numpy(), want_i) and np.array_equal(bits(got_d.cpu().numpy()), bits(want_d))
    want_d, want_i = RC.knn_truth(D[::2, ::2], 10)
    got_d, got_i = R().hyperbolic_knn(cols[::2], wide[::2, 20:120], 10, sign_convention=mode)
    assert np.array_equal(got_i.cpu().numpy(), want_i) and np.array_equal(bits(got_d.cpu().numpy()), bits(want_d))


@pytest.mark.parametrize("mode", MODES)
def test_knn_pads_rows_with_too_few_selectable_keys(oracle, mode):
    rs = np.random.RandomState(12)
    q = RC.points(rs, 66, 5, 1.0)
    keys = RC.points(rs, 40, 5, 1.0)
    keys[5:33, 2] = np.nan                                                                       # 12 selectable keys
    q[64, 1] = np.nan                                                                            # a query with none
    idx = check_knn(oracle, q, keys, 20, 1.0, mode)
    assert (idx[0, 12:] == -1).all() and (idx[0, :12] >= 0).all() and (idx[64] == -1).all()
    idx = check_knn(oracle, keys, keys, 40, 2.0, mode, exclude_self=True)                        # k = N with the own row skipped
    assert (idx[:, -1] == -1).all()


# ---- 4. full size: against this repository's own batch_distance, in slabs ---------------------------------------------
def test_full_size_ranks_knn_memory_and_determinism():
    from hyptokenizer_amd.embedding import lorentz_model as LM
    B, d1, k, slab = 16384, 65, 10, 1024
    a, b = RC.pairs(np.random.RandomState(2024), B, d1 - 1, 0.3, 0.7)
    ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    R().retrieval_ranks(ta[:64], tb[:64], sign_convention="lorentz")                             # warm-up
    R().hyperbolic_knn(ta[:64], tb[:64], k, sign_convention="lorentz")
    torch.cuda.synchronize()
    limit = 16 * B * d1 * 4

    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    rank_r, rank_c = R().retrieval_ranks(ta, tb, sign_convention="lorentz")
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base
    print(f"ranks: peak extra bytes {extra} (limit {limit}, one B x B fp32 matrix {B * B * 4})")
    assert extra < limit

    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    knn_d, knn_i = R().hyperbolic_knn(ta, tb, k, sign_convention="lorentz")
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base
    print(f"knn: peak extra bytes {extra} (limit {limit + B * k * 12})")
    assert extra < limit + B * k * 12

    again_r, again_c = R().retrieval_ranks(ta, tb, sign_convention="lorentz")
    again_d, again_i = R().hyperbolic_knn(ta, tb, k, sign_convention="lorentz")
    assert torch.equal(rank_r, again_r) and torch.equal(rank_c, again_c) and torch.equal(knn_i, again_i)
    assert torch.equal(knn_d.view(torch.int32), again_d.view(torch.int32))

    allj = torch.arange(B, device=DEV)
    for s in range(0, B, slab):
        own = allj[s:s + slab]
        D = LM.batch_distance(ta[s:s + slab], tb, 1.0, sign_convention="lorentz")                # rows s .. s + slab
        diag = D[torch.arange(slab, device=DEV), own]
        want = (D < diag[:, None]).sum(1) + ((D == diag[:, None]) & (allj[None, :] < own[:, None])).sum(1)
        assert torch.equal(rank_r[s:s + slab].long(), want), s
        sd, si = torch.sort(D, dim=1, stable=True)
        assert torch.equal(knn_i[s:s + slab], si[:, :k]), s
        assert torch.equal(knn_d[s:s + slab].view(torch.int32), sd[:, :k].contiguous().view(torch.int32)), s
        D = LM.batch_distance(ta, tb[s:s + slab], 1.0, sign_convention="lorentz")                # columns s .. s + slab
        diag = D[own, torch.arange(slab, device=DEV)]
        want = (D < diag[None, :]).sum(0) + ((D == diag[None, :]) & (allj[:, None] < own[None, :])).sum(0)
        assert torch.equal(rank_c[s:s + slab].long(), want), s
    r1 = float((rank_r < 1).sum()) / B
    print(f"R@1 text2image at B = {B}: {r1}")
    assert 0.0 < r1 < 1.0


@pytest.mark.parametrize("mode", MODES)
def test_small_calls_are_deterministic(mode):
    rs = np.random.RandomState(3)
    a, b = RC.special_pairs(rs, 1000, 32)
    ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    r0 = R().retrieval_ranks(ta, tb, sign_convention=mode)
    r1 = R().retrieval_ranks(ta, tb, sign_convention=mode)
    assert torch.equal(r0[0], r1[0]) and torch.equal(r0[1], r1[1])
    k0 = R().hyperbolic_knn(ta, tb, 100, 2.0, sign_convention=mode, exclude_self=True)
    k1 = R().hyperbolic_knn(ta, tb, 100, 2.0, sign_convention=mode, exclude_self=True)
    assert torch.equal(k0[1], k1[1]) and torch.equal(k0[0].view(torch.int32), k1[0].view(torch.int32))
    assert R().compute_recall_at_k(ta, tb, [1, 5], sign_convention=mode) == R().compute_recall_at_k(ta, tb, [1, 5], sign_convention=mode)
