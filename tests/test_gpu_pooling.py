"""Lorentz-centroid pooling on the GPU (csrc/hm_pool.hip, hyptokenizer_amd.embedding.pooling, BatchEncoder.encode_device,
HyperbolicTokenizer.embed_batch) against the float64 truth of tests/pooling_cases.py.

Bound of every comparison with the truth (the rule of test_gpu_autograd.py, set by the feature's specification, not tuned):
with e_ref the error of the same expression run by torch in fp32 on the CPU against the float64 truth and e_hip ours, both the
largest absolute error of an array relative to the array's largest magnitude, ``e_hip <= 4 * e_ref + 2**-20``.  Each case
prints ``name e_ref e_hip`` before it asserts (run with -s to collect the table of DESIGN.md 5.18).  Every case has at most
257 bags and fewer than 4 000 positions.
"""
import os

import numpy as np
import pytest
import torch

import pooling_cases as PC
import riemannian_cases as RC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILL = 777.0


def P():
    from hyptokenizer_amd.embedding import pooling
    return pooling


def leaf(x: torch.Tensor, pad: int = 0, shift: bool = False) -> torch.Tensor:
    """A leaf on the device holding ``x``: contiguous, or a view with leading dimension ``x.shape[1] + pad`` over FILL whose
    base pointer, with ``shift``, is 4 bytes past a 16-byte boundary."""
    if pad == 0 and not shift:
        return x.to(DEV).clone().requires_grad_(True)
    v, ld = x.shape[0], x.shape[1] + pad
    buf = torch.full((v * ld + 1,), FILL, device=DEV)
    view = buf[int(shift):int(shift) + v * ld].view(v, ld)[:, :x.shape[1]]
    view.copy_(x.to(DEV))
    assert view.data_ptr() % 16 == (4 if shift else 0)
    return view.detach().requires_grad_(True)


def dev(t):
    return None if t is None else t.to(DEV)


def hip_eval(x, ids, offsets, lengths, weights, g, pad=0, shift=False, sparse_grad=True):
    """((mu, dense table gradient, weight gradient | None) as numpy, raw table gradient) of sum(g * mu) through the Python layer.
    The sparse gradient is densified by ``coalesce().to_dense()``: a sort and a segmented sum, where ``to_dense()`` alone adds
    repeated indices with atomics in any order."""
    t = leaf(x, pad, shift)
    w = None if weights is None else weights.to(DEV).clone().requires_grad_(True)
    mu = P().lorentz_centroid(t, dev(ids), dev(offsets), dev(lengths), w, sparse_grad=sparse_grad)
    (mu * g.to(DEV)).sum().backward()
    assert t.grad.is_sparse == sparse_grad
    dense = t.grad.coalesce().to_dense() if sparse_grad else t.grad
    return (mu.detach().cpu().numpy(), dense.cpu().numpy(), None if w is None else w.grad.cpu().numpy()), t.grad


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(params=[0, 1], ids=["group_per_segment", "wave_per_segment"])
def form(request):
    """Both work decompositions of the pooling kernels (hm_debug_centroid_form); the default, -1 (chosen per call), is
    restored afterwards."""
    from hyptokenizer_amd import _lib
    L = _lib.load()
    _lib.check(L.hm_debug_centroid_form(request.param))
    yield request.param
    _lib.check(L.hm_debug_centroid_form(-1))


VARIANTS = ((True, True), (True, False), (False, True), (False, False))          # (lengths, weights)


# ---- 1. centroid and gradients against the truth ---------------------------------------------------------------------------------
@pytest.mark.parametrize("d1", PC.WIDTHS)
def test_centroid_and_gradients_every_batch_and_variant(d1, form):
    failures = []
    for n in PC.BATCHES:
        for use_lengths, use_weights in VARIANTS:
            truth, ref32 = PC.reference(d1, n, use_lengths, use_weights)
            ours, _ = hip_eval(PC.table(d1), *PC.variant(n, use_lengths, use_weights), PC.upstream(n, d1))
            PC.compare(f"f{form}_w{d1}_n{n}_l{int(use_lengths)}_w{int(use_weights)}", truth, ref32, ours, failures)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("d1", PC.WIDTHS)
def test_padded_leading_dimensions_and_unaligned_base(d1, form):
    """Leading dimensions d1 + 1, + 2, + 3 and a base pointer 4 bytes past a 16-byte boundary, on the tables without rows near
    the origin."""
    failures = []
    for pad, shift, n, use_lengths, use_weights in ((1, False, 37, True, True), (2, False, 37, False, True), (3, True, 257, True, False),
                                                    (0, True, 37, True, True)):
        truth, ref32 = PC.reference(d1, n, use_lengths, use_weights, PC.WELL)
        ours, _ = hip_eval(PC.table(d1, scales=PC.WELL), *PC.variant(n, use_lengths, use_weights), PC.upstream(n, d1), pad=pad, shift=shift)
        PC.compare(f"f{form}_well_w{d1}_ld{d1 + pad}_s{int(shift)}_n{n}", truth, ref32, ours, failures)
    assert not failures, "\n".join(failures)


# ---- 2. the centroids lie on the hyperboloid --------------------------------------------------------------------------------------
def test_hyperboloid_defect(form):
    """|mu0^2 - |mu_s|^2 - 1|, largest over the bags, against the same figure of the fp32 CPU reference under the same rule."""
    failures = []
    for d1 in PC.WIDTHS:
        for n in PC.BATCHES[1:]:
            _, ref32 = PC.reference(d1, n, True, True)
            ids, offsets, lengths, weights = PC.variant(n, True, True)
            with torch.no_grad():
                mu = P().lorentz_centroid(PC.table(d1).to(DEV), dev(ids), dev(offsets), dev(lengths), dev(weights)).cpu().numpy()
            e_ref, e_hip = float(PC.defect(ref32[0]).max()), float(PC.defect(mu).max())
            print(f"f{form}_w{d1}_n{n}:defect e_ref={e_ref:.3e} e_hip={e_hip:.3e}")
            if not e_hip <= PC.FACTOR * e_ref + PC.FLOOR:
                failures.append(f"w{d1}_n{n}: e_ref={e_ref:.3e} e_hip={e_hip:.3e}")
    assert not failures, "\n".join(failures)


# ---- 3. bits -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d1", [5, 66])
def test_bit_identities(d1, form):
    n = 257
    x, g = PC.table(d1), PC.upstream(n, d1)
    ids, offsets, lengths, weights = PC.bags(n)
    (mu1, gx1, gw1), raw1 = hip_eval(x, ids, offsets, lengths, weights, g)
    (mu2, gx2, gw2), raw2 = hip_eval(x, ids, offsets, lengths, weights, g)
    # two calls
    assert np.array_equal(bits(mu1), bits(mu2)) and np.array_equal(bits(gw1), bits(gw2))
    assert torch.equal(raw1._values().view(torch.int32), raw2._values().view(torch.int32)) and torch.equal(raw1._indices(), raw2._indices())
    assert raw1._values().shape == (ids.numel(), d1) and not raw1.is_coalesced()
    # no weights == weights of ones
    (mu_n, _, _), raw_n = hip_eval(x, ids, offsets, lengths, None, g)
    (mu_o, _, _), raw_o = hip_eval(x, ids, offsets, lengths, torch.ones_like(weights), g)
    assert np.array_equal(bits(mu_n), bits(mu_o)) and torch.equal(raw_n._values().view(torch.int32), raw_o._values().view(torch.int32))
    # weights scaled by 2: s doubles, q quadruples, nu doubles, all exactly
    (mu_2, _, _), _ = hip_eval(x, ids, offsets, lengths, 2 * weights, g)
    assert np.array_equal(bits(mu_2), bits(mu1))
    # the slab with lengths == the compacted form without
    cids, coff, cw = PC.compact(ids, offsets, lengths, weights)
    (mu_c, gx_c, gw_c), raw_c = hip_eval(x, cids, coff, None, cw, g)
    keep = (PC.segment_of(ids.numel(), offsets, lengths) >= 0).numpy()
    assert np.array_equal(bits(mu_c), bits(mu1)) and np.array_equal(bits(gw_c), bits(gw1[keep])) and not gw1[~keep].any()
    assert np.array_equal(bits(raw_c._values().cpu().numpy()), bits(raw1._values().cpu().numpy()[keep]))
    assert np.array_equal(raw_c._indices().cpu().numpy()[0], raw1._indices().cpu().numpy()[0][keep])
    # sparse_grad=True densified == sparse_grad=False
    (_, gx_d, _), _ = hip_eval(x, ids, offsets, lengths, weights, g, sparse_grad=False)
    assert np.array_equal(bits(gx_d), bits(gx1))


def test_the_two_forms_agree_to_rounding():
    from hyptokenizer_amd import _lib
    L = _lib.load()
    d1, n = 66, 257
    x, g = PC.table(d1, scales=PC.WELL), PC.upstream(n, d1)
    out = []
    try:
        for f in (0, 1):
            _lib.check(L.hm_debug_centroid_form(f))
            (mu, _, gw), raw = hip_eval(x, *PC.bags(n), g)
            out.append((mu, raw._values().cpu().numpy(), raw._indices().cpu().numpy(), gw))
    finally:
        _lib.check(L.hm_debug_centroid_form(-1))
    (m0, v0, i0, w0), (m1, v1, i1, w1) = out
    assert np.array_equal(i0, i1) and np.array_equal(v0.any(axis=1), v1.any(axis=1))
    # another order of a sum of at most 70 rows of magnitude <= max |x|: relative to the largest entry, 2^-20 leaves room for
    # 16 ulps
    assert np.abs(m0 - m1).max() <= 2.0 ** -20 * np.abs(m0).max() and np.abs(v0 - v1).max() <= 2.0 ** -20 * np.abs(v0).max()


# ---- 4. degenerate segments, skipped positions ---------------------------------------------------------------------------------
@pytest.mark.parametrize("d1", [2, 17, 66])
def test_degenerate_segments_and_nan_rows(d1, form):
    x = PC.table(d1).clone()
    x[11] = float("nan")
    ids = torch.tensor([-1, 40, 2, 3, 11, 5, 6, 7, 6])
    #                        empty  masked  zero-weight  NaN row  plain
    offsets = torch.tensor([0, 0, 2, 4, 6, 9])
    w = torch.tensor([1.0, 1.0, 0.0, 0.0, 1.0, 1.0, 1.0, 0.5, 2.0])
    g = PC.upstream(5, d1)
    (mu, gx, gw), raw = hip_eval(x, ids, offsets, None, w, g)
    origin = np.zeros(d1, np.float32)
    origin[0] = 1
    assert all(np.array_equal(bits(mu[i]), bits(origin)) for i in range(4))
    val, coo = raw._values().cpu().numpy(), raw._indices().cpu().numpy()[0]
    assert not val[:6].any() and not gw[:6].any() and val[6:].any(axis=1).all() and np.isfinite(val).all()
    assert coo.tolist() == [0, 0, 2, 3, 11, 5, 6, 7, 6]
    # the NaN row poisons only its own segment: the plain one is the truth's
    truth, ref32 = (PC.evaluate(x, ids, offsets, None, w, g, dt) for dt in (torch.float64, torch.float32))
    failures = []
    PC.compare(f"f{form}_degenerate_w{d1}", truth, ref32, (mu, gx, gw), failures)
    assert not failures, "\n".join(failures)


def test_no_segments_and_no_tokens(form):
    x = PC.table(5)
    ids, _, _, weights = PC.bags(3)
    (mu, gx, gw), raw = hip_eval(x, ids, torch.zeros(1, dtype=torch.int64), None, weights, torch.zeros(0, 5))        # n = 0
    assert mu.shape == (0, 5) and not gx.any() and not gw.any()
    assert raw._values().shape == (ids.numel(), 5) and not raw._values().any() and not raw._indices().any()
    empty = torch.zeros(0, dtype=torch.int64)
    (mu, gx, gw), raw = hip_eval(x, empty, torch.zeros(4, dtype=torch.int64), torch.zeros(3, dtype=torch.int32), torch.zeros(0),
                                 PC.upstream(3, 5))                                                                   # T = 0
    assert mu.shape == (3, 5) and (mu[:, 0] == 1).all() and not mu[:, 1:].any() and not gx.any() and raw._values().shape == (0, 5)


@pytest.mark.parametrize("d1", [5, 129])
def test_every_position_is_written_once_under_a_filled_buffer(d1, form):
    """The C entry points on buffers pre-filled with FILL: T entries, indices in [0, V), zero rows exactly at the skipped
    positions -- slack, ids out of range, and the positions before offsets[0] and behind offsets[n]."""
    from hyptokenizer_amd import _lib
    L = _lib.load()
    n = 37
    ids0, off0, lengths, w0 = PC.bags(n)
    head, tail = 3, 5
    ids = torch.cat([torch.arange(head), ids0, torch.arange(tail)])
    ids[head + int(off0[7])] = PC.V                             # one past the end, in the bag of 70
    w = torch.cat([torch.ones(head), w0, torch.ones(tail)])
    offsets = off0 + head
    t = ids.numel()
    x, g = PC.table(d1).to(DEV), PC.upstream(n, d1).to(DEV)
    ids_d, off_d, len_d, w_d = ids.to(DEV), offsets.to(DEV), lengths.to(DEV), w.to(DEV)
    mu = torch.full((n, d1), FILL, device=DEV)
    inv = torch.full((n,), FILL, device=DEV)
    val = torch.full((t, d1), FILL, device=DEV)
    gw = torch.full((t,), FILL, device=DEV)
    coo = torch.full((t,), -7, dtype=torch.int64, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    _lib.check(L.hm_centroid_fwd(x.data_ptr(), d1, PC.V, d1, ids_d.data_ptr(), t, off_d.data_ptr(), len_d.data_ptr(), w_d.data_ptr(), n,
                                 mu.data_ptr(), inv.data_ptr(), stream))
    _lib.check(L.hm_centroid_bwd(x.data_ptr(), d1, PC.V, d1, ids_d.data_ptr(), t, off_d.data_ptr(), len_d.data_ptr(), w_d.data_ptr(), n,
                                 mu.data_ptr(), inv.data_ptr(), g.data_ptr(), val.data_ptr(), coo.data_ptr(), gw.data_ptr(), stream))
    torch.cuda.synchronize()
    mu, inv, val, gw, coo = (a.cpu().numpy() for a in (mu, inv, val, gw, coo))
    assert not (mu == FILL).any() and not (inv == FILL).any() and not (val == FILL).any() and not (gw == FILL).any()
    assert coo.min() >= 0 and coo.max() < PC.V
    seg = PC.segment_of(t, offsets, lengths).numpy()
    live = (seg >= 0) & (ids.numpy() >= 0) & (ids.numpy() < PC.V)
    assert live.sum() < t - head - tail and not live[:head].any() and not live[t - tail:].any()
    assert not val[~live].any() and not gw[~live].any() and not coo[~live].any()
    assert val[live].any(axis=1).all() and np.array_equal(coo[live], ids.numpy()[live])
    assert (inv[lengths.numpy() == 0] == 0).all() and (inv[lengths.numpy() > 0] > 0).all()


def test_backward_allocates_nothing_of_the_tables_size():
    """The gradient is T value rows and T indices, whatever V: forward + backward over a 2^18-row table stay below a
    quarter of the table's bytes above the inputs (a dense [V, d1] gradient alone would be all of them)."""
    v, d1 = 1 << 18, 17
    table = P().init_table(v, d1 - 1, 0.1, 0, DEV).requires_grad_(True)
    ids, offsets, lengths, weights = (t.to(DEV) for t in PC.bags(37))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    P().lorentz_centroid(table, ids, offsets, lengths, weights).sum().backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    assert table.grad.is_sparse and table.grad._nnz() == ids.numel()
    assert peak < v * d1 * 4 // 4, peak


# ---- 5. composition: pooled bags -> InfoNCE -> Riemannian SGD ----------------------------------------------------------------------
def test_contrastive_training_on_pooled_bags():
    """Two sets of 32 bags over a 60-row table of width 6 (PC.E2E), 30 steps of RiemannianSGD on the hyperbolic InfoNCE between
    their centroids.  The same loop in float64 on the CPU (truth pooling, autograd_cases.infonce, riemannian_cases.sgd_step;
    test_pooling_host.py runs it and checks that it descends step by step) takes the loss from 3.162030 to 1.127057.
    Trajectories diverge by rounding, so only the size of the decrease is comparable: the GPU run must lose at least half of
    2.034973, i.e. 1.017487."""
    from hyptokenizer_amd import optim
    from hyptokenizer_amd.multimodal.contrastive_loss import hyperbolic_contrastive_loss
    e = PC.E2E
    x, a, b = PC.e2e_inputs()
    p = torch.nn.Parameter(x.to(DEV))
    a, b = tuple(t.to(DEV) for t in a), tuple(t.to(DEV) for t in b)
    opt = optim.RiemannianSGD([p], lr=e["lr"])

    def loss_of():
        return hyperbolic_contrastive_loss(P().lorentz_centroid(p, *a), P().lorentz_centroid(p, *b), temp=e["temp"],
                                           sign_convention="lorentz")

    before = float(loss_of().detach())
    for _ in range(e["steps"]):
        opt.zero_grad(set_to_none=True)
        loss_of().backward()
        assert p.grad.is_sparse
        opt.step()
    after = float(loss_of().detach())
    b64, a64 = PC.E2E_FLOAT64
    print(f"e2e: loss {before:.6f} -> {after:.6f} (float64 {b64:.6f} -> {a64:.6f})")
    assert abs(before - b64) <= 1e-4
    assert before - after >= 0.5 * (b64 - a64)
    # every row ends on the hyperboloid: the tolerance and the reasoning of test_gpu_graph_embedding.py's end-to-end test (the
    # step recomputes x0 = sqrt(1 + |xs|^2) from 5 squares in fp32)
    xd = p.detach().double().cpu()
    assert float(((RC.ldot(xd, xd) + 1).abs() / xd[:, 0] ** 2).max()) <= 8 * 2.0 ** -24


def test_embedding_bag_steps_under_riemannian_adam():
    from hyptokenizer_amd import optim
    bag = P().HyperbolicEmbeddingBag(PC.V, 16, init_scale=0.1, seed=4, device=DEV)
    ids, offsets, lengths, weights = (t.to(DEV) for t in PC.bags(37))
    ids = torch.where(ids < 30, ids, torch.full_like(ids, -1))                   # rows 30.. are never named
    opt = optim.RiemannianAdam(bag.parameters(), lr=0.05)
    start = bag.weight.detach().clone()
    out = bag(ids, offsets, lengths, per_sample_weights=weights)
    assert out.shape == (37, 17)
    (out[:, 1:] ** 2).sum().backward()
    assert bag.weight.grad.is_sparse and bag.weight.grad._nnz() == ids.numel()
    opt.step()
    moved = (bag.weight.detach() != start).any(dim=1).cpu().numpy()
    assert not moved[30:].any() and moved[:30].sum() >= 25
    xd = bag.weight.detach().double().cpu()
    assert float(((RC.ldot(xd, xd) + 1).abs() / xd[:, 0] ** 2).max()) <= 2.0 ** -20


# ---- 6. the tokenizer ------------------------------------------------------------------------------------------------------------
def test_tokenizer_encode_device_and_embed_batch(golden_dir):
    from hyptokenizer_amd.tokenizer.hyperbolic_merge import HyperbolicTokenizer
    tok = HyperbolicTokenizer.load(os.path.join(golden_dir, "g7_saved_lorentz", "std"), device=torch.device(DEV), sign_convention="lorentz")
    v = tok.vocab
    texts = ["丗丣丗丗丣" + v[0] + v[1], "", "xyz ?!", "丗丗丣丗丣丗丗丣" + v[9] + "q" + v[10],
             v[5] * 7, "丗丣" * 40]
    enc = tok._batch_encoder()
    ids, offsets, lengths = enc.encode_device(texts)
    assert ids.dtype == torch.int64 and offsets.dtype == torch.int64 and lengths.dtype == torch.int32 and ids.is_cuda
    want = tok.encode_batch(texts)
    assert want == [tok.encode(t) for t in texts]
    ids_h, off_h, len_h = ids.cpu().tolist(), offsets.cpu().tolist(), lengths.cpu().tolist()
    assert off_h == np.concatenate([[0], np.cumsum([len(t) for t in texts])]).tolist() and len_h == [len(w) for w in want]
    for k, w in enumerate(want):
        assert ids_h[off_h[k]:off_h[k] + len_h[k]] == w
        assert all(i == -1 for i in ids_h[off_h[k] + len_h[k]:off_h[k + 1]])
    assert len_h[1] == 0 and want[2] == [tok.token2idx.get("<unk>", 3)] * len(texts[2]) and len_h[5] < len(texts[5])
    e_ids, e_off, e_len = enc.encode_device([])
    assert e_ids.numel() == 0 and e_off.tolist() == [0] and e_len.numel() == 0
    # embed_batch == the centroid over the compacted host arrays, bit for bit
    got = tok.embed_batch(texts)
    flat, off = enc.encode_arrays(texts)
    table = tok.embeddings.data[:tok.current_vocab_size]
    ref = P().lorentz_centroid(table, torch.from_numpy(flat).to(DEV), torch.from_numpy(off).to(DEV))
    assert got.shape == (len(texts), table.shape[1]) and torch.equal(got.detach().view(torch.int32), ref.view(torch.int32))
    assert got[1].tolist() == [1.0] + [0.0] * (table.shape[1] - 1)
    got.sum().backward()
    assert tok.embeddings.grad.is_sparse and tok.embeddings.grad.shape == tok.embeddings.shape
    w = torch.rand(ids.numel(), device=DEV) + 0.5
    wref = P().lorentz_centroid(table, ids, offsets, lengths, w)
    assert torch.equal(tok.embed_batch(texts, weights=w).detach().view(torch.int32), wref.view(torch.int32))
