"""Lorentz-centroid pooling, the part that needs no GPU: the module and its entry points exist and refuse bad arguments before a
device is touched, the Python layer raises what it documents, and the truth of tests/pooling_cases.py agrees with the closed
form of DESIGN.md 5.18 and follows the degenerate rule."""
import ctypes as C

import numpy as np
import pytest
import torch

import pooling_cases as PC

SYMBOLS = ("hm_centroid_fwd", "hm_centroid_bwd", "hm_debug_centroid_form")


def P():
    from hyptokenizer_amd.embedding import pooling
    return pooling


# ---- 1. the entry points ----------------------------------------------------------------------------------------------------
def test_module_and_symbols_exist():
    from hyptokenizer_amd import _lib, embedding
    assert embedding.lorentz_centroid is P().lorentz_centroid and embedding.HyperbolicEmbeddingBag is P().HyperbolicEmbeddingBag
    L = _lib.load()
    for name in SYMBOLS:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(L, name), name
    from hyptokenizer_amd.tokenizer.batch_encoder import BatchEncoder
    from hyptokenizer_amd.tokenizer.hyperbolic_merge import HyperbolicTokenizer
    assert callable(BatchEncoder.encode_device) and callable(HyperbolicTokenizer.embed_batch)


def test_argument_errors_come_back_without_a_device():
    """Non-NULL pointers are addresses of host buffers: a call that got past its argument check would fault on them or fail on
    the missing device, it would not return HM_E_ARG."""
    from hyptokenizer_amd import _lib
    L = _lib.load()
    buf = np.zeros(1024, np.int64)
    p = C.c_void_p(buf.ctypes.data)

    def fwd(x=p, ld=6, v=10, d1=6, ids=p, t=4, off=p, n=2):
        return L.hm_centroid_fwd(x, ld, v, d1, ids, t, off, None, None, n, p, p, None)

    def bwd(x=p, ld=6, v=10, d1=6, ids=p, t=4, off=p, n=2):
        return L.hm_centroid_bwd(x, ld, v, d1, ids, t, off, None, None, n, p, p, p, p, p, None, None)

    for call in (fwd, bwd):
        assert call(x=None) == _lib.HM_E_ARG                    # null table
        assert call(d1=1, ld=6) == _lib.HM_E_ARG                # d1 outside 2..129
        assert call(d1=130, ld=130) == _lib.HM_E_ARG
        assert call(ld=5) == _lib.HM_E_ARG                      # ld < d1
        assert call(n=-1) == _lib.HM_E_ARG                      # negative n
        assert call(off=None) == _lib.HM_E_ARG                  # null offsets with n > 0
        assert call(ids=None) == _lib.HM_E_ARG                  # null ids with t > 0
        assert L.hm_last_error(None)
    assert fwd(n=0, off=None) == _lib.HM_OK                     # no segment: nothing to launch
    assert L.hm_debug_centroid_form(2) == _lib.HM_E_ARG and L.hm_debug_centroid_form(-2) == _lib.HM_E_ARG
    assert L.hm_debug_centroid_form(-1) == _lib.HM_OK


def _cpu_case():
    x = PC.table(5)
    ids, offsets, lengths, weights = PC.bags(3)
    return x, ids, offsets, lengths, weights


def test_cpu_tensors_raise_unavailable():
    from hyptokenizer_amd.engine import HypMergeUnavailable
    x, ids, offsets, lengths, weights = _cpu_case()
    for validate in (True, False):
        with pytest.raises(HypMergeUnavailable):
            P().lorentz_centroid(x, ids, offsets, lengths, weights, validate=validate)
    if not torch.cuda.is_available():
        bag = P().HyperbolicEmbeddingBag(10, 4, device="cpu")
        assert bag.weight.shape == (10, 5) and float(PC.ldot(bag.weight.detach().double(), bag.weight.detach().double()).add(1).abs().max()) < 1e-6
        with pytest.raises(HypMergeUnavailable):
            bag(ids.clamp(0, 9), offsets)


def test_bad_arguments_raise_value_error():
    x, ids, offsets, lengths, weights = _cpu_case()
    f = P().lorentz_centroid
    with pytest.raises(ValueError):
        f(x, ids, offsets, sign_convention="reference")
    with pytest.raises(ValueError):
        f(x.double(), ids, offsets)
    with pytest.raises(ValueError):
        f(x, ids.int(), offsets)
    with pytest.raises(ValueError):
        f(x, ids, offsets.int())
    with pytest.raises(ValueError):
        f(x, ids, offsets, lengths.long())
    with pytest.raises(ValueError):
        f(x, ids, offsets, lengths, weights.double())
    with pytest.raises(ValueError):
        f(x, ids, offsets, lengths[:-1])                        # shapes
    with pytest.raises(ValueError):
        f(x, ids, offsets, lengths, weights[:-1])
    with pytest.raises(ValueError):
        f(x[:, :1], ids, offsets)
    with pytest.raises(ValueError):
        f(x.t().contiguous().t(), ids, offsets)                 # no unit stride in the last dimension
    with pytest.raises(ValueError):
        f(x, ids, torch.tensor([0, 2, 1, 3]))                   # decreasing offsets
    with pytest.raises(ValueError):
        f(x, ids, torch.tensor([-1, 1, 2, 3]))
    with pytest.raises(ValueError):
        f(x, ids, torch.tensor([0, 1, 2, ids.numel() + 1]))
    with pytest.raises(ValueError):
        f(x, ids, offsets, lengths + 1)                         # lengths beyond the span
    with pytest.raises(ValueError):
        f(x, ids, offsets, lengths - 1)
    with pytest.raises(ValueError):
        P().HyperbolicEmbeddingBag(10, 129, device="cpu")


def test_embed_batch_needs_the_lorentz_convention():
    from helpers import OracleEngine
    from hyptokenizer_amd.tokenizer.hyperbolic_merge import HyperbolicTokenizer
    tok = HyperbolicTokenizer(["a", "b"], torch.nn.Parameter(PC.table(5)[:2].clone()), device=torch.device("cpu"), max_vocab_size=8,
                              sign_convention="reference", engine=OracleEngine(8, 5, "reference"))
    with pytest.raises(ValueError):
        tok.embed_batch(["ab"])


# ---- 2. the truth itself ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d1,n,use_lengths,use_weights", [(2, 3, True, True), (5, 37, True, False), (17, 37, False, True),
                                                           (66, 3, False, False), (129, 257, True, True)])
def test_autograd_gradient_of_the_truth_is_the_closed_form(d1, n, use_lengths, use_weights):
    x, g = PC.table(d1), PC.upstream(n, d1)
    ids, offsets, lengths, weights = PC.variant(n, use_lengths, use_weights)
    mu, gx, gw = PC.evaluate(x, ids, offsets, lengths, weights, g, torch.float64)
    cx, cw = PC.closed_form(x.double(), ids, offsets, lengths, weights, g.double())
    assert np.abs(cx.numpy() - gx).max() <= 1e-10 * np.abs(gx).max()
    if use_weights:
        assert np.abs(cw.numpy() - gw).max() <= 1e-10 * np.abs(gw).max()
    live = offsets[1:] > offsets[:-1] if lengths is None else lengths > 0
    assert PC.defect(mu)[live.numpy()].max() <= 1e-10           # points of the hyperboloid


def test_definition_on_a_case_written_out_by_hand():
    x = PC.table(5).double()
    ids = torch.tensor([3, 7, -1, 7, 40, 9, 1])
    offsets, lengths = torch.tensor([0, 5, 7]), torch.tensor([5, 1], dtype=torch.int32)
    w = torch.tensor([0.5, 1.0, 9.0, 2.0, 9.0, 1.0, 9.0], dtype=torch.float64)
    mu, ok = PC.centroid(x, ids, offsets, lengths, w)
    s = 0.5 * x[3] + 3.0 * x[7]
    want0 = s / torch.sqrt(s[0] ** 2 - (s[1:] ** 2).sum())
    assert ok.tolist() == [True, True] and torch.allclose(mu[0], want0, rtol=0, atol=1e-14)
    assert torch.allclose(mu[1], x[9] / torch.sqrt(-PC.ldot(x[9], x[9])), rtol=0, atol=1e-14)      # one token: the row, renormalised
    mu2, _ = PC.centroid(x, ids, offsets, lengths, 2 * w)
    assert torch.allclose(mu, mu2, rtol=0, atol=1e-14)          # scale invariance in the weights


def test_degenerate_rule_holds_in_the_truth():
    x = PC.table(5).clone()
    x[11] = float("nan")
    ids = torch.tensor([-1, 40, 2, 3, 11, 5, 6])
    #            empty  masked  zero-weight  NaN row  plain
    offsets = torch.tensor([0, 0, 2, 4, 6, 7])
    w = torch.tensor([1.0, 1.0, 0.0, 0.0, 1.0, 1.0, 1.0])
    g = PC.upstream(5, 5)
    for dtype in (torch.float64, torch.float32):
        mu, gx, gw = PC.evaluate(x, ids, offsets, None, w, g, dtype)
        origin = np.zeros(5)
        origin[0] = 1
        assert all(np.array_equal(mu[i], origin) for i in range(4)) and np.isfinite(mu[4]).all() and mu[4, 0] > 1
        assert np.isfinite(gx[np.arange(40) != 11]).all() and not gw[:6].any()
        assert not gx[[2, 3, 5]].any() and not gx[11].any() and gx[6].any()


def test_float64_composition_loop_descends():
    before, after, history = PC.e2e_loop_float64()
    assert (before, after) == pytest.approx(PC.E2E_FLOAT64, rel=1e-9)
    steps = [before] + history
    assert all(b < a for a, b in zip(steps[:-1], steps[1:])) and before - after > 1.5
