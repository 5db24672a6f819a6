"""The engine's table limit, 2^20 rows (engine.MAX_TABLE_ROWS), where no GPU is needed: the C ABI's argument check and the
tokenizer classes' construction check.  Tables of more than 131 072 rows (engine.MAX_ROWS) use the wide argmin key of the
pair scan; tests/test_gpu_wide_key.py runs them."""
import ctypes as C

import pytest
import torch


def test_limit_constants():
    from hyptokenizer_amd import engine
    assert engine.MAX_TABLE_ROWS == 1 << 20
    assert engine.MAX_ROWS == 131072          # the narrow key's largest table, unchanged


def test_engine_create_takes_2_20_rows():
    from hyptokenizer_amd import _lib
    L = _lib.load()
    h = C.c_void_p(0)
    st = L.hm_engine_create(C.byref(h), 0, 1 << 20, 17, 1, 0)
    assert st != _lib.HM_E_ARG, L.hm_last_error(None)
    if torch.cuda.is_available():
        assert st == _lib.HM_OK and h.value
        assert L.hm_engine_destroy(h) == _lib.HM_OK
    else:
        assert st > 0 and not h.value             # the no-device status (a hipError_t)
        assert b"no HIP device" in L.hm_last_error(None)
    h = C.c_void_p(0)
    assert L.hm_engine_create(C.byref(h), 0, (1 << 20) + 1, 17, 1, 0) == _lib.HM_E_ARG
    assert b"1048576" in L.hm_last_error(None) and not h.value


def _vocab(n):
    return [f"t{k}" for k in range(n)]


def test_tokenizer_constructs_past_the_narrow_limit():
    from hyptokenizer_amd.engine import HypMergeUnavailable
    from hyptokenizer_amd.synthetic import lorentz_table
    from hyptokenizer_amd.tokenizer.hyperbolic_merge import HyperbolicTokenizer
    n = 64
    tok = HyperbolicTokenizer(_vocab(n), torch.nn.Parameter(lorentz_table(n, 8, seed=1, scale=0.05)), merge_threshold=0.5,
                              device=torch.device("cpu"), max_vocab_size=200_000, sign_convention="lorentz")
    assert tok.embeddings.shape == (200_000, 9) and tok.max_vocab_size == 200_000
    with pytest.raises(HypMergeUnavailable):          # the engine is created lazily, by the first search
        tok.optimize_merges(steps=1, log_every=10 ** 9)


def test_tokenizer_refuses_more_than_max_table_rows():
    from hyptokenizer_amd.synthetic import lorentz_table
    from hyptokenizer_amd.tokenizer.hyperbolic_merge import HyperbolicTokenizer
    n = 64
    with pytest.raises(ValueError, match="MAX_TABLE_ROWS"):
        HyperbolicTokenizer(_vocab(n), torch.nn.Parameter(lorentz_table(n, 8, seed=1, scale=0.05)), merge_threshold=0.5,
                            device=torch.device("cpu"), max_vocab_size=2 ** 20 + 1, sign_convention="lorentz")
