"""Corpus metrics of a trained tokenizer as integer counts (C-ABI ``hm_tokstats``, hm_tokstats.hip).

The reference answers "how good is this tokenizer on a corpus?" with three host loops over ``tokenize(text)``
(scripts/compare_tokenizers.py: ``benchmark_hyperbolic_tokenizer`` :146-221, ``evaluate_linguistic_quality`` :224-289,
``evaluate_compression_efficiency`` :292-329; scripts/benchmark_efficiency.py:58-94 walks the same tokens).  Every number
they report is a ratio of the counts in ``CorpusStatistics``:

* ``tokens``, ``token_chars``: ``len(tokens)`` and ``sum(len(t) for t in tokens)`` (:181-183);
* ``word_boundary``: tokens in which ``[^\\w]`` finds something (:249, :266);
* ``morpheme``: tokens matching the suffix pattern (:250-252, :270-273);
* ``subword``: tokens with a word character on both sides of the boundary to a neighbour in the same line (:276-278);
* ``lines``, ``chars``: ``len(corpus)`` and ``sum(len(text))`` (:312).

On a HIP device the batch encoder leaves the token stream on the device (``BatchEncoder.run``) and ``hm_tokstats`` counts
it there: what it needs of a token is one 32-bit attribute word per symbol, built here ONCE per encoder state with Python's
own ``re`` and the reference's two patterns, and a bitmap of ``\\w`` over the code space for the characters outside the
rules.  No token comes back to the host.  A tokenizer whose ``tokenize`` is customised (subclass or instance) takes the
host loop ``corpus_statistics_host`` -- the reference's loops, restated once; there is no other CPU path: on a CPU device
the batch encoder raises ``HypMergeUnavailable``.
"""
from __future__ import annotations

import ctypes as C
import re
from dataclasses import dataclass
from typing import Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import _lib
from .pair_counter import SLAB_CODE_POINTS, tokenize_customised

N_CODEPOINTS = 0x110000
#: the reference's two patterns, verbatim (compare_tokenizers.py:249-252)
WORD_BOUNDARY_PATTERN = re.compile(r'[^\w]')
MORPHEME_PATTERN = re.compile(r'(ion|tion|ation|ment|ance|ence|ly|ish|less|ful|ness|ing|ed|er|est|pre|un|re|de|dis)$')
DEFAULT_BATCH_LINES = 1 << 18


@dataclass
class CorpusStatistics:
    lines: int = 0
    chars: int = 0           # sum(len(text))
    tokens: int = 0
    token_chars: int = 0     # sum(len(token)); equals chars whenever every rule's result is the concatenation of its operands
    word_boundary: int = 0
    morpheme: int = 0
    subword: int = 0

    def __add__(self, other: "CorpusStatistics") -> "CorpusStatistics":
        return CorpusStatistics(*(a + b for a, b in zip(self.astuple(), other.astuple())))

    def astuple(self) -> Tuple[int, ...]:
        return (self.lines, self.chars, self.tokens, self.token_chars, self.word_boundary, self.morpheme, self.subword)


def token_list_counts(tokens: Sequence[str]) -> Tuple[int, int, int, int, int]:
    """(tokens, token_chars, word_boundary, morpheme, subword) of ONE line's tokens: the reference's loop body."""
    n = len(tokens)
    chars = wb = mo = sub = 0
    search = WORD_BOUNDARY_PATTERN.search
    for i, token in enumerate(tokens):
        chars += len(token)
        if search(token):
            wb += 1
        if MORPHEME_PATTERN.search(token):
            mo += 1
        if (i > 0 and not search(tokens[i - 1][-1] + token[0])) or \
                (i < n - 1 and not search(token[-1] + tokens[i + 1][0])):
            sub += 1
    return n, chars, wb, mo, sub


def corpus_statistics_host(tokenize, texts: Iterable[str]) -> CorpusStatistics:
    """The reference's loops over ``tokenize(text)`` (any callable str -> list of str)."""
    st = CorpusStatistics()
    for text in texts:
        n, chars, wb, mo, sub = token_list_counts(tokenize(text))
        st.lines += 1
        st.chars += len(text)
        st.tokens += n
        st.token_chars += chars
        st.word_boundary += wb
        st.morpheme += mo
        st.subword += sub
    return st


# ----------------------------------------------------------------------------------------------
# the two tables of the kernel
# ----------------------------------------------------------------------------------------------
def token_attribute(s: str) -> int:
    """The attribute word of include/hypmerge.h for one token string."""
    if len(s) > _lib.TOKSTATS_MAX_LEN:
        raise ValueError(f"a token of {len(s)} code points: the attribute word holds lengths up to {_lib.TOKSTATS_MAX_LEN}")
    word = len(s) << _lib.TOKSTATS_LEN_SHIFT
    if not s:
        return word
    search = WORD_BOUNDARY_PATTERN.search
    if search(s):
        word |= _lib.TOKSTATS_NONWORD
    if MORPHEME_PATTERN.search(s):
        word |= _lib.TOKSTATS_MORPHEME
    if not search(s[0]):
        word |= _lib.TOKSTATS_FIRST_WORD
    if not search(s[-1]):
        word |= _lib.TOKSTATS_LAST_WORD
    return word


def attribute_table(strings: Sequence[str]) -> np.ndarray:
    """uint32[len(strings)]: ``token_attribute`` of every symbol's string."""
    return np.fromiter((token_attribute(s) for s in strings), dtype=np.uint32, count=len(strings))


_WORDMAP: Optional[np.ndarray] = None


def word_bitmap() -> np.ndarray:
    """uint32[0x110000 / 32]: bit ``cp & 31`` of word ``cp >> 5`` is set when ``re``'s ``\\w`` matches ``chr(cp)``.
    Built once per process by ONE substitution over the whole code space (surrogates included)."""
    global _WORDMAP
    if _WORDMAP is None:
        every = "".join(map(chr, range(N_CODEPOINTS)))
        marked = WORD_BOUNDARY_PATTERN.sub("\x00", every)          # chr(0) is itself not a word character
        cps = np.frombuffer(marked.encode("utf-32-le", "surrogatepass"), dtype=np.uint32)
        assert cps.shape[0] == N_CODEPOINTS
        bits = np.packbits((cps != 0).astype(np.uint8), bitorder="little")
        _WORDMAP = bits.view(np.uint32).copy()
        _WORDMAP.setflags(write=False)
    return _WORDMAP


def is_word_codepoint(cp: int) -> bool:
    return bool((int(word_bitmap()[cp >> 5]) >> (cp & 31)) & 1)


_WORDMAP_DEV: dict = {}


def _device_tables(tok, enc) -> Tuple[torch.Tensor, torch.Tensor]:
    """(attr, wordmap) on the encoder's device.  The attribute table lives beside ``tok._batch_encoder()``'s cache and
    is keyed the same way: it is rebuilt exactly when the encoder is."""
    cached = getattr(tok, "_token_attributes", None)
    if cached is None or cached[0] is not enc:
        attr = attribute_table(enc.strings)
        cached = (enc, torch.from_numpy(attr.view(np.int32)).to(enc.device))
        tok._token_attributes = cached
    key = (enc.device.type, enc.device.index if enc.device.index is not None else torch.cuda.current_device())
    wm = _WORDMAP_DEV.get(key)
    if wm is None:
        wm = torch.from_numpy(word_bitmap().view(np.int32).copy()).to(enc.device)
        _WORDMAP_DEV[key] = wm
    return cached[1], wm


# ----------------------------------------------------------------------------------------------
# the kernel
# ----------------------------------------------------------------------------------------------
def token_statistics(tokens: torch.Tensor, offsets: torch.Tensor, lengths: torch.Tensor, attr: torch.Tensor,
                     wordmap: torch.Tensor, *, per_line: bool = False, max_blocks: int = 0
                     ) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """``hm_tokstats`` on device arrays: int32 ``tokens``, int64 ``offsets[n + 1]``, int32 ``lengths[n]``, the int32 views of
    the attribute table and the bitmap -> (int64 totals[5], int64 per-line counts[n, 5] or None), both on the device.
    Asynchronous on the current stream.  Columns: tokens, token_chars, word_boundary, morpheme, subword."""
    L = _lib.load()
    for t in (tokens, offsets, lengths, attr, wordmap):
        if t.device.type != "cuda":
            raise _lib.HypMergeUnavailable("token_statistics needs tensors on a HIP device (there is no CPU path)")
    n_lines = offsets.numel() - 1
    if tokens.dtype != torch.int32 or offsets.dtype != torch.int64 or lengths.dtype != torch.int32 or \
            attr.dtype != torch.int32 or wordmap.dtype != torch.int32 or n_lines < 0 or lengths.numel() < n_lines or \
            wordmap.numel() != N_CODEPOINTS // 32:
        raise ValueError("token_statistics: int32 tokens / lengths / attr / wordmap, int64 offsets[n + 1], a whole bitmap")
    if not all(t.is_contiguous() for t in (tokens, offsets, lengths, attr, wordmap)):
        raise ValueError("token_statistics: contiguous tensors")
    dev = tokens.device
    with torch.cuda.device(dev):
        totals = torch.empty(_lib.TOKSTATS_COUNTERS, dtype=torch.int64, device=dev)
        lines = torch.empty((n_lines, _lib.TOKSTATS_COUNTERS), dtype=torch.int64, device=dev) if per_line else None
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None  # noqa: E731
        _lib.check(L.hm_tokstats(ptr(tokens), ptr(offsets), ptr(lengths), n_lines, tokens.numel(), ptr(attr), attr.numel(),
                                 ptr(wordmap), ptr(totals), ptr(lines), int(max_blocks),
                                 C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    return totals, lines


def _slabs(texts: Sequence[str], batch_lines: int, slab_code_points: int):
    start = 0
    while start < len(texts):
        stop, cps = start, 0
        while stop < len(texts) and stop - start < batch_lines and (stop == start or cps + len(texts[stop]) <= slab_code_points):
            cps += len(texts[stop])
            stop += 1
        yield start, stop
        start = stop


def corpus_statistics_device(tok, texts: Sequence[str], *, batch_lines: int = DEFAULT_BATCH_LINES,
                             slab_code_points: int = SLAB_CODE_POINTS, per_line: bool = False, timing: Optional[dict] = None):
    """``corpus_statistics`` on the HIP device of ``tok``; with ``per_line`` also the int64 array [len(texts), 5] of every
    line's counts (host).  ``timing`` (optional) receives event-timed ms of the encoder and of the statistics kernel."""
    if batch_lines < 1:
        raise ValueError("batch_lines must be at least 1")
    enc = tok._batch_encoder()
    attr, wordmap = _device_tables(tok, enc)
    dev = enc.device
    st = CorpusStatistics(lines=len(texts))
    rows: List[torch.Tensor] = []
    events = []
    with torch.cuda.device(dev):
        acc = torch.zeros(_lib.TOKSTATS_COUNTERS, dtype=torch.int64, device=dev)
        for start, stop in _slabs(texts, batch_lines, slab_code_points):
            sym_h, off_h = enc.symbols(texts[start:stop])
            st.chars += int(off_h[-1])
            lens_h = np.diff(off_h)
            if lens_h.max() >= 2 ** 31:
                raise ValueError("a line of 2^31 or more characters")
            sym = torch.from_numpy(sym_h).to(dev)
            off = torch.from_numpy(off_h).to(dev)
            lens = off[1:] - off[:-1]
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)] if timing is not None else None
            if ev:
                ev[0].record()
            if enc.n_rules:
                order = torch.argsort(lens, descending=True, stable=True)
                out, out_len, _ = enc.run(sym, off, order)
            else:                  # no rules: the tokens are the characters
                out, out_len = sym, lens.to(torch.int32)
            if ev:
                ev[1].record()
            totals, lines = token_statistics(out, off, out_len.contiguous(), attr, wordmap, per_line=per_line)
            if ev:
                ev[2].record()
                events.append(ev)
            acc += totals
            if lines is not None:
                rows.append(lines)
        got = acc.cpu().tolist()
        if timing is not None:
            timing["encode_kernel_ms"] = sum(e[0].elapsed_time(e[1]) for e in events)
            timing["stats_kernel_ms"] = sum(e[1].elapsed_time(e[2]) for e in events)
            timing["slabs"] = len(events)
    st.tokens, st.token_chars, st.word_boundary, st.morpheme, st.subword = (int(x) for x in got)
    if per_line:
        table = torch.cat(rows).cpu().numpy() if rows else np.zeros((0, _lib.TOKSTATS_COUNTERS), dtype=np.int64)
        return st, table
    return st


def corpus_statistics(tok, texts: Sequence[str], *, batch_lines: int = DEFAULT_BATCH_LINES) -> CorpusStatistics:
    """The counts of ``texts`` under ``tok``: the HIP path (slabs of ``batch_lines`` lines through the batch encoder and
    ``hm_tokstats``), or the host loop over ``tok.tokenize`` when ``tokenize`` is customised."""
    texts = texts if isinstance(texts, (list, tuple)) else list(texts)
    if tokenize_customised(tok):
        return corpus_statistics_host(tok.tokenize, texts)
    return corpus_statistics_device(tok, texts, batch_lines=batch_lines)
