"""Adjacent token-pair counts of a corpus file (``hm_pairfreq_*``, hm_pairfreq.hip).

The reference fills ``pair_frequencies`` line by line (frequency_aware_hyperbolic_merge.py:92-112; the same loop in
enhanced_fast_hyperbolic_merge.py:266-289)::

    for line in open(corpus_path, "r", encoding="utf-8"):
        tokens = self.tokenize(line.strip())
        for pair in zip(tokens, tokens[1:]): freq[pair] = freq.get(pair, 0) + 1

``count_pair_frequencies`` gives the same dict (contents and insertion order) and the same total:

* lines are read as that loop reads them: strict UTF-8, universal newlines, a split on ``"\\n"`` only (never
  ``str.splitlines``, which also splits on ``\\x0b``, ``\\x0c``, ``\\x1c``-``\\x1e``, ``\\x85``, ``\\u2028``), then
  ``str.strip()``;
* on a HIP device every slab of lines goes through ``hm_tokenize_batch`` (only when there are merge rules: without
  them the symbols are the characters) and ``hm_pairfreq_add``; the distinct pairs come back with their counts and
  first positions, sorted by position, which is the order in which the dict first meets them;
* the rules are those of ``tok._batch_encoder()``: frozen at the first ``tokenize`` call, as the reference's
  ``_merge_rules`` cache is.

The host loop (``count_pair_frequencies_host``) serves non-HIP devices and runs whenever ``tokenize`` is customised by
a subclass or an instance.  Deviation, documented: the file is decoded before anything is counted, so a decoding
error leaves the dict untouched (the reference has counted the lines before the bad byte when it raises).
"""
from __future__ import annotations

import ctypes as C
import time
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .._handle import DeviceHandle
from .hyperbolic_merge import HyperbolicTokenizer

SLAB_CODE_POINTS = 1 << 26        # code points per device upload
_BIAS = 0x10FFFF + 2              # symbol -> 22-bit key field (hm_pairfreq.hip)
_FIELD = (1 << 22) - 1


def read_corpus_lines(corpus_path: str) -> List[str]:
    """``[line.strip() for line in open(corpus_path, "r", encoding="utf-8")]``: the text-mode reader's own newline
    translation, one split on ``"\\n"``; a final newline starts no further line."""
    with open(corpus_path, "r", encoding="utf-8") as f:
        text = f.read()
    if not text:
        return []
    lines = text.split("\n")
    if lines[-1] == "":
        lines.pop()
    return [line.strip() for line in lines]


def count_pair_frequencies_host(tok, lines: Sequence[str], into: Dict[Tuple[str, str], int]) -> int:
    """The reference loop over ``tok.tokenize``."""
    total = 0
    for line in lines:
        toks = tok.tokenize(line)
        for pair in zip(toks, toks[1:]):
            into[pair] = into.get(pair, 0) + 1
            total += 1
    return total


def tokenize_customised(tok) -> bool:
    return type(tok).tokenize is not HyperbolicTokenizer.tokenize or "tokenize" in tok.__dict__


class PairCounter(DeviceHandle):
    """One ``hm_pairfreq`` counter on a HIP device: slabs of (symbols, offsets, lengths) in, distinct pairs out."""

    PREFIX = "hm_pairfreq"

    def __init__(self, device: torch.device, initial_capacity: int = 0):
        super().__init__(device, int(initial_capacity))
        self.base = 0                 # flat position of the next slab's first symbol

    def add(self, sym: torch.Tensor, offsets: torch.Tensor, lengths: Optional[torch.Tensor] = None) -> None:
        """One slab: int32 ``sym``, int64 ``offsets[n + 1]`` (offsets[0] = 0, offsets[n] = sym.numel()), optional
        int32 ``lengths[n]`` (line l holds ``sym[offsets[l] : offsets[l] + lengths[l]]``)."""
        n_lines = offsets.numel() - 1
        n_pos = int(sym.numel())
        if sym.dtype != torch.int32 or offsets.dtype != torch.int64 or \
                (lengths is not None and (lengths.dtype != torch.int32 or lengths.numel() < n_lines)):
            raise ValueError("PairCounter.add: int32 symbols, int64 offsets, int32 lengths")
        self._check(self._L.hm_pairfreq_add(
            self._h, C.c_void_p(sym.data_ptr() if n_pos else 0), C.c_void_p(offsets.data_ptr()),
            C.c_void_p(lengths.data_ptr()) if lengths is not None else None, n_lines, n_pos, self.base, self._stream()))
        self.base += n_pos

    def sizes(self) -> Tuple[int, int, int]:
        """(distinct pairs, total pairs, slab recounts)"""
        d, p, r = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        self._check(self._L.hm_pairfreq_read(self._h, C.byref(d), C.byref(p), C.byref(r), None, None, None, 0,
                                             self._stream()))
        return d.value, p.value, r.value

    def read(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray, int]:
        """(left symbols, right symbols, counts, first positions) sorted by first position, and the total pair count."""
        d, total, _ = self.sizes()
        m = max(d, 1)
        keys = torch.empty(m, dtype=torch.int64, device=self.device)
        counts = torch.empty(m, dtype=torch.int64, device=self.device)
        first = torch.empty(m, dtype=torch.int64, device=self.device)
        self._check(self._L.hm_pairfreq_read(self._h, None, None, None, C.c_void_p(keys.data_ptr()),
                                             C.c_void_p(counts.data_ptr()), C.c_void_p(first.data_ptr()), m,
                                             self._stream()))
        order = torch.argsort(first[:d])
        k = keys[:d][order].cpu().numpy()
        a = ((k >> 22) & _FIELD) - _BIAS
        b = (k & _FIELD) - _BIAS
        return a, b, counts[:d][order].cpu().numpy(), first[:d][order].cpu().numpy(), total


def _symbol_strings(enc, syms: np.ndarray) -> list:
    out = np.empty(syms.shape[0], dtype=object)
    known = syms >= 0
    out[known] = enc._strings_arr[syms[known]]
    if not known.all():
        out[~known] = [chr(-int(s) - 2) for s in syms[~known].tolist()]
    return out.tolist()


def count_lines_device(tok, lines: Sequence[str], into: Dict[Tuple[str, str], int],
                       slab_code_points: int = SLAB_CODE_POINTS, initial_capacity: int = 0,
                       timing: Optional[dict] = None) -> int:
    """``count_pair_frequencies_host`` on the HIP device of ``tok``: slabs of lines through the tokenizer kernel and the
    pair counter.  ``timing`` (optional) receives ms per phase (encode: host symbols, upload, tokenize, count, dict)
    and the number of slab recounts."""
    if not lines:
        return 0
    t = timing if timing is not None else {}
    for key in ("encode_ms", "upload_ms", "tokenize_ms", "count_ms", "dict_ms"):
        t.setdefault(key, 0.0)
    enc = tok._batch_encoder()
    dev = enc.device
    counter = PairCounter(dev, initial_capacity)
    stream = torch.cuda.current_stream(dev)
    try:
        with torch.cuda.device(dev):
            start = 0
            while start < len(lines):
                stop, cps = start, 0
                while stop < len(lines) and (stop == start or cps + len(lines[stop]) <= slab_code_points):
                    cps += len(lines[stop])
                    stop += 1
                t0 = time.perf_counter()
                sym_h, off_h = enc.symbols(lines[start:stop])
                t1 = time.perf_counter()
                sym = torch.from_numpy(sym_h).to(dev)
                off = torch.from_numpy(off_h).to(dev)
                stream.synchronize()
                t2 = time.perf_counter()
                if enc.n_rules:
                    if int(np.diff(off_h).max()) >= 2 ** 31:
                        raise ValueError("a line of 2^31 or more characters")
                    lens = off[1:] - off[:-1]
                    order = torch.argsort(lens, descending=True, stable=True)
                    out, out_len, _ = enc.run(sym, off, order)
                    stream.synchronize()
                    t3 = time.perf_counter()
                    counter.add(out, off, out_len)
                else:
                    t3 = t2
                    counter.add(sym, off, None)
                t4 = time.perf_counter()
                t["encode_ms"] += (t1 - t0) * 1e3
                t["upload_ms"] += (t2 - t1) * 1e3
                t["tokenize_ms"] += (t3 - t2) * 1e3
                t["count_ms"] += (t4 - t3) * 1e3
                start = stop
            t5 = time.perf_counter()
            a, b, counts, _first, total = counter.read()
            t["recounts"] = counter.sizes()[2]
    finally:
        counter.close()
    left, right = _symbol_strings(enc, a), _symbol_strings(enc, b)
    if not into:                   # a fresh dict: one update in first-occurrence order
        into.update(zip(zip(left, right), counts.tolist()))
    else:
        get = into.get
        for pair, c in zip(zip(left, right), counts.tolist()):
            into[pair] = get(pair, 0) + c
    t["dict_ms"] += (time.perf_counter() - t5) * 1e3
    return int(total)


def count_pair_frequencies(tok, corpus_path: str, into: Dict[Tuple[str, str], int]) -> int:
    """Add the adjacent token pairs of every line of ``corpus_path`` to ``into`` (reference order) -> total pairs."""
    lines = read_corpus_lines(corpus_path)
    if tok.device.type == "cuda" and not tokenize_customised(tok):
        return count_lines_device(tok, lines, into)
    return count_pair_frequencies_host(tok, lines, into)
