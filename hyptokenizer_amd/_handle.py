"""What the wrappers of the text-side library components share: ownership of one library handle on a HIP device
(``DeviceHandle``) and the strings -> code points conversion of the C ABI (``code_points``)."""
from __future__ import annotations

import ctypes as C
from typing import Sequence, Tuple

import numpy as np
import torch


def code_points(strings: Sequence[str], errors: str = "strict") -> Tuple[np.ndarray, np.ndarray, str]:
    """(UTF-32 code points int32 of ``strings`` concatenated, int64 offsets ``[len(strings) + 1]``, the joined text).
    ``errors`` is the encoder's error mode: ``"surrogatepass"`` lets lone surrogates through as code points."""
    flat = "".join(strings)
    cps = np.frombuffer(flat.encode("utf-32-le", errors), dtype=np.int32)
    offsets = np.zeros(len(strings) + 1, np.int64)
    np.cumsum(np.fromiter(map(len, strings), dtype=np.int64, count=len(strings)), out=offsets[1:])
    return cps, offsets, flat


class DeviceHandle:
    """Owns a handle made by ``<PREFIX>_create`` and freed by ``<PREFIX>_destroy``.  ``args`` follow the device index in
    the create call; with ``engine`` (a ``MergeEngine``) the handle is created on that engine instead, whose device it
    shares and whose error text ``_check`` reports."""

    PREFIX = ""

    def __init__(self, device=None, *args, engine=None):
        from . import _lib
        self._lib = _lib
        self._L = _lib.load()
        self._h = C.c_void_p(0)
        self._engine = engine._h if engine is not None else None
        device = torch.device(engine.device if engine is not None else device)
        if device.type != "cuda":
            raise _lib.HypMergeUnavailable(f"{type(self).__name__} needs a HIP device (device={device})")
        idx = device.index if device.index is not None else torch.cuda.current_device()
        self.device = torch.device("cuda", idx)
        self._create_args = (self._engine,) if engine is not None else (int(idx),) + args
        self._create()

    def _create(self) -> None:
        """A fresh handle in place of the current one."""
        self.close()
        h = C.c_void_p(0)
        self._check(getattr(self._L, self.PREFIX + "_create")(C.byref(h), *self._create_args))
        self._h = h

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            getattr(self._L, self.PREFIX + "_destroy")(self._h)
            self._h = C.c_void_p(0)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self) -> C.c_void_p:
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _check(self, status: int) -> None:
        self._lib.check(status, self._engine)
