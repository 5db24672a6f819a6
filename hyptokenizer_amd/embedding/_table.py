"""The Lorentz table the lane-group kernels gather rows from (csrc/hm_rowgroup.h): its widths, its leading dimension and the
one check of its dtype, shape and strides."""
from __future__ import annotations

import torch

MIN_WIDTH, MAX_WIDTH = 2, 129


def ld(table: torch.Tensor) -> int:
    return table.stride(0) if table.shape[0] > 1 else max(table.stride(0), table.shape[1])


def check_table(who: str, table: torch.Tensor) -> None:
    if table.dtype != torch.float32:
        raise ValueError(f"{who}: the table must be float32, got {table.dtype}")
    if table.dim() != 2 or not (MIN_WIDTH <= table.shape[1] <= MAX_WIDTH):
        raise ValueError(f"{who}: the table must be [V, d + 1] with d + 1 in {MIN_WIDTH}..{MAX_WIDTH}, got shape {tuple(table.shape)}")
    if table.stride(1) != 1 or (table.shape[0] > 1 and table.stride(0) < table.shape[1]):
        raise ValueError(f"{who}: the table needs unit stride in its last dimension (strides {table.stride()})")
