"""Tile plan of tile-packed attention (``--attn-tile-pack``).

A pure function of ``cu_seqlens`` and the packed row count ``T``: which
64-row attention tiles a packed batch needs when several whole consecutive
short sequences may share one tile. The GPU builds it on the device
(``fa_tile_plan_kernel`` in csrc/attention.hip); :func:`tile_plan_reference`
is the same walk in Python, integer for integer, for tests and tools.
"""

from __future__ import annotations

from typing import List, NamedTuple, Sequence, Tuple

import torch

TILE = 64          # rows of an attention tile
SEQ_CAP = 1024     # key cap of the attention kernels (LDS-resident rows)
PLAN_HEADER = 4    # int32 slots ahead of the item list; [0] is the count


def tile_plan_max_items(total_rows: int, num_seqs: int) -> int:
    """Upper bound on the item count from ``(T, B)`` alone; it sizes the
    item list and the attention grid (proof: csrc/attention.hip,
    ``flash_attn_tilepack_max_items``)."""
    return max(1, min(total_rows // TILE + num_seqs,
                      3 * total_rows // 65 + 1))


def tile_plan_reference(cu_seqlens: Sequence[int], total_rows: int
                        ) -> Tuple[List[Tuple[int, int, int]],
                                   List[Tuple[int, int]]]:
    """``(items, bounds)`` of the plan.

    ``items``: ``(first packed row, row count, tile)`` in sequence order. A
    sequence of more than 64 rows gives one item per 64-row tile of itself;
    consecutive sequences of at most 64 rows are collected greedily into a
    group of at most 64 contiguous rows, which is one item (tile 0). Empty
    sequences give nothing. ``bounds[r]`` is ``(start, end)`` of packed row
    r's sequence, ``(0, 0)`` for a row outside every sequence."""
    T = int(total_rows)
    cu = [min(max(int(c), 0), T) for c in cu_seqlens]
    items: List[Tuple[int, int, int]] = []
    bounds = [(0, 0)] * T
    g0 = gn = 0
    for s0, s1 in zip(cu[:-1], cu[1:]):
        n = min(s1 - s0, SEQ_CAP)
        if n <= 0:
            continue
        bounds[s0:s0 + n] = [(s0, s0 + n)] * n
        if n > TILE:
            if gn:
                items.append((g0, gn, 0))
            gn = 0
            items.extend((s0, n, t) for t in range((n + TILE - 1) // TILE))
        else:
            if gn and (g0 + gn != s0 or gn + n > TILE):
                items.append((g0, gn, 0))
                gn = 0
            if not gn:
                g0 = s0
            gn += n
    if gn:
        items.append((g0, gn, 0))
    return items, bounds


class AttnTilePlan(NamedTuple):
    """Device-side plan: ``buf`` is what the kernels read; ``count`` [1],
    ``items`` [max_items, 4] and ``bounds`` [T, 2] are views of it."""
    buf: torch.Tensor
    count: torch.Tensor
    items: torch.Tensor
    bounds: torch.Tensor


def plan_views(buf: torch.Tensor, total_rows: int) -> AttnTilePlan:
    m = (buf.numel() - PLAN_HEADER - 2 * total_rows) // 4
    return AttnTilePlan(
        buf, buf[:1], buf[PLAN_HEADER:PLAN_HEADER + 4 * m].view(m, 4),
        buf[PLAN_HEADER + 4 * m:].view(total_rows, 2))


def plan_from_reference(cu_seqlens: torch.Tensor,
                        total_rows: int) -> AttnTilePlan:
    """The reference plan in the device layout (host path: reads
    ``cu_seqlens``)."""
    cu = cu_seqlens.tolist()
    m = tile_plan_max_items(total_rows, len(cu) - 1)
    items, bounds = tile_plan_reference(cu, total_rows)
    buf = torch.zeros(PLAN_HEADER + 4 * m + 2 * total_rows, dtype=torch.int32)
    buf[0] = len(items)
    if items:
        buf[PLAN_HEADER:PLAN_HEADER + 4 * len(items)] = torch.tensor(
            [(r0, n, t, 0) for r0, n, t in items],
            dtype=torch.int32).flatten()
    buf[PLAN_HEADER + 4 * m:] = torch.tensor(
        bounds, dtype=torch.int32).reshape(-1)
    return plan_views(buf.to(cu_seqlens.device), total_rows)
