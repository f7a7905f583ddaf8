"""Phase B of nav_field_tiled_kernel (csrc/ffmp_nav.hip) restated in NumPy / heapq: the
cost plane relaxed a T x T tile at a time, each tile to its local fixed point against a read-only
one-cell halo, with the kernel's dirty-tile work-list — the same scan order and the same rule for
which neighbours a write-back makes due.  The checker of tests/test_nav_tiled_host.py: the plane it
leaves must be tests/nav_field_ref.py's cost_to_go bit for bit.

The tile-local fixed point: the kernel's sweeps only lower values, so they end on the largest plane
below the tile's present values that no relaxation can lower; that is the shortest-path plane whose
sources are the halo cells and the tile's own cells at their present values, which a Dijkstra seeded
with all of them computes."""
from __future__ import annotations

import heapq

import numpy as np

from tests.nav_field_ref import INF, NEIGH, WEIGHT


def visit_bound(G: int) -> int:
    """The kernel's hard bound on tile visits per env."""
    return 2 * G * G


def tile_edge(G: int, tile: int) -> int:
    """The tile edge in use: 0 = 256, and no larger than the grid rounded up to 32."""
    T = tile or 256
    return min(T, (G + 31) // 32 * 32)


def _tile_fixed_point(d, hard, soft, q, soft_pen, i0, j0, R, Cn):
    """The tile's cells relaxed in place against the plane around it; True if any went down."""
    G = d.shape[0]
    heap = []
    for i in range(max(i0 - 1, 0), min(i0 + R + 1, G)):
        for j in range(max(j0 - 1, 0), min(j0 + Cn + 1, G)):
            if d[i, j] < INF:
                heap.append((int(d[i, j]), i, j))
    heapq.heapify(heap)
    changed = False
    while heap:
        db, bi, bj = heapq.heappop(heap)
        if db > d[bi, bj]:
            continue
        for (di, dj), w in zip(NEIGH, WEIGHT):
            ai, aj = bi - di, bj - dj  # the cell a whose move k lands on b
            if not (i0 <= ai < i0 + R and j0 <= aj < j0 + Cn) or hard[ai, aj] or (ai, aj) == q:
                continue  # only the tile's interior is relaxed: halo cells are read
            if di and dj and (hard[ai + di, aj] or hard[ai, aj + dj]):
                continue
            cand = db + w + (soft_pen if soft[ai, aj] else 0)
            if cand <= INF - 1 and cand < d[ai, aj]:
                d[ai, aj] = cand
                changed = True
                heapq.heappush(heap, (cand, ai, aj))
    return changed


def tiled_cost_to_go(hard, soft, q, soft_pen, tile):
    """(d uint16, tile visits, visit order): the kernel's phase B."""
    G = hard.shape[0]
    T = tile_edge(G, tile)
    nt = (G + T - 1) // T
    d = np.full((G, G), INF, dtype=np.int64)
    d[q] = 0
    dirty = np.zeros(nt * nt, dtype=bool)
    dirty[(q[0] // T) * nt + q[1] // T] = True
    visits, order, start = 0, [], 0
    while visits < visit_bound(G):
        due = [(start + s) % (nt * nt) for s in range(nt * nt) if dirty[(start + s) % (nt * nt)]]
        if not due:
            break
        t = due[0]  # the first dirty tile at or after `start`, cyclically
        start = (t + 1) % (nt * nt)
        visits += 1
        order.append(t)
        dirty[t] = False
        ti, tj = divmod(t, nt)
        i0, j0 = ti * T, tj * T
        R, Cn = min(T, G - i0), min(T, G - j0)
        old = d[i0:i0 + R, j0:j0 + Cn].copy()
        if not _tile_fixed_point(d, hard, soft, q, soft_pen, i0, j0, R, Cn):
            continue
        diff = d[i0:i0 + R, j0:j0 + Cn] != old
        # who sees what changed: an edge row / column its side neighbour, a corner cell the diagonal one
        seen = {(-1, 0): diff[0].any(), (1, 0): diff[-1].any(), (0, -1): diff[:, 0].any(), (0, 1): diff[:, -1].any(),
                (-1, -1): diff[0, 0], (-1, 1): diff[0, -1], (1, -1): diff[-1, 0], (1, 1): diff[-1, -1]}
        for (di, dj), hit in seen.items():
            ni, nj = ti + di, tj + dj
            if hit and 0 <= ni < nt and 0 <= nj < nt:
                dirty[ni * nt + nj] = True
    return d.astype(np.uint16), visits, order
