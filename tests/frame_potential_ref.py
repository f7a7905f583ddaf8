"""The potential field of an occupancy frame (include/ffmp.h ffmp_frame_potential) restated in
NumPy — the checker of tests/test_frame_potential_host.py and tests/test_gpu_frame_potential.py.  Nothing here
is shared with the kernel.

The clearance comes in two forms: dist2_brute, the SPEC's window minimum taken literally ((2 reach + 1)^2 shifted
planes), and dist2_separable, the same minimum taken along j and then along i (2 (2 reach + 1) shifted planes).
The host test holds the two equal on random planes; the GPU test, whose planes are larger, uses the second."""
from __future__ import annotations

import math

import numpy as np

F32 = np.float32
NONE = 65535


def obstacles(frames, occ_min=255) -> np.ndarray:
    """obst = F >= occ_min: a float compare for a float32 frame (a NaN is free), an integer one for uint8."""
    frames = np.asarray(frames)
    with np.errstate(invalid="ignore"):
        return frames >= (F32(occ_min) if frames.dtype == np.float32 else int(occ_min))


def _shift(a, di, dj, fill):
    """s[..., i, j] = a[..., i + di, j + dj], `fill` where that leaves the plane."""
    G = a.shape[-1]
    out = np.full_like(a, fill)
    if abs(di) < G and abs(dj) < G:
        out[..., max(-di, 0):G - max(di, 0), max(-dj, 0):G - max(dj, 0)] = \
            a[..., max(di, 0):G + min(di, 0), max(dj, 0):G + min(dj, 0)]
    return out


def dist2_brute(obst, reach) -> np.ndarray:
    """d2 (…, G, G) uint16: min di^2 + dj^2 over obstacle cells inside the square window, 65535 if none."""
    obst = np.asarray(obst, bool)
    d2 = np.full(obst.shape, NONE, np.int64)
    for di in range(-reach, reach + 1):
        for dj in range(-reach, reach + 1):
            hit = _shift(obst, di, dj, False)
            d2 = np.where(hit, np.minimum(d2, di * di + dj * dj), d2)
    return d2.astype(np.uint16)


def dist2_separable(obst, reach) -> np.ndarray:
    """The same plane in two passes: g = min |dj| along the row, then min di^2 + g^2 along the column."""
    obst = np.asarray(obst, bool)
    big = 1 << 20
    g = np.full(obst.shape, big, np.int64)
    for dj in range(-reach, reach + 1):
        g = np.where(_shift(obst, 0, dj, False), np.minimum(g, abs(dj)), g)
    d2 = np.full(obst.shape, NONE, np.int64)
    for di in range(-reach, reach + 1):
        gs = _shift(g, di, 0, big)
        d2 = np.where(gs < big, np.minimum(d2, di * di + gs * gs), d2)
    return d2.astype(np.uint16)


def potential(d2, goal, cfg) -> np.ndarray:
    """U (N, G, G) float32 from d2 (N, G, G) and the ego goals (N, 2) float32: the SPEC's expressions, one float32
    operation at a time."""
    k = cfg.f32_constants()
    d2 = np.asarray(d2)
    n, G = d2.shape[0], d2.shape[-1]
    goal = np.asarray(goal, F32).reshape(n, 2)
    coord = np.arange(G, dtype=F32) * k["res_f"] - k["half_f"]
    with np.errstate(all="ignore"):
        dx = coord[None, :, None] - goal[:, 0, None, None]
        dy = coord[None, None, :] - goal[:, 1, None, None]
        U = k["half_ka_f"] * (dx * dx + dy * dy)
        d = np.sqrt(d2.astype(F32)) * k["res_f"]
        d = np.maximum(d, k["rho_min_f"])
        q = F32(1.0) / d - k["inv_rho0_f"]
        rep = U + k["half_kr_f"] * (q * q)
    assert U.dtype == F32 and rep.dtype == F32
    return np.where((d2 != NONE) & (d < k["rho0_f"]), rep, U)


def default_reach(cfg) -> int:
    return int(math.ceil(cfg.rho0 / cfg.res))


def frame_potential(frames, goal, cfg, occ_min=255, reach=None, dtype=np.float32, mask=None, dist2_in=None, potential_in=None,
                    grad_in=None, robot_d2_in=None, brute=False):
    """frames (N, G, G) float32 or uint8, goal (N, 2) float32 -> dict(dist2 uint16, potential `dtype`, grad (N, 2)
    float32, robot_d2 (N,) int32).  mask: envs with 0 keep what the *_in arrays hold."""
    frames = np.asarray(frames)
    n, G = frames.shape[0], frames.shape[-1]
    c = G // 2
    reach = default_reach(cfg) if reach is None else int(reach)
    k = cfg.f32_constants()
    d2 = (dist2_brute if brute else dist2_separable)(obstacles(frames, occ_min), reach)
    U = potential(d2, goal, cfg)
    with np.errstate(all="ignore"):
        grad = np.stack([(U[:, c + 1, c] - U[:, c - 1, c]) * k["inv_2res_f"], (U[:, c, c + 1] - U[:, c, c - 1]) * k["inv_2res_f"]], axis=1)
        plane = U.astype(dtype)  # binary16: round to nearest even
    assert grad.dtype == F32
    rd2 = np.where(d2[:, c, c] == NONE, -1, d2[:, c, c].astype(np.int32)).astype(np.int32)
    out = {"dist2": d2, "potential": plane, "grad": grad, "robot_d2": rd2}
    if mask is not None:
        m = np.asarray(mask).astype(bool)
        for key, prev in (("dist2", dist2_in), ("potential", potential_in), ("grad", grad_in), ("robot_d2", robot_d2_in)):
            sel = m.reshape((n,) + (1,) * (out[key].ndim - 1))
            out[key] = np.where(sel, out[key], np.asarray(prev)).astype(out[key].dtype)
    return out


def clearance(robot_d2, res) -> np.ndarray:
    """(N,) float64 metres: sqrt(robot_d2) * res, inf where -1."""
    r = np.asarray(robot_d2).astype(np.float64)
    return np.where(r < 0, np.inf, np.sqrt(np.maximum(r, 0.0)) * float(res))


def policy_field(grad, dt) -> np.ndarray:
    """ffmp_policy_field's rule in float64, operation for operation: (N, 2) float32 gradients -> (N, 2) [v, w]."""
    g = np.asarray(grad, F32).astype(np.float64)
    out = np.zeros((g.shape[0], 2))
    for e, (gx, gy) in enumerate(g):
        m2 = gx * gx + gy * gy
        if m2 > 0.0 and np.isfinite(m2):
            m = np.sqrt(m2)
            dx, dy = -gx / m, -gy / m
            w = dy / dt
            w = -0.6 if w < -0.6 else (0.6 if w > 0.6 else w)
            if dx < 0.0:
                w = 0.6 if dy >= 0.0 else -0.6
            out[e] = (0.6 * (dx if dx > 0.0 else 0.0), w)
    return out


def same_bits(got, exp) -> np.ndarray:
    """Elementwise: the same bits, any NaN equal to any NaN (a NaN's sign and payload are the machine's)."""
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.dtype == exp.dtype and got.shape == exp.shape, (got.dtype, exp.dtype, got.shape, exp.shape)
    if got.dtype.kind != "f":
        return got == exp
    u = {2: np.uint16, 4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    return (got.view(u) == exp.view(u)) | (np.isnan(got) & np.isnan(exp))
