"""Wide-prior and global relocalisation (include/ffmp.h ffmp_scan_relocalize) restated in NumPy —
the checker of tests/test_gpu_scan_reloc.py.

The cells of every beam and rotation are scan_match_ref._cells', so the fine score is ffmp_scan_match's word for
word.  exhaustive() scores every shift of any radius by summing, per `on` beam, the (2R + 1)^2 window of the
zero-padded plane round its cell.  sliding_max() is X, bounds() is U, and relocalize() follows the SPEC's schedule
literally: the seed, S1, the refined set, the winner over the refined blocks' shifts — it never looks at a shift
outside the refined set.  The winner is picked by a lexicographic sort of the SPEC's tie order, as
scan_match_ref._finish picks it.

kidnapped() is the physical tie: rooms mapped over 30 steps, then the robot located on the whole plane and the full
circle with no prior.  `python tests/scan_reloc_ref.py` prints its figures."""
import math
import os
import sys

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

if __name__ == "__main__":  # run as a script: the repository root is not on the path yet
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle.ffmp_oracle import Cfg
from tests import scan_match_ref as SM
from tests import world_map_ref as W

F32 = np.float32
INT32_MIN = -2 ** 31


def n_blocks(R: int, B: int) -> int:
    return (2 * R + B) // B


class Scene:
    """What every function below starts from: the planes, the cells of every (env, rotation, beam) and the gate's inputs."""

    def __init__(self, cfg: Cfg, m, ranges, pose, R: int, T: int, dtheta: float = 0.0, range_max=np.inf, beams=None, turns=None):
        self.cfg, self.R, self.T = cfg, int(R), int(T)
        self.m = np.asarray(m, np.int8)
        self.ranges = np.asarray(ranges, F32)
        n, L = self.ranges.shape
        self.n, self.Wc = n, self.m.shape[1]
        self.pose = np.ascontiguousarray(np.asarray(pose, F32).reshape(n, -1)[:, 0:4])
        beams = SM.beam_dirs(L) if beams is None else np.asarray(beams, F32)
        self.turns = SM.turn_table(T, dtheta) if turns is None else np.asarray(turns, F32)
        assert self.turns.shape == (2 * T + 1, 2) and beams.shape == (L, 2) and 0 <= R <= 1024 and 0 <= T <= 512
        self.valid, fp, fq, self.on, self.ck, self.sk = SM._cells(cfg, self.Wc, self.ranges, self.pose, beams, self.turns, R, range_max)
        self.gp = np.where(self.on, fp, F32(0.0)).astype(np.int64)  # converted only where on holds
        self.gq = np.where(self.on, fq, F32(0.0)).astype(np.int64)
        self.pad = 2 * R + 16  # fp in -R .. Wc-1+R and a in -R .. R; a block's window may reach B - 1 past R
        self.mp = np.zeros((n, self.Wc + 2 * self.pad, self.Wc + 2 * self.pad), np.int8)
        self.mp[:, self.pad:self.pad + self.Wc, self.pad:self.pad + self.Wc] = self.m

    def cells(self, e: int, k: int):
        sel = self.on[e, k]
        return self.gp[e, k][sel], self.gq[e, k][sel]

    def window_scores(self, e: int, k: int, a0: int, b0: int, h: int, w: int) -> np.ndarray:
        """S(k - T, a, b) for a in a0..a0+h-1, b in b0..b0+w-1: (h, w) int32."""
        p, q = self.cells(e, k)
        win = sliding_window_view(self.mp[e], (h, w))
        return win[p + self.pad + a0, q + self.pad + b0].sum(axis=0, dtype=np.int32).reshape(h, w)

    def zero_score(self, e: int) -> int:
        return int(self.window_scores(e, self.T, 0, 0, 1, 1)[0, 0])


def _order(kk, aa, bb, S):
    """Index of the winner under ffmp_scan_match's total order (scan_match_ref._finish's sort, over the candidates
    of the largest score)."""
    top = np.nonzero(S == S.max())[0]
    kk, aa, bb = kk[top], aa[top], bb[top]
    return top[np.lexsort((bb, aa, kk, np.abs(kk), aa * aa + bb * bb))[0]]


def refined_from_volume(U: np.ndarray, vol: np.ndarray, R: int, B: int) -> np.ndarray:
    """The schedule's refined count (n,) read off an exhaustive volume: S1 is the seed block's largest S."""
    n = U.shape[0]
    top = block_max(vol, R, B).reshape(n, -1)
    flat = U.reshape(n, -1)
    S1 = top[np.arange(n), np.argmax(flat, axis=1)]
    return (flat >= S1[:, None]).sum(axis=1)


def _gate(sc: Scene, winners, zero, refined, min_valid: int, min_gain: int, min_score: int):
    """pose_out (n, 4) float32 and info (n, 8) int32 from the winners (n, 4) {k, a, b, S}."""
    res = F32(sc.cfg.f["res_f"])
    finite = np.isfinite(sc.pose).all(axis=1)
    nvalid = sc.valid.sum(axis=1).astype(np.int32)
    pose_out = sc.pose.copy()
    info = np.zeros((sc.n, 8), np.int32)
    for e in range(sc.n):
        k, a, b, best = (int(v) for v in winners[e])
        z = int(zero[e])
        ok = bool(finite[e]) and nvalid[e] >= min_valid and best - z >= min_gain and (k, a, b) != (0, 0, 0) and best >= min_score
        info[e] = (1, k, a, b, best, z, nvalid[e], refined[e]) if ok else (0, 0, 0, 0, best, z, nvalid[e], refined[e])
        if ok:
            da = F32(a) * res
            db = F32(b) * res
            pose_out[e] = (sc.pose[e, 0] + da, sc.pose[e, 1] + db, sc.ck[e, k + sc.T], sc.sk[e, k + sc.T])
    assert pose_out.dtype == F32
    return pose_out, info


def exhaustive(cfg: Cfg, m, ranges, pose, R: int, T: int, dtheta: float = 0.0, range_max=np.inf, min_valid: int = 0,
               min_gain: int = 0, min_score: int = INT32_MIN, block=None, beams=None, turns=None, scene=None):
    """Every shift scored, any R: (pose_out, info, volume (n, 2T+1, 2R+1, 2R+1) int32).  info[7] is what
    FFMP_RELOC_EXHAUSTIVE reports with `block`, else 0."""
    sc = Scene(cfg, m, ranges, pose, R, T, dtheta, range_max, beams, turns) if scene is None else scene
    A, K = 2 * R + 1, 2 * T + 1
    vol = np.zeros((sc.n, K, A, A), np.int32)
    kk, aa, bb = np.meshgrid(np.arange(-T, T + 1), np.arange(-R, R + 1), np.arange(-R, R + 1), indexing="ij")
    kk, aa, bb = kk.ravel(), aa.ravel(), bb.ravel()
    winners = np.zeros((sc.n, 4), np.int64)
    for e in range(sc.n):
        for k in range(K):
            vol[e, k] = sc.window_scores(e, k, -R, -R, A, A)
        S = vol[e].ravel()
        w = _order(kk, aa, bb, S)
        winners[e] = (kk[w], aa[w], bb[w], S[w])
    refined = np.full(sc.n, K * n_blocks(R, block) ** 2 if block else 0)
    pose_out, info = _gate(sc, winners, vol[:, T, R, R], refined, min_valid, min_gain, min_score)
    return pose_out, info, vol


def sliding_max(m, B: int) -> np.ndarray:
    """X[p][q] for p, q in -(B - 1)..Wc - 1 at index [p + B - 1][q + B - 1]: (n, Wc + B - 1, Wc + B - 1) int8.  0 elsewhere."""
    m = np.asarray(m, np.int8)
    n, Wc, _ = m.shape
    mz = np.zeros((n, Wc + 2 * (B - 1), Wc + 2 * (B - 1)), np.int8)
    mz[:, B - 1:B - 1 + Wc, B - 1:B - 1 + Wc] = m
    return sliding_window_view(mz, (B, B), axis=(1, 2)).max(axis=(3, 4))


def _bounds(sc: Scene, B: int) -> np.ndarray:
    R, K, nb = sc.R, 2 * sc.T + 1, n_blocks(sc.R, B)
    X = sliding_max(sc.m, B)
    Wx = X.shape[1]
    a0 = -R + B * np.arange(nb)
    U = np.zeros((sc.n, K, nb, nb), np.int32)
    for e in range(sc.n):
        for k in range(K):
            p, q = sc.cells(e, k)
            P = p[:, None] + a0[None, :] + (B - 1)  # X's index of fp + a0(A)
            Q = q[:, None] + a0[None, :] + (B - 1)
            inP, inQ = (P >= 0) & (P < Wx), (Q >= 0) & (Q < Wx)
            got = X[e][np.clip(P, 0, Wx - 1)[:, :, None], np.clip(Q, 0, Wx - 1)[:, None, :]].astype(np.int32)
            U[e, k] = (got * (inP[:, :, None] & inQ[:, None, :])).sum(axis=0, dtype=np.int32)
    return U


def bounds(cfg: Cfg, m, ranges, pose, R: int, T: int, B: int, dtheta: float = 0.0, range_max=np.inf, beams=None, turns=None):
    """U (n, 2T+1, nb, nb) int32."""
    return _bounds(Scene(cfg, m, ranges, pose, R, T, dtheta, range_max, beams, turns), B)


def block_max(vol: np.ndarray, R: int, B: int) -> np.ndarray:
    """The largest S of every block of an exhaustive volume: (n, K, nb, nb) int64."""
    nb = n_blocks(R, B)
    n, K, A, _ = vol.shape
    v = np.full((n, K, nb * B, nb * B), np.iinfo(np.int64).min, np.int64)
    v[:, :, :A, :A] = vol
    return v.reshape(n, K, nb, B, nb, B).max(axis=(3, 5))


def relocalize(cfg: Cfg, m, ranges, pose, R: int, T: int, B: int, dtheta: float = 0.0, range_max=np.inf, min_valid: int = 0,
               min_gain: int = 0, min_score: int = INT32_MIN, beams=None, turns=None, scene=None, U=None):
    """One ffmp_scan_relocalize call, the schedule read literally: (pose_out, info, U)."""
    assert B in (2, 4, 8, 16)
    sc = Scene(cfg, m, ranges, pose, R, T, dtheta, range_max, beams, turns) if scene is None else scene
    U = _bounds(sc, B) if U is None else U
    nb = n_blocks(R, B)
    winners = np.zeros((sc.n, 4), np.int64)
    refined = np.zeros(sc.n, np.int64)
    zero = np.zeros(sc.n, np.int64)

    def block(e, lin):
        k, A, Cc = lin // (nb * nb), (lin // nb) % nb, lin % nb
        a0, b0 = -R + A * B, -R + Cc * B
        S = sc.window_scores(e, k, a0, b0, B, B)[:R - a0 + 1, :R - b0 + 1]
        aa, bb = np.meshgrid(a0 + np.arange(S.shape[0]), b0 + np.arange(S.shape[1]), indexing="ij")
        return np.full(S.size, k - T), aa.ravel(), bb.ravel(), S.ravel()

    for e in range(sc.n):
        flat = U[e].ravel()
        seed = int(np.argmax(flat))  # the first of the largest: the smallest linear index
        S1 = int(block(e, seed)[3].max())
        todo = np.nonzero(flat >= S1)[0]
        refined[e] = todo.size
        kk, aa, bb, S = (np.concatenate(x) for x in zip(*(block(e, int(lin)) for lin in todo)))
        w = _order(kk, aa, bb, S)
        winners[e] = (kk[w], aa[w], bb[w], S[w])
        zero[e] = sc.zero_score(e)
    pose_out, info = _gate(sc, winners, zero, refined, min_valid, min_gain, min_score)
    return pose_out, info, U


# ---------------------------------------------------------------- random planes, the poses and ranges of the matcher's tests
DTH = 0.03


def random_case(cells: int, L: int, NP: int, seed: int, range_max=None):
    """(config, cfg, planes, ranges, pose, range_max) as tests/test_gpu_scan_match.Raw makes its batch: _planes, _poses,
    _mixed_rows — corners, off the plane, NaN/inf words, |(c, s)| != 1; saturated and empty planes."""
    from flow_field_based_motion_planner_amd.config import FFMPConfig
    from tests.test_gpu_scan_match import _mixed_rows, _planes, _poses
    config = FFMPConfig(grid=64, n_obst=0, n_beams=0)
    res = config.res
    wh = cells * res / 2.0
    rm = (np.inf if L == 1 else 0.6 * wh if L == 7 else 0.45 * wh) if range_max is None else range_max
    pose = _poses(wh, res, NP, seed)
    rows = _mixed_rows(NP, L, min(1.2 * wh, 4.0), seed + 1)
    if L == 1:
        rows[:, 0] = np.resize(np.array([0.4 * wh, np.inf, np.nan, -np.inf, 0.0, -0.7, 0.1 * wh], F32), NP)
    return config, Cfg.from_config(config), _planes(NP, cells, seed + 2), rows, pose, rm


# ---------------------------------------------------------------- the physical tie
def kidnapped(seed: int, n: int, moving: bool = False, steps: int = 30):
    """Rooms mapped over `steps` random steps exactly as scan_match_ref.single_shot maps them, then no prior: the pose
    is the plane's centre with yaw 0, the window the whole plane and the full circle.  A dict of the call's inputs
    (config, cfg, m, ranges, pose, R, T, dtheta, range_max, min_valid), the true poses and the kept envs."""
    from oracle.ffmp_oracle import OracleVecEnv
    config = SM.tie_config(**(dict(moving=True, obst_vmax=0.5) if moving else {}))
    cfg = Cfg.from_config(config)
    Wc = W.default_cells(config) + 24
    env = OracleVecEnv(config, n, with_potential=False)
    env.reset()
    rng = np.random.default_rng(seed)
    m = np.zeros((n, Wc, Wc), np.int8)
    alive = np.ones(n, bool)
    episode = env.episode.copy()
    for k in range(steps + 1):
        if k:
            env.step(rng.integers(0, 28, n))
            alive &= (env.episode == episode) & (env.record[:, 10] == 0)
        if k < steps:
            m = W.from_config(config, m, env.lidar, env.record[:, 0:4], first=np.full(n, k == 0))
    T = 45
    pose = np.tile(np.array([[0.0, 0.0, 1.0, 0.0]], F32), (n, 1))
    return dict(config=config, cfg=cfg, m=m, ranges=np.asarray(env.lidar, F32).copy(), pose=pose, R=Wc // 2, T=T,
                dtheta=2.0 * math.pi / (2 * T + 1), range_max=float(config.lidar_range), min_valid=max(8, env.lidar.shape[1] // 6),
                true=env.record[:, 0:4].astype(F32), alive=alive, cells=Wc)


def kidnapped_call(s: dict) -> dict:
    """The keyword arguments of relocalize() / exhaustive() for a kidnapped() scene."""
    return dict(cfg=s["cfg"], m=s["m"], ranges=s["ranges"], pose=s["pose"], R=s["R"], T=s["T"], dtheta=s["dtheta"],
                range_max=s["range_max"], min_valid=s["min_valid"])


def kidnapped_errors(s: dict, pose_out: np.ndarray):
    """(position error in cells (kept,), yaw error in rotation steps (kept,))."""
    d, yaw = SM.pose_errors(pose_out, s["true"])
    return d[s["alive"]] / float(s["config"].res), yaw[s["alive"]] / s["dtheta"]


if __name__ == "__main__":
    for seed, n, moving in ((1, 6, False), (2, 8, False), (3, 8, False), (4, 8, True)):
        s = kidnapped(seed, n, moving)
        for B in (8, 16):
            pose_out, info, U = relocalize(B=B, **kidnapped_call(s))
            d, yaw = kidnapped_errors(s, pose_out)
            total = U[0].size
            print(f"seed {seed} n {n} {'moving' if moving else 'static'} B {B}: kept {int(s['alive'].sum())}, status "
                  f"{info[s['alive'], 0].tolist()}, position error max {d.max():.2f} cells, yaw error max {yaw.max():.2f} steps, "
                  f"refined {info[s['alive'], 7].min()}..{info[s['alive'], 7].max()} of {total} blocks "
                  f"({100 * info[s['alive'], 7].max() / total:.3f} %)", flush=True)
