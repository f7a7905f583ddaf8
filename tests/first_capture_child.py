"""The first launch of a process that asks for more than 64 KiB of dynamic LDS, made while a stream is capturing.

ffmp_flow_predict, ffmp_frame_potential and ffmp_scan_flow raise their kernel's cap of dynamic LDS behind a
per-process latch at the first call that needs it (grids of 408 and above).  Inside the suite
some earlier test has always made that call eagerly, so this program is started as a fresh process
(tests/test_gpu_flow_predict.py) and, for each of the three passes, through the C ABI on torch tensors:

1. makes one eager call at grid 64 on the current stream — the code object is loaded, the latch untouched;
2. captures one call at grid 512 into a torch.cuda.CUDAGraph, the capturing stream as the stream argument;
3. replays the graph onto poisoned outputs;
4. compares with the pass's restatement (tests/flow_predict_ref.py, tests/frame_potential_ref.py,
   tests/scan_flow_ref.py), bit for bit.

It prints one JSON line per pass, {"pass": ..., "outcome": "match" | "refused" | "mismatch" | "error", ...}, stops at
the first pass that does not match, and exits 0 only when all three match.

    python tests/first_capture_child.py
"""
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

F32 = np.float32
DEV = "cuda:0"
SMALL, LARGE = 64, 512


def _t(x):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x)).to(DEV)


def _cfg(G):
    from flow_field_based_motion_planner_amd.config import FFMPConfig
    return FFMPConfig(grid=G, n_obst=1, n_beams=0)


class Predict:
    """ffmp_flow_predict, float32 frame and flow: the open x overflow case of tests/flow_predict_cases.py."""
    name = "ffmp_flow_predict"

    def __init__(self, G):
        import torch
        from tests import flow_predict_cases as K
        from tests import flow_predict_ref as R
        self.G, self.n = G, 2
        self.knobs = dict(K.KNOBS, **K.knobs("open", G))
        frame, flow = K.cast(*K.planes(G, self.n, seed=G, density=K.density("overflow", G)), np.float32, np.float32)
        self.exp = dict(zip(("out", "n_swept"), R.flow_predict(frame, flow, **self.knobs)))
        assert self.exp["n_swept"].sum() > 0
        self.frame, self.flow = _t(frame), _t(flow)
        self.got = dict(out=torch.full((self.n, G, G), 7, dtype=torch.uint8, device=DEV),
                        n_swept=torch.full((self.n,), -1, dtype=torch.int32, device=DEV))

    def launch(self, lib, stream):
        from flow_field_based_motion_planner_amd import _abi
        cfg, k, G2 = _abi.make_cfg(_cfg(self.G)), self.knobs, self.G * self.G
        return lib.ffmp_flow_predict(C.byref(cfg), self.n, self.frame.data_ptr(), G2, _abi.OBS_F32, self.flow.data_ptr(), 2 * G2,
                                     _abi.OBS_F32, None, self.got["out"].data_ptr(), G2, self.got["n_swept"].data_ptr(), int(k["steps"]),
                                     float(k["cps"]), int(k["pace"]), int(k["slack"]), int(k["swept"]), int(k["other"]), stream)


class Potential:
    """ffmp_frame_potential, float32 frame and potential, reach 32 (95,240 bytes of LDS at 512 x 512)."""
    name = "ffmp_frame_potential"

    def __init__(self, G):
        import torch
        from tests import frame_potential_ref as R
        self.G, self.n, self.reach, self.occ_min = G, 2, 32, 255
        rng = np.random.default_rng(G + 1)
        u = rng.random((self.n, G, G))
        frame = np.zeros((self.n, G, G), F32)
        frame[u < 0.03] = 255
        frame[(u >= 0.03) & (u < 0.06)] = 100
        frame[:, 0, ::4] = frame[:, G - 1, 1::4] = frame[:, 2::4, 0] = frame[:, 3::4, G - 1] = 255
        goal = rng.uniform(-3.0, 3.0, (self.n, 2)).astype(F32)
        self.exp = R.frame_potential(frame, goal, _cfg(G), occ_min=self.occ_min, reach=self.reach, dtype=np.float32)
        self.exp = {k: self.exp[k] for k in ("dist2", "potential", "grad", "robot_d2")}
        assert ((self.exp["dist2"] != 65535) & (self.exp["dist2"] != 0)).any()
        self.frame, self.goal = _t(frame), _t(goal)
        self.got = dict(dist2=_t(np.full((self.n, G, G), 7, np.uint16)), potential=torch.full((self.n, G, G), -3.0, device=DEV),
                        grad=torch.full((self.n, 2), -3.0, device=DEV), robot_d2=torch.full((self.n,), -9, dtype=torch.int32, device=DEV))

    def launch(self, lib, stream):
        from flow_field_based_motion_planner_amd import _abi
        cfg, G2, g = _abi.make_cfg(_cfg(self.G)), self.G * self.G, self.got
        return lib.ffmp_frame_potential(C.byref(cfg), self.n, self.frame.data_ptr(), G2, _abi.OBS_F32, self.goal.data_ptr(), 2, None,
                                        self.occ_min, self.reach, g["dist2"].data_ptr(), G2, g["potential"].data_ptr(), G2, _abi.OBS_F32,
                                        g["grad"].data_ptr(), g["robot_d2"].data_ptr(), stream)


class ScanFlow:
    """ffmp_scan_flow, float32 flow (117,120 bytes of LDS at 512 x 512): env 0 a frame moved by (2, -1) cells under the
    identity motion, env 1 two independent frames under a small ego motion."""
    name = "ffmp_scan_flow"

    def __init__(self, G):
        import torch
        from oracle.ffmp_oracle import Cfg
        from tests import scan_flow_ref as R
        self.G, self.n, self.scale, self.knobs = G, 2, F32(0.125), R.KNOBS
        rng = np.random.default_rng(G + 2)
        prev = np.where(rng.random((self.n, G, G)) < 0.05, 255, rng.integers(0, 255, (self.n, G, G))).astype(np.uint8)
        cur = prev.copy()
        cur[0] = np.roll(prev[0], (2, -1), (0, 1))
        cur[1] = np.where(rng.random((G, G)) < 0.05, 255, 0)
        was = np.array([[0, 0, 1, 0], [0.3, -0.2, np.cos(0.5), np.sin(0.5)]], F32)
        now = np.array([[0, 0, 1, 0], [0.35, -0.12, np.cos(0.54), np.sin(0.54)]], F32)
        self.exp = dict(zip(("flow", "kind"), R.scan_flow(Cfg.from_config(_cfg(G)), cur, prev, now, was, self.scale)))
        assert all((self.exp["kind"] == v).any() for v in (0, 1, 2))
        self.cur, self.prev, self.now, self.was = _t(cur), _t(prev), _t(now), _t(was)
        self.got = dict(flow=torch.full((self.n, 2, G, G), 7.0, device=DEV),
                        kind=torch.full((self.n, G, G), 7, dtype=torch.uint8, device=DEV))

    def launch(self, lib, stream):
        from flow_field_based_motion_planner_amd import _abi
        cfg, G2, k = _abi.make_cfg(_cfg(self.G)), self.G * self.G, self.knobs
        return lib.ffmp_scan_flow(C.byref(cfg), self.n, self.cur.data_ptr(), self.prev.data_ptr(), G2, self.now.data_ptr(), 4,
                                  self.was.data_ptr(), 4, None, None, self.got["flow"].data_ptr(), 2 * G2, self.got["kind"].data_ptr(), G2,
                                  0, float(self.scale), k["radius"], k["block"], k["gate"], k["min_hits"], stream)


def _differing(case):
    from tests.frame_potential_ref import same_bits
    return {k: int((~same_bits(case.got[k].cpu().numpy(), v)).sum()) for k, v in case.exp.items()}


def first_capture(lib, kind):
    """One pass: {"pass", "outcome", ...}."""
    import torch
    res = {"pass": kind.name}
    small = kind(SMALL)
    rc = small.launch(lib, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    if rc != 0 or any(_differing(small).values()):
        return dict(res, outcome="error", where="eager call at grid 64", rc=rc, error=lib.ffmp_last_error().decode())
    large = kind(LARGE)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=torch.cuda.Stream(device=DEV)):
        rc = large.launch(lib, torch.cuda.current_stream().cuda_stream)
    if rc != 0:
        return dict(res, outcome="refused", rc=rc, error=lib.ffmp_last_error().decode())
    torch.cuda.synchronize()
    if not any(_differing(large).values()):  # every output still holds its poison: the capture ran nothing
        return dict(res, outcome="error", where="the capture wrote the outputs")
    graph.replay()
    torch.cuda.synchronize()
    bad = _differing(large)
    return dict(res, outcome="mismatch" if any(bad.values()) else "match", differing=bad)


def main():
    import torch
    from flow_field_based_motion_planner_amd import _abi
    lib = _abi.load()
    assert torch.cuda.is_available()
    for kind in (Predict, Potential, ScanFlow):
        try:
            res = first_capture(lib, kind)
        except Exception as exc:  # noqa: BLE001  a capture that was invalidated raises when it ends
            res = {"pass": kind.name, "outcome": "error", "error": f"{type(exc).__name__}: {exc}", "last_error": lib.ffmp_last_error().decode()}
        print(json.dumps(res), flush=True)
        if res["outcome"] != "match":
            return 1  # nothing more is started on the GPU after a failure
    return 0


if __name__ == "__main__":
    sys.exit(main())
