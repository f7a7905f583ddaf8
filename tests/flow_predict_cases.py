"""The planes, knob sets and sizes of the predicted-frame comparisons (include/ffmp.h ffmp_flow_predict, DESIGN
§5.14): shared by tests/test_gpu_flow_predict.py, which runs them on the GPU, and tests/test_flow_predict_host.py,
which proves on the restatement (tests/flow_predict_ref.py) that every case puts bits where it is meant to.
Nothing here needs a GPU.

The size ladder (G, n):
    100  the half-used last word of the bit plane (G*G % 32 = 16)        128  C2's grid
    256  C3's grid (n = 3, and 70 once)                                  260  no power of two, G*G % 32 = 16
    404  the largest grid on the default cap of dynamic LDS (65,304 B)   408  the smallest that opts in (66,520 B)
    508  opt-in with the half-used last word (100,872 B)                 512  the maximum (102,400 B)
The knob sets, on top of KNOBS:
    open      steps 24, slack -1: no gate, bits over the whole plane
    far       steps 64, slack 3, pace ceil(7 * (G // 2) / 64): the arrival time at the corner is about the horizon,
              so the gate passes some targets and refuses others out to the border
    default   KNOBS: the gate passes nothing further than about 33 cells from the robot cell
The densities: `listed` keeps every env below FFMP_PRED_LIST = 1,024 moving sources (the LDS list takes them all),
`overflow` puts every env above it (the lanes that find the list full walk their own)."""
import functools

import numpy as np

F32 = np.float32
KNOBS = dict(steps=24, cps=F32(2.0), pace=6, slack=3, swept=254, other=128)
FORMATS = [(np.float32, np.float32), (np.float32, np.float16), (np.uint8, np.float32), (np.uint8, np.float16)]
ENDS = [(np.float32, np.float32), (np.uint8, np.float16)]
LIST = 1024  # FFMP_PRED_LIST
LADDER = [(100, 3), (128, 3), (256, 3), (260, 3), (404, 2), (408, 2), (508, 2), (512, 2)]
SIZES = [g for g, _ in LADDER]
MANY = (256, 70)
# two of the 15 grids at which the kernel's float quotient (float)q * (1.0f / G) truncates to q / G - 1 for some flat
# cells q (all of them multiples of G: column 0), so that its `++i` correction runs: one on each side of the LDS cap.
# No grid in 8..512 needs the `--i` one, and no ladder size needs either (uncorrected_cells, asserted on the host).
CORRECTED = [(244, 3), (460, 2)]


def uncorrected_cells(G):
    """(too high, too low): the flat cells q < G*G whose float32 quotient, truncated, is above / below q // G."""
    q = np.arange(G * G)
    i0 = (q.astype(F32) * (F32(1.0) / F32(G))).astype(np.int64)
    return q[i0 * G > q], q[(i0 + 1) * G <= q]


def lds_bytes(G):
    """Dynamic LDS of one workgroup, the source's formula: bits, cls and the list, 4 bytes each."""
    return 4 * ((G * G + 31) // 32 + G * G // 16 + LIST)


def planes(G, n, seed, cps=2.0, dense=False, density=0.03):
    """(frame float32 with values a uint8 holds, flow float32): `density` sources and 3 % other occupied cells, flows
    within +-2 cells per step, special values sprinkled over the flow, outward sources on the borders."""
    rng = np.random.default_rng(seed)
    u = rng.random((n, G, G))
    frame = np.zeros((n, G, G), F32)
    frame[u < density] = 255
    other = (u >= density) & (u < density + 0.03)
    frame[other] = rng.integers(1, 255, int(other.sum()))
    if dense:
        frame[:] = 255
    flow = (rng.uniform(-2.0, 2.0, (n, 2, G, G)) / cps).astype(F32)
    # the borders: every fourth cell a source that points outward (and sideways)
    frame[:, 0, ::4] = frame[:, G - 1, 1::4] = frame[:, 2::4, 0] = frame[:, 3::4, G - 1] = 255
    flow[:, 0, 0, ::4] = -np.abs(flow[:, 0, 0, ::4]) - F32(0.3)
    flow[:, 0, G - 1, 1::4] = np.abs(flow[:, 0, G - 1, 1::4]) + F32(0.3)
    flow[:, 1, 2::4, 0] = -np.abs(flow[:, 1, 2::4, 0]) - F32(0.3)
    flow[:, 1, 3::4, G - 1] = np.abs(flow[:, 1, 3::4, G - 1]) + F32(0.3)
    s = rng.random((n, 2, G, G))
    flow[s < 0.01] = np.nan
    flow[(s >= 0.01) & (s < 0.02)] = np.inf
    flow[(s >= 0.02) & (s < 0.03)] = -np.inf
    flow[(s >= 0.03) & (s < 0.06)] = -0.0
    flow[(s >= 0.06) & (s < 0.08)] = 0.0
    flow[(s >= 0.08) & (s < 0.09)] = 3e38
    return frame, flow


def f32_only(frame):
    """A copy with the values only a float32 frame can hold on rows 1..4."""
    f32 = frame.copy()
    f32[:, 1, 1::5] = np.nan
    f32[:, 2, 1::5] = -4.0
    f32[:, 3, 1::5] = 0.25
    f32[:, 4, 1::5] = 255.5
    return f32


def density(which, G):
    """The source density of a ladder case: 3 % is 2,231 moving sources per env at 256 x 256 and about 570 at
    128 x 128; the small grids need 15 % / 10 % to overflow the list, the large ones 0.1 % to stay on it."""
    if which == "listed":
        return 0.03 if G <= 128 else 0.001
    assert which == "overflow"
    return 0.15 if G <= 100 else 0.10 if G <= 128 else 0.03


def knobs(which, G):
    """The overrides of KNOBS for a knob set."""
    if which == "open":
        return dict(steps=24, slack=-1)
    if which == "far":
        return dict(steps=64, slack=3, pace=-(-7 * (G // 2) // 64))
    assert which == "default"
    return {}


# at 0.1 % only about every second seed sends a source into the last 16 flat cells: the first that does, per size
LISTED_SEED = {100: 100503, 128: 128503, 256: 256504, 260: 260503, 404: 404505, 408: 408502, 508: 508503, 512: 512504}


@functools.lru_cache(maxsize=None)
def case_planes(G, n, which):
    """(frame, flow) of a ladder case, read-only: one seed per (G, n, density), the same planes for every knob set."""
    frame, flow = planes(G, n, seed=LISTED_SEED[G] if which == "listed" else 1000 * G + n, density=density(which, G))
    frame.setflags(write=False)
    flow.setflags(write=False)
    return frame, flow


def cast(frame, flow, ft, vt):
    """The planes in a frame x flow format pair; a float32 frame gets f32_only's values.  3e38 is inf in binary16."""
    with np.errstate(over="ignore"):
        return (f32_only(frame) if ft is np.float32 else frame.astype(ft)), flow.astype(vt)


def moving_sources(frame, flow, cps=KNOBS["cps"]):
    """Per env, the number of sources by the kernel's own rule: frame == 255, both displacements (one float32
    multiply by cps each) finite and not both zero."""
    with np.errstate(all="ignore"):
        su = flow[:, 0].astype(F32) * F32(cps)
        sv = flow[:, 1].astype(F32) * F32(cps)
        moves = np.isfinite(su) & np.isfinite(sv) & ~((su == 0) & (sv == 0))
        return ((np.asarray(frame) == 255) & moves).sum(axis=(1, 2))


# what tests/test_gpu_flow_predict.py runs on the ladder: (knob set, density, formats, sizes)
GPU_LADDER = [("open", "overflow", FORMATS, SIZES), ("far", "overflow", ENDS, SIZES), ("far", "listed", ENDS, SIZES),
              ("open", "listed", ENDS, SIZES), ("default", "overflow", ENDS[:1], [256, 512])]
