"""ffmp_temporal_maps called through the C ABI on synthetic buffers, against a NumPy gather written here:

    out[e, c] = frames[lag[d] + e * env_stride : ... + plane],  d = min(k-1-c, max(since[e], 0))

and d = k-1-c with since = NULL.  Bit-exact: the kernel copies.  The frame store holds random bytes, so one
misplaced 16-byte vector shows; `out` is a 16-byte-aligned slice of a larger sentinel-filled buffer whose bytes
before and after it must keep the sentinel, and the frame store must come back unchanged.

The planes, in 16-byte vectors (a block moves 1024 of them, a thread 4 that lie 256 apart): 1, 4 (one thread's
worth, or less), 255 / 256 / 257 (around one unrolled step of a block), 625 (a uint8 plane at G = 100: the third
step partly taken), 1023 / 1024 / 1025 (around one block), 2500 (a float32 plane at G = 100: 3 blocks, the last
holds 452), 10000 (a float32 BEV image at G = 100).  Each is run at elem_bytes 1, 2 and 4; k, n, the stride, the
lag layout and `since` cycle over the 33 (plane, elem_bytes) pairs with periods chosen so that every (k, stride)
and every (n, since) combination occurs; PAIR adds the contiguous [older, newest] layout of a window of 2, whose
lag offsets are smaller than the env stride."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from flow_field_based_motion_planner_amd import _abi

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

VECTORS = [1, 4, 255, 256, 257, 625, 1023, 1024, 1025, 2500, 10000]
KS, NS, SINCE, LAGS = [1, 2, 3, 16], [1, 3, 70], ["null", "old", "mixed"], ["ring", "repeat"]
GUARD, SENTINEL = 4096, 0xA5


def _grid():
    out = []
    for i, (vec, eb) in enumerate(itertools.product(VECTORS, (1, 2, 4))):
        out.append((vec, eb, KS[i % 4], NS[i % 3], bool((i // 3) % 2), LAGS[(i // 2) % 2], SINCE[(i // 3) % 3]))
    return out


GRID = _grid()
# the contiguous pair: offsets [plane, 0], env stride 2 * plane (padded once)
PAIR = [(625, 1, 2, 70, False, "pair", "mixed"), (2500, 4, 2, 3, False, "pair", "mixed"),
        (1, 2, 2, 70, False, "pair", "null"), (257, 2, 2, 3, True, "pair", "old"),
        (1025, 1, 2, 1, False, "pair", "mixed")]
# the deepest series with many envs of different ages, and the same on the smallest planes
DEEP = [(257, 4, 16, 70, True, "ring", "mixed"), (4, 1, 16, 70, False, "repeat", "mixed"),
        (1, 2, 3, 70, True, "ring", "mixed")]


def test_grid_covers_what_it_claims():
    """Every elem_bytes sees a one-vector plane, a plane ragged inside the unrolled step and a ragged multi-block
    one; every k with both strides; every n with every kind of `since`; both lag layouts at k > 1."""
    for eb in (1, 2, 4):
        mine = {c[0] for c in GRID if c[1] == eb}
        assert mine == set(VECTORS)
    assert {(c[2], c[4]) for c in GRID} == set(itertools.product(KS, (False, True)))
    assert {(c[3], c[6]) for c in GRID} == set(itertools.product(NS, SINCE))
    assert {c[5] for c in GRID if c[2] > 1} == set(LAGS)
    assert {c[2] for c in GRID if c[6] == "mixed"} == set(KS)


def _lag_slots(kind, k, rng):
    """(slots of lag 0 .. k-1, slots in the store)."""
    if kind == "ring":  # shuffled ring slots: not monotonic, one slot of the store never read
        return rng.permutation(k + 1)[:k], k + 1
    s = rng.permutation(k + 1)[:k]  # a repeated slot: lag k-1 reads what lag 0 reads
    if k > 1:
        s[k - 1] = s[0]
    return s, k + 1


def case_data(vec, eb, k, n, padded, lags, since):
    """(store bytes, lag byte offsets, env stride in bytes, since or None, want (n, k, plane bytes)) of a case."""
    rng = np.random.default_rng([vec, eb, k, n, int(padded)])
    plane_b = 16 * vec
    if lags == "pair":
        env_b = 2 * plane_b + (16 if padded else 0)
        lag_b = np.array([plane_b, 0], np.int64)
        store_b = n * env_b
    else:
        env_b = plane_b + (16 if padded else 0)
        slots, S = _lag_slots(lags, k, rng)
        lag_b = slots.astype(np.int64) * n * env_b
        store_b = S * n * env_b
    # every byte the kernel may read lies inside the store
    assert int(lag_b.max()) + (n - 1) * env_b + plane_b <= store_b
    store = rng.integers(0, 256, store_b, dtype=np.uint8)
    if since == "null":
        sv = None
        lagd = np.broadcast_to(k - 1 - np.arange(k), (n, k))
    else:
        sv = (np.full(n, k, np.int32) + rng.integers(0, 3, n, dtype=np.int32) if since == "old"
              else rng.integers(-2, k + 3, n, dtype=np.int32))
        lagd = np.minimum(k - 1 - np.arange(k)[None, :], np.maximum(sv, 0)[:, None])
    want = np.empty((n, k, plane_b), np.uint8)
    for e in range(n):
        for c in range(k):
            at = int(lag_b[lagd[e, c]]) + e * env_b
            want[e, c] = store[at:at + plane_b]
    return store, lag_b, env_b, sv, want


@pytest.mark.parametrize("vec,eb,k,n,padded,lags,since", GRID + PAIR + DEEP,
                         ids=lambda v: str(int(v)) if isinstance(v, (bool, int)) else v)
def test_temporal_maps_equal_a_numpy_gather(vec, eb, k, n, padded, lags, since):
    store, lag_b, env_b, sv, want = case_data(vec, eb, k, n, padded, lags, since)
    plane_b, store_b = 16 * vec, store.size

    # frames and out at addresses that are 16-byte aligned and no more
    fbuf = torch.full((store_b + 32,), SENTINEL, dtype=torch.uint8, device=DEV)
    frames = fbuf[16:16 + store_b]
    frames.copy_(torch.from_numpy(store))
    out_b = n * k * plane_b
    obuf = torch.full((out_b + 2 * GUARD + 16,), SENTINEL, dtype=torch.uint8, device=DEV)
    out = obuf[GUARD + 16:GUARD + 16 + out_b]
    assert frames.data_ptr() % 32 == 16 and out.data_ptr() % 32 == 16
    sd = None if sv is None else torch.from_numpy(sv).to(DEV)
    lag = (C.c_int64 * k)(*[int(b) // eb for b in lag_b])
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _abi.check(_abi.load().ffmp_temporal_maps(n, frames.data_ptr(), lag, k, env_b // eb, plane_b // eb, eb,
                                              None if sd is None else sd.data_ptr(), out.data_ptr(), stream),
               "ffmp_temporal_maps")
    torch.cuda.synchronize()
    got = obuf.cpu().numpy()
    body = got[GUARD + 16:GUARD + 16 + out_b].reshape(n, k, plane_b)
    bad = np.argwhere((body != want).any(axis=2))
    assert bad.size == 0, f"(env, channel) mismatches {bad[:8].tolist()}, since {None if sv is None else sv[:8].tolist()}"
    assert (got[:GUARD + 16] == SENTINEL).all(), "bytes before out were written"
    assert (got[GUARD + 16 + out_b:] == SENTINEL).all(), "bytes after out were written"
    fgot = fbuf.cpu().numpy()
    assert np.array_equal(fgot[16:16 + store_b], store), "the frame store was written"
    assert (fgot[:16] == SENTINEL).all() and (fgot[16 + store_b:] == SENTINEL).all()
