"""The mixed-ages runs of tests/series_cases.py on the NumPy oracle alone (no GPU): every (config, n, steps, action
seed) a GPU test of the frame series steps ends at least n episodes by something other than the max_steps
truncation, shows at least 4 distinct episode ages across the envs at some step, and leaves at least 5 % of the
newest frames' cells occupied.  These are conditions on the inputs: a run that misses one tests nothing about the
per-env clamp of ffmp_temporal_maps or the replay memory's s_since, whatever the GPU computes.

Measured on the oracle (resets, not truncations, most distinct ages, occupied G100 / G36 / G12 / G8):
    n 24, 22 steps, seed 3:            125, 57, 6, 0.29 / 0.16 / 0.10 / 0.11
    n 16, 7 steps, seed 5, no limit:    20, 20, 6, 0.25 / 0.15 / 0.08 / 0.09
    n 24, 18 steps, seed 4, flow:       95, 47, 6, 0.28 / 0.17 / 0.10 / 0.11
    n 32, 11 steps, seed 2:             68, 37, 6, 0.28 / - / 0.09 / -
    n 24, 9 steps, seed 6 (G12):        48, 28, 6, 0.09
"""
import pytest

from tests import series_cases as S


def test_configs_are_the_stated_grids():
    assert {name: c.grid for name, c in S.SERIES.items()} == {"G100": 100, "G36": 36, "G12": 12, "G8": 8}
    for name, c in S.SERIES.items():
        assert c.n_beams <= 32 and c.moving and c.max_steps == 6 and not c.flow and S.SERIES_FLOW[name].flow
        assert S.SERIES_FLOW[name].replace(flow=False) == c
    # the plane sizes in 16-byte vectors the grids were chosen for
    assert [S.SERIES[g].grid ** 2 // 16 for g in ("G100", "G36", "G12", "G8")] == [625, 81, 9, 4]
    assert 100 * 100 * 4 // 16 == 2500 and 2500 - 2 * 1024 == 452 and 4 * 12 * 12 * 4 // 16 == 144


@pytest.mark.parametrize("name,flow,n,steps,seed", S.RUNS, ids=lambda v: str(v))
def test_runs_mix_episode_ages(name, flow, n, steps, seed):
    cfg = S.config(name, flow)
    if (n, steps, seed) == S.MASKED_RUN:
        cfg = cfg.replace(max_steps=0)  # test_temporal_maps_masked_reset_and_reload runs without the step limit
    resets, early, ages, occupied = S.age_mix(cfg, n, steps, seed)
    print(f"{name} flow={flow} n={n} steps={steps} seed={seed}: resets {resets}, not truncations {early}, "
          f"most distinct ages {ages}, occupied {occupied:.3f}")
    assert early >= n, (early, n)
    assert ages >= S.MIN_AGES, ages
    assert occupied >= S.MIN_OCCUPIED, occupied
    assert resets > early or cfg.max_steps == 0  # truncations happen too: both kinds of reset are exercised
