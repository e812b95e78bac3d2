"""CPU tests of the Taxi closed-loop rollouts' test policy (tests/taxi_controller_oracle.py): the threshold rows it
lowers to, and that the conditions the directed GPU case asserts on the device's run hold for the policy's law itself
(the Taxi oracle on numpy's stream, the actions sampled with a numpy Generator). No GPU."""
import numpy as np
import pytest

from gym_po_amd.controller import controller_thresholds
from taxi_controller_oracle import A, marginal_greedy_probs, obs_table, policy_rollout_sampled
from taxi_table_oracle import per_tile_floor, rare_rows

TOP = 1 << 31
DYADIC = dict(reward_goal=2.0, reward_bad=-1.0, reward_any=-0.25)
DIRECTED = dict(map="TAXI", hansen_obs=True, num_passengers=2, time_limit=24, **DYADIC)
B, K = 2051, 48


def test_marginal_policy_is_stochastic_and_covers_the_obs_space():
    probs = marginal_greedy_probs(DIRECTED)
    obs_of, n_obs = obs_table(DIRECTED)
    assert probs.shape == (n_obs, A) == (320, 5)
    np.testing.assert_allclose(probs.sum(1), 1.0, rtol=0, atol=1e-12)
    assert (probs >= 0).all()
    mixed = int(((probs > 0).sum(1) > 1).sum())
    assert mixed == 210  # rows with mass on more than one action: the policy is stochastic
    unmapped = np.setdiff1d(np.arange(n_obs), obs_of)
    assert unmapped.size and (probs[unmapped] == 1.0 / A).all()  # obs values no state maps to: uniform rows


@pytest.mark.parametrize("map", ["TAXI", "EXTENDED"])
def test_threshold_rows_are_valid(map):
    probs = marginal_greedy_probs(dict(DIRECTED, map=map))
    t = controller_thresholds(probs)
    assert t.dtype == np.uint32 and t.shape == (1, probs.shape[0], A)
    t = t[0].astype(np.int64)
    assert (np.diff(t, axis=-1) >= 0).all()                # nondecreasing
    assert (t >= 0).all() and (t[:, -1] == TOP).all()      # within [0, 2^31], ending at 2^31
    widths = np.diff(t, axis=-1, prepend=0)
    assert (probs == 0).any() and (widths[probs == 0] == 0).all()  # zero-probability actions: empty intervals
    assert (widths[probs > 0] > 0).all()


@pytest.mark.parametrize("seed", [3, 7, 11])
def test_law_reaches_every_rare_row_in_every_tile(seed):
    """B = 2,051 envs, K = 48 steps, time_limit = 24, two passengers: what the GPU case asserts with floors of 1
    holds for the law with floors of 100 per full 1,024-env tile."""
    probs = marginal_greedy_probs(DIRECTED)
    ora, outs = policy_rollout_sampled(DIRECTED, B, seed, K, probs, policy_seed=100 + seed)
    rr = rare_rows(ora, outs[1], outs[2], outs[3])
    floor = per_tile_floor(rr)  # (the 3-env last tile is left out)
    print(f"seed {seed}: per-tile minimum {floor}, terminations {int(outs[2].sum())}, "
          f"truncations {int(outs[3].sum())}")
    assert floor["goal"] >= 100 and floor["task"] >= 100, floor
    assert outs[2].any() and outs[3].any()
