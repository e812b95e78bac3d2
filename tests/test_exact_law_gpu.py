"""GPU tests of the closed-loop rollouts against exact policy evaluation (tests/exact_law.py): after
reset(seed), set_controller and rollout_controller(K), the per-step histogram of the controller table cells is
Multinomial(B, p_k) under the exact law of the chain that the handle's integer tables and the controller's thresholds
define, and every entry of controller_statistics and metrics is an unbiased estimate of its exact value. The reference
shares nothing with the kernels or their numpy oracles; every bound is in `exact_law.assert_law`, and the numpy oracles
pass the same cases at the same (seed, B, K) in tests/test_exact_law_cpu.py. This file adds the exact identities.

Three kernels: the tabular POMDP (csrc/pomdp.hip; scanned and searched rows, the model and the table in LDS and in
global memory), RockSample (csrc/rocksample.hip, lowered to tables by `exact_law_cases.rocksample_tables`) and grid
Heaven-Hell (csrc/heavenhell.hip, lowered by the product's `heaven_hell_pomdp`). Only the [K, cells] histogram, the two
statistics tables and the four metrics come to the host.
"""
import numpy as np
import pytest

import exact_law
from exact_law_cases import CASES, GAMMA, SEED

pytestmark = pytest.mark.gpu


def host(x):
    return x.cpu().numpy()


def assert_same_tables(case, env):
    """The handle is configured with the very tables the exact law was computed from."""
    if case.kind == "pomdp":
        for got, want in zip((env.trans_thr, env.obs_thr, env.start_thr, env.reset_obs_thr), case.model.tables):
            assert np.array_equal(got, want)
        assert np.array_equal(env.reward, case.model.R) and np.array_equal(env.terminal, case.model.terminal)
    elif case.kind == "rocksample":
        assert np.array_equal(env.sensor_thresholds, case.spec.thr) and env.obs_type == case.model_name
    else:
        from exact_law_cases import hh_stand_in
        twin = hh_stand_in(*case.model_name, case.time_limit)
        assert np.array_equal(env.flags, twin.flags) and env.keep_thr == twin.keep_thr
        assert np.array_equal(env.obs_base, twin.obs_base) and env.rewards == twin.rewards
    assert env.time_limit == case.time_limit


class Run:
    """One case, run once on the device: the procedure of every case."""

    def __init__(self, name):
        import torch
        case = CASES[name]
        B, K, M = case.B, case.K, case.M
        env = case.make_env(B)
        assert_same_tables(case, env)
        O, A = int(env.single_observation_space.n), int(env.single_action_space.n)
        assert (O, A) == (case.model.O, case.model.A)
        case.install_controller(env)
        self.lds = (env.query("pomdp_lds") if case.kind == "pomdp" else None, env.query("controller_lds"))
        obs0 = env.reset(seed=SEED)[0]
        planes = env.rollout_controller(K)
        self.stats = {k: host(v) for k, v in env.controller_statistics(planes, obs0, gamma=GAMMA).items()}
        self.metrics = env.metrics()
        before = torch.cat((obs0[None], planes["obs"][:-1])).long()
        after = torch.cat((planes["nodes"][1:], env.controller_nodes[None])).long()
        ended = planes["term"] | planes["trunc"]
        cells = M * O * A * (M + 1)
        cell = ((planes["nodes"].long() * O + before) * A + planes["actions"].long()) * (M + 1)
        cell += torch.where(ended, torch.full_like(after, M), after)
        cell += torch.arange(K, device=cell.device)[:, None] * cells
        self.hist = host(torch.bincount(cell.reshape(-1), minlength=K * cells)).reshape(K, cells)
        self.ended = int(ended.sum())
        env.check()


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_samples_the_exact_law(name, gpu_device):
    run, case = Run(name), CASES[name]
    B, K = case.B, case.K
    if name in ("m5", "tiger"):
        assert run.lds == (1, 1)
    if name == "m5_global":
        assert run.lds == (0, 0)
    # the exact identities
    counts = run.stats["counts"].reshape(-1)
    assert np.array_equal(counts, run.hist.sum(0)) and counts.sum() == B * K
    assert run.metrics["env_steps"] == B * K and run.metrics["episodes"] == run.ended
    # the law
    rep = exact_law.assert_law(run.hist, run.metrics, run.stats, case.exact(), B)
    print(f"\n{name}: B = {B}, " + ", ".join(f"{k} {v:.3g}" for k, v in rep.items()))
    assert rep["cells"] >= 100
