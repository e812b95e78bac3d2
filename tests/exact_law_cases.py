"""TEST INFRASTRUCTURE — the cases of the exact-law tests (tests/test_exact_law_cpu.py on the numpy oracles,
tests/test_exact_law_gpu.py on the device) and the lowerings to tables they need: RockSample from the rule text of the
csrc/rocksample.hip header (`rocksample_tables`), Heaven-Hell through the product's `heaven_hell_pomdp`.

A case names a model, a controller, a seed, B and K; both files run it at the same values, so the oracle's pass is
the check, made without a GPU, that the reference stays inside every bound of `exact_law.assert_law`.
"""
import types

import numpy as np

import exact_law

TOP = 1 << 31
GAMMA = 0.95
SEED = 11
ROCKS_232 = ((0, 1), (1, 2))
RS_REWARDS = dict(exit_reward=4.0, good_reward=2.0, bad_reward=-2.0, empty_reward=-1.0, check_reward=-0.25,
                  step_reward=-0.5, wall_reward=-0.75)
HH_REWARDS = dict(heaven_reward=1.0, hell_reward=-1.0, step_reward=-0.25, wall_reward=-0.5)
HH_T3 = ("LPR",
         "#.#",
         "#S#")


def point_rows(index, n):
    """Threshold rows [..., n] of the point masses on `index` [...]: 0 before the index, 2^31 from it on."""
    index = np.asarray(index, dtype=np.int64)
    return np.where(np.arange(n) >= index[..., None], TOP, 0).astype(np.uint32)


def rocksample_tables(sp):
    """RockSample as the integer tables of a tabular POMDP (an `exact_law.Model`). `sp` carries what a handle is
    configured with: H, W, rock_cells, k, init_cell, thr (the uint32 [H * W, k] sensor table), obs_cell, time_limit,
    rewards (the seven, by name).

    States: cell * 2^k + mask, and one absorbing terminal state "exited" (the last). A = 5 + k. N / S / W move inside
    the grid (step_reward) or stay (wall_reward); E the same, except that from the last column it exits (exit_reward).
    SAMPLE on rock i's cell pays good_reward / bad_reward by bit i of the mask and clears it; elsewhere empty_reward.
    CHECK i pays check_reward and reads GOOD with probability thr[cell][i] / 2^31 if bit i is set, else with
    1 - thr[cell][i] / 2^31; every other action reads NULL. Start: init_cell x uniform over the 2^k masks; the first
    obs reads NULL."""
    H, W, k = sp.H, sp.W, sp.k
    n_mask = 1 << k
    S, A = H * W * n_mask + 1, 5 + k
    O = H * W * 3 if sp.obs_cell else 3
    exited = S - 1
    r = sp.rewards
    thr = np.asarray(sp.thr, dtype=np.int64).reshape(H * W, k)
    nxt = np.full((S, A), exited, dtype=np.int64)
    R = np.zeros((S, A, S), dtype=np.float32)
    obs_thr = np.empty((A, S, O), dtype=np.uint32)
    obs_thr[:, exited] = point_rows(np.zeros(A), O)
    for cell in range(H * W):
        row, col = divmod(cell, W)
        base = cell * 3 if sp.obs_cell else 0
        for mask in range(n_mask):
            s = cell * n_mask + mask
            for a, (dr, dc) in enumerate(((-1, 0), (0, 1), (1, 0), (0, -1))):
                rr, cc = row + dr, col + dc
                if a == 1 and col == W - 1:
                    nxt[s, a], rew = exited, r["exit_reward"]
                elif 0 <= rr < H and 0 <= cc < W:
                    nxt[s, a], rew = (rr * W + cc) * n_mask + mask, r["step_reward"]
                else:
                    nxt[s, a], rew = s, r["wall_reward"]
                R[s, a, nxt[s, a]] = rew
            if cell in sp.rock_cells:
                i = list(sp.rock_cells).index(cell)
                nxt[s, 4] = cell * n_mask + (mask & ~(1 << i))
                R[s, 4, nxt[s, 4]] = r["good_reward"] if (mask >> i) & 1 else r["bad_reward"]
            else:
                nxt[s, 4] = s
                R[s, 4, s] = r["empty_reward"]
            obs_thr[:5, s] = point_rows(np.full(5, base), O)  # NULL
            for i in range(k):
                nxt[s, 5 + i] = s
                R[s, 5 + i, s] = r["check_reward"]
                good = int(thr[cell, i]) if (mask >> i) & 1 else TOP - int(thr[cell, i])
                row_thr = point_rows(base + 2, O).astype(np.int64)  # NULL: never; GOOD: [0, good); BAD: the rest
                row_thr[base + 1] = good
                obs_thr[5 + i, s] = row_thr
    nxt[exited] = exited
    trans_thr = point_rows(nxt, S)
    start = np.zeros(S, dtype=np.int64)
    first = sp.init_cell * n_mask
    start[first:first + n_mask] = (np.arange(n_mask) + 1) * (TOP >> k)
    start[first + n_mask:] = TOP
    init_obs = sp.init_cell * 3 if sp.obs_cell else 0
    terminal = np.arange(S) == exited
    return exact_law.Model(trans_thr, obs_thr, start.astype(np.uint32), point_rows(np.full(S, init_obs), O), R,
                           terminal, sp.time_limit)


def controller(M, O, A, seed):
    """The seeded random controller of a case: rng.random(...) ** 2, normalised per row, lowered."""
    from gym_po_amd.controller import controller_thresholds
    p = np.random.default_rng(seed).random((M, O, A, M)) ** 2
    return controller_thresholds(p / p.sum((2, 3), keepdims=True))


def pomdp_tables(name):
    """(T, Z, R, start, terminal, reset_obs) of a tabular case's model."""
    from pomdp_oracle import TIGER, random_model
    if name == "tiger":
        from gym_po_amd import parse_pomdp
        m = parse_pomdp(TIGER)
        return m["T"], m["Z"], m["R"].astype(np.float32), m["start"], np.zeros(2, dtype=bool), np.full((2, 2), 0.5)
    S, A, O = {"m5": (5, 2, 3), "m37": (37, 3, 21)}[name]
    return random_model(S, A, O, seed=S, n_terminal=max(1, S // 8))


def hh_stand_in(obs_type, p, time_limit):
    """What `heaven_hell_pomdp` and the oracle's Spec read of a HeavenHellGridEnv on the "t3" maze, without a GPU."""
    from gym_po_amd.envs.heaven_hell_grid import FLAG_START, hansen_codes, keep_threshold, parse_maze
    H, W, flags = parse_maze(HH_T3)
    cell_obs = obs_type == "cell_signal"
    return types.SimpleNamespace(
        maze=HH_T3, map_size=(H, W), flags=flags, obs_type=obs_type,
        obs_base=np.arange(H * W, dtype=np.int32) if cell_obs else hansen_codes(H, W, flags),
        obs_base_n=H * W if cell_obs else 16, action_failure_probability=float(p), keep_thr=keep_threshold(p),
        start_cells=np.flatnonzero(flags & FLAG_START).astype(np.int32), time_limit=time_limit,
        rewards=dict(HH_REWARDS))


class Case:
    """kind: "pomdp" (model: a name of `pomdp_tables`), "rocksample" (model: the obs type), "heavenhell" (model:
    (obs type, action_failure_probability)). `knobs`: debug knobs of the device run (the oracle has no memory paths)."""

    def __init__(self, kind, model, M, time_limit, K=16, B=1 << 18, ctrl_seed=3, knobs=None):
        self.kind, self.model_name, self.M, self.time_limit, self.K, self.B = kind, model, M, time_limit, K, B
        self.ctrl_seed, self.knobs = ctrl_seed, dict(knobs or {})
        self._built = None

    def _build(self):
        """(the exact_law.Model, the oracle's Spec), made once."""
        if self._built is None:
            if self.kind == "pomdp":
                from gym_po_amd import row_thresholds
                from pomdp_oracle import Spec
                T, Z, R, start, terminal, reset_obs = pomdp_tables(self.model_name)
                spec = Spec(row_thresholds(T), row_thresholds(Z), row_thresholds(start), row_thresholds(reset_obs), R,
                            terminal, self.time_limit)
                model = exact_law.Model(spec.trans_thr, spec.obs_thr, spec.start_thr, spec.reset_obs_thr, spec.reward,
                                        spec.terminal, self.time_limit)
            elif self.kind == "rocksample":
                from gym_po_amd.envs.rocksample import rocksample_sensor_thresholds
                from rocksample_oracle import Spec
                spec = Spec((2, 3), ROCKS_232, (1, 0), rocksample_sensor_thresholds((2, 3), ROCKS_232, 1.5),
                            self.model_name, self.time_limit, **RS_REWARDS)
                model = rocksample_tables(spec)
            else:
                from gym_po_amd import heaven_hell_pomdp, row_thresholds
                from heavenhell_oracle import Spec
                env = hh_stand_in(*self.model_name, self.time_limit)
                spec = Spec.of_env(env)
                T, Z, R, start, terminal, reset_obs = heaven_hell_pomdp(env)
                model = exact_law.Model(row_thresholds(T), row_thresholds(Z), row_thresholds(start),
                                        row_thresholds(reset_obs), R, terminal, self.time_limit)
            self._built = (model, spec)
        return self._built

    @property
    def model(self):
        return self._build()[0]

    @property
    def spec(self):
        return self._build()[1]

    @property
    def thr(self):
        m = self.model
        return controller(self.M, m.O, m.A, self.ctrl_seed)

    def exact(self):
        if not hasattr(self, "_exact"):
            self._exact = exact_law.evaluate(self.model, self.thr, self.K, GAMMA)
        return self._exact

    def oracle(self, B):
        if self.kind == "pomdp":
            from pomdp_oracle import PomdpOracle as Oracle
        elif self.kind == "rocksample":
            from rocksample_oracle import RockSampleOracle as Oracle
        else:
            from heavenhell_oracle import HeavenHellOracle as Oracle
        return Oracle(B, self.spec)

    def install_controller(self, env):
        """set_controller under the case's ctrl_lds_max knob (gp_set_controller reads it), if it has one."""
        from gym_po_amd._lib import debug_knobs
        with debug_knobs(**{k: v for k, v in self.knobs.items() if k == "ctrl_lds_max"}):
            env.set_controller(thresholds=self.thr)

    def make_env(self, B):
        """The device env of the case (GPU tests only), under the case's creation-time knobs."""
        from gym_po_amd._lib import debug_knobs
        with debug_knobs(**{k: v for k, v in self.knobs.items() if k != "ctrl_lds_max"}):
            if self.kind == "pomdp":
                from gym_po_amd import TabularPOMDPEnv
                T, Z, R, start, terminal, reset_obs = pomdp_tables(self.model_name)
                return TabularPOMDPEnv(B, T, Z, R, start=start, terminal=terminal, reset_obs=reset_obs,
                                       time_limit=self.time_limit)
            if self.kind == "rocksample":
                from gym_po_amd import RockSample
                return RockSample(B, map_size=(2, 3), rocks=ROCKS_232, init_pos=(1, 0), obs_type=self.model_name,
                                  time_limit=self.time_limit, half_efficiency_distance=1.5, **RS_REWARDS)
            from gym_po_amd import HeavenHellGridEnv
            return HeavenHellGridEnv(B, maze=HH_T3, obs_type=self.model_name[0],
                                     action_failure_probability=self.model_name[1], time_limit=self.time_limit,
                                     **HH_REWARDS)


CASES = {
    "tiger": Case("pomdp", "tiger", M=3, time_limit=6),                 # rows of 9, padded to 12
    "m5": Case("pomdp", "m5", M=3, time_limit=7),
    "m37": Case("pomdp", "m37", M=2, time_limit=9, K=12),               # searched rows, odd quad count
    "m5_global": Case("pomdp", "m5", M=3, time_limit=7, knobs=dict(pomdp_lds_max=0, ctrl_lds_max=0)),
    "rs_cell": Case("rocksample", "cell_sensor", M=2, time_limit=9),    # A = 7: rows of 14, padded to 16
    "rs_sensor": Case("rocksample", "sensor", M=2, time_limit=9),
    "hh_cell_p13": Case("heavenhell", ("cell_signal", 1 / 3), M=2, time_limit=8),
    "hh_cell_p0": Case("heavenhell", ("cell_signal", 0.0), M=2, time_limit=8),
    "hh_hansen_p13": Case("heavenhell", ("hansen_signal", 1 / 3), M=2, time_limit=8),
    "hh_hansen_p0": Case("heavenhell", ("hansen_signal", 0.0), M=2, time_limit=8),
}
