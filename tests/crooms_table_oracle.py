"""Test helpers shared by the C-ROOMS tests (test_crooms_gpu.py, test_crooms_table_cpu.py, test_crooms_table_gpu.py)
and the fixture generator (tests/golden/make_golden.py run_crooms_table): the oracle (oracle/crooms.py) set to the
rows of a `crooms_table` fixture, the capture of the reference stream's values per env for the device's replay mode,
and the PCG64 state in the six words the fixtures store.
"""
import numpy as np

from oracle.crooms import CRoomsOracle
from oracle.draws import NumpyDraws


class RecordingDraws(NumpyDraws):
    """The reference's numpy calls (NumpyDraws) + per-env capture of every value for GPU replay."""

    def __init__(self, gen, B, valid):
        super().__init__(gen)
        self.B, self.valid, self.rec = B, valid, {}

    def uniform(self, n):
        u = super().uniform(n)
        self.rec["u"] = np.round(u * 2.0 ** 53).astype(np.uint64)  # random() = k * 2^-53 exactly
        return u

    def choice(self, values, mask, site):
        v = super().choice(values, mask, site)
        idx = np.zeros(self.B, np.int32)
        idx[mask] = np.searchsorted(self.valid, v)
        self.rec[site] = idx
        return v

    def record_normal(self, site, mask, v):
        arr = np.zeros((self.B, 2), np.float64)
        arr[mask] = v
        self.rec[site] = arr


def replay_args(rec, B):
    """The keyword arguments of CRoomsEnv.set_replay from one step's RecordingDraws.rec."""
    z2 = np.zeros((B, 2))
    return dict(u=rec.get("u", np.zeros(B, np.uint64)), goal_idx=rec.get("goal", np.zeros(B, np.int32)),
                agent_idx=rec.get("agent", np.zeros(B, np.int32)), noise=rec.get("noise", z2),
                wall_noise=rec.get("wall_noise", z2))


def ctor_kwargs(kw):
    kw = dict(kw)
    for k in ("goal_xy", "agent_xy"):
        if kw.get(k) is not None:
            kw[k] = tuple(kw[k])
    return kw


class TableOracle(CRoomsOracle):
    """CRoomsOracle that keeps what one step decided: the effective move (action * action_power, after the
    action-failure draw), the out-of-bounds flags and the position after the move and before any reset."""

    def _apply_action(self, a, draws):
        self.last_move = np.array(a, dtype=np.float64)
        self.last_oob = super()._apply_action(a, draws)
        self.last_pos = self.agent.copy()
        return self.last_oob


def rng6(gen):
    st = gen.bit_generator.state
    m = (1 << 64) - 1
    return [st["state"]["state"] >> 64, st["state"]["state"] & m, st["state"]["inc"] >> 64, st["state"]["inc"] & m,
            int(st["has_uint32"]), int(st["uinteger"])]


def state_of_rng6(v):
    """numpy's PCG64.state dict from the six recorded words."""
    v = [int(x) for x in v]
    return {"bit_generator": "PCG64", "state": {"state": (v[0] << 64) | v[1], "inc": (v[2] << 64) | v[3]},
            "has_uint32": v[4], "uinteger": v[5]}


def set_rows(ora, data):
    """Overwrite the oracle's state with the table's recorded input rows."""
    ora.agent = data["in_agent"].astype(np.float64).copy()
    ora.goal = data["in_goal_cell"].astype(np.float64) + 0.5  # the goal centre ignores cell_size
    ora.velocity = data["in_velocity"].astype(np.float64).copy()
    ora.elapsed = data["in_elapsed"].astype(int).copy()


def table_oracle_step(meta, data, recording=True):
    """The oracle on numpy's Generator at the recorded pre-step state, set to the table's rows, one step.
    Returns (oracle, (obs, rew, term, trunc), draws)."""
    B = meta["num_envs"]
    ora = TableOracle(B, **ctor_kwargs(meta["kwargs"]))
    ora.reset_seed(meta["seed"])
    ora.gen.bit_generator.state = state_of_rng6(data["pre_rng_state"])
    set_rows(ora, data)
    draws = RecordingDraws(ora.gen, B, ora.valid) if recording else NumpyDraws(ora.gen)
    out = ora.step(data["in_action"].copy(), draws)
    return ora, out, draws
