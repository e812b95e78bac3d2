"""ORACLE / TEST INFRASTRUCTURE — the scalar index obs of grid Ant-Tag (csrc/anttag.hip header, gp_anttag_config
obs_index = 1) computed from the state of an `oracle.anttag.AntTagOracle`, independently of the vector
obs: with nc = size * size,

    obs = ant_cell * (nc + 1) + (target_cell if d^2 < visible_radius2 else nc)

The oracle's reset and step are used as they are (transitions, draws, rewards and flags do not depend on the obs kind);
only the obs they return is replaced.
"""
import numpy as np


def index_obs(ora):
    """int32 [B]: the index obs of the state `ora` is in."""
    N = ora.N
    nc = N * N
    ay, ax = np.divmod(ora.ant, N)
    ty, tx = np.divmod(ora.target, N)
    visible = (ay - ty) ** 2 + (ax - tx) ** 2 < ora.vis_r2
    return (ora.ant * (nc + 1) + np.where(visible, ora.target, nc)).astype(np.int32)


class IndexObs:
    """An AntTagOracle whose reset / step return the index obs (every other attribute is the oracle's)."""

    def __init__(self, ora):
        self.ora = ora

    def __getattr__(self, name):
        return getattr(self.ora, name)

    def obs(self):
        return index_obs(self.ora)

    def reset(self, dr):
        self.ora.reset(dr)
        return self.obs()

    def step(self, actions, dr):
        _, rew, term, trunc = self.ora.step(actions, dr)
        return self.obs(), rew, term, trunc
