"""Env classes mirroring `gym_po.envs` (gym_po/envs/__init__.py:1-4)."""
from .rooms import CRoomsEnv, MultistoryFourRoomsEnv, RoomsEnv
from .extended_taxi import (EXTENDED_TAXI_MAP, TAXI_MAP, ExtendedHansenTaxiVecEnv, ExtendedTaxiVecEnv,
                            HansenTaxiVecEnv, TaxiVecEnv)
from .ant_tag_grid import AntTagGridEnv, ant_tag_obs_index, ant_tag_obs_vector
from .car_flag import CarVecEnv, DiscreteActionCarVecEnv
from .rocksample import RockSample, rocksample_sensor_thresholds
from .heaven_hell_grid import HeavenHellGridEnv, heaven_hell_maze
from .tabular_pomdp import TabularPOMDPEnv, heaven_hell_pomdp, row_thresholds

__all__ = ["RoomsEnv", "CRoomsEnv", "MultistoryFourRoomsEnv", "TaxiVecEnv", "HansenTaxiVecEnv",
           "ExtendedTaxiVecEnv", "ExtendedHansenTaxiVecEnv", "TAXI_MAP", "EXTENDED_TAXI_MAP", "AntTagGridEnv",
           "ant_tag_obs_index", "ant_tag_obs_vector", "CarVecEnv", "DiscreteActionCarVecEnv", "RockSample",
           "rocksample_sensor_thresholds", "HeavenHellGridEnv", "heaven_hell_maze", "TabularPOMDPEnv",
           "heaven_hell_pomdp", "row_thresholds"]
