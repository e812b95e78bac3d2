"""GPU tests of the law of gp_metrics (include/gym_po_amd.h): return_sum is the float64 sum of the float32 rewards of
all env-steps since reset, accumulated in float64 from the thread on, so |return_sum - exact| <= N * 2^-52 * sum|r|
(N env-steps); episodes, length_sum and env_steps are exact integers, 64-bit from the wave shuffle on.

Every other test of the metrics uses dyadic rewards, whose float32 sums are exact in any order. Here no reward is a
short binary fraction (step -0.1, wall -0.3, goal / exit / heaven / tag 0.7, ...; the tabular models take
R = random - 0.3), so a float32 accumulation anywhere between the thread and the slot rounds at every addition and
misses the bound by orders of magnitude: tests/test_metrics_precision_cpu.py shows that at these shapes without a GPU.
Car-Flag's rewards are fixed by its reference (+1, -1, 0); its cases check the counters and the plumbing only.

The reference is tests/metrics_reference.py over the planes the run itself emitted; the env is not restated.

a. B = 1,027 (two 1,024-env tiles, the last quad ragged), K = 257, one case per rollout kernel family, open and closed
   loop, the belief rollout, the grid population kernel (gp_metrics beside the scores), and per kind one grid of one
   block per CU whose blocks loop over two tiles (the accumulator runs on across tiles).
b. The numpy-exact grid kernels (windowed, 4,096- and 512-env blocks; fused), whose epilogues multiply counts by rewards
   once per launch: B = 8,192, launches of 1, 7 and 12 steps.
c. Launches of 65,536 steps with nothing stored, every reward float32(0.1): the exact return is B K float64(0.1f)
   whatever the trajectory; the integers come from a same-seed twin that stores its flags over 64 launches. One
   16,384-step launch with varying rewards against its own rew plane summed on the device.
d. 300 single step() calls: the slot's += across launches.

Not here: a block whose env-steps in one launch pass 2^32 (B = G = 1,024, K = 2^22 + 5, where 32-bit block totals wrap
to 5,120). That launch takes 18 s on an MI355X, too long for this suite; the arithmetic is in the CPU test.
"""
import contextlib
import time

import numpy as np
import pytest

import metrics_reference as mr
from gym_po_amd.controller import controller_thresholds, population_thresholds

pytestmark = pytest.mark.gpu

B, K, SEED, TL = mr.B_SMALL, mr.K_SMALL, 11, 20
F32 = np.float32
MID = ("L..P..R",
       "L.PPP.R",
       "##...##",
       "##.S.##",
       "##S..##")
ROCKS_3 = ((0, 3), (2, 1), (3, 2))


def host(x):
    return x.cpu().numpy()


def knobs_ctx(knobs):
    from gym_po_amd._lib import debug_knobs
    return debug_knobs(**knobs) if knobs else contextlib.nullcontext()


def pomdp_tables(name, constant=None):
    """The m5 / m37 models of tests/test_pomdp_gpu.py with non-dyadic rewards (or one constant reward)."""
    from test_pomdp_gpu import tables
    T, Z, R, start, terminal, reset_obs = tables(name)
    if constant is None:
        R = (np.random.default_rng(R.size).random(R.shape).astype(F32) - F32(0.3)).astype(F32)
    else:
        R = np.full(R.shape, constant, dtype=F32)
    return T, Z, R, start, terminal, reset_obs


def make(kind, num_envs=B, rewards=None, time_limit=TL, **knobs):
    """An env of a kind with the non-dyadic rewards of metrics_reference.REWARDS (`rewards`: every reward that one
    value), created under debug knobs if given."""
    import gym_po_amd as gp
    base = kind.split("_")[0]

    def rw(name):
        r = dict(mr.REWARDS[name])
        return r if rewards is None else {k: float(rewards) for k in r}

    with knobs_ctx(knobs):
        if base == "rocksample":
            return gp.RockSample(num_envs, map_size=(4, 4), rocks=ROCKS_3, init_pos=(1, 0), obs_type="cell_sensor",
                                 time_limit=time_limit, half_efficiency_distance=1.5, **rw("rocksample"))
        if base == "heavenhell":
            return gp.HeavenHellGridEnv(num_envs, maze=MID, obs_type="hansen_signal",
                                        action_failure_probability=1 / 3, time_limit=time_limit, **rw("heavenhell"))
        if base == "anttag":
            return gp.AntTagGridEnv(num_envs, size=4, min_distance=2.0, time_limit=time_limit,
                                    obs_type="vector" if kind == "anttag_vector" else "index", **rw("anttag"))
        if base == "taxi":
            return gp.TaxiVecEnv(num_envs, hansen_obs=True, num_passengers=1, time_limit=time_limit,
                                 rng_mode="numpy" if "numpy" in kind else "philox", **rw("taxi"))
        if base == "crooms":
            return gp.CRoomsEnv(num_envs, layout="1", time_limit=time_limit, action_type="cardinal", obs_type="hansen",
                                rng_mode="numpy" if "numpy" in kind else "philox", **rw("crooms"))
        if base == "carflag":
            return gp.CarVecEnv(num_envs, time_limit=time_limit, rng_mode="philox")
        if base == "pomdp":
            T, Z, R, start, terminal, reset_obs = pomdp_tables(kind.split("_")[1], rewards)
            return gp.TabularPOMDPEnv(num_envs, T, Z, R, start=start, terminal=terminal, reset_obs=reset_obs,
                                      time_limit=time_limit)
        if base == "grid":
            return gp.MultistoryFourRoomsEnv(num_envs, grid_z=1, obs_type="hansen", time_limit=time_limit,
                                             rng_mode="numpy" if "numpy" in kind else "philox", **rw("grid"))
    raise KeyError(kind)


def random_actions(env, n_steps, seed):
    rng = np.random.default_rng(seed)
    space = getattr(env, "single_action_space", None)
    if getattr(space, "n", None) is None:  # Car-Flag: a force
        return rng.uniform(-1.5, 1.5, (n_steps, env.num_envs)).astype(F32)
    return rng.integers(0, int(space.n), (n_steps, env.num_envs)).astype(np.int32)


def random_probs(M, n_obs, A, seed):
    """Rows in which about a third of the entries are exactly 0 and the last joint choice never is."""
    rng = np.random.default_rng(seed)
    p = rng.random((M, n_obs, A, M)) ** 3 * (rng.random((M, n_obs, A, M)) > 0.35)
    p[:, :, A - 1, M - 1] += 0.05
    return p / p.sum((-1, -2), keepdims=True)


def controller_shape(env):
    n_obs = getattr(env, "no", None) or int(env.single_observation_space.n)
    return int(n_obs), int(env.single_action_space.n)


def install_controller(env, M=2, seed=5):
    n_obs, A = controller_shape(env)
    env.set_controller(thresholds=controller_thresholds(random_probs(M, n_obs, A, seed)))


def check_against_planes(env, rew, term, trunc, what, t0, nontrivial=True):
    """The assertion of every stored case: metrics() against the planes the run emitted."""
    big = rew.numel() > mr.FSUM_MAX
    want = mr.want_metrics(*((rew, term, trunc) if big else (host(rew), host(term), host(trunc))))
    got = env.metrics()
    print(f"{what}: {time.perf_counter() - t0:.3f} s to here")
    mr.assert_metrics(got, want, what)
    env.check()
    if nontrivial:
        assert want["episodes"] > 0 and want["length_sum"] >= want["episodes"]
        if type(env).__name__ != "CarVecEnv":  # (its rewards are 0 until a flag is reached)
            assert float(rew.min()) != float(rew.max())  # more than one reward value was paid
    return want


def open_loop(kind, n_steps=K, num_envs=B, **knobs):
    t0 = time.perf_counter()
    env = make(kind, num_envs, **knobs)
    env.reset(seed=SEED)
    _, rew, term, trunc = env.rollout(random_actions(env, n_steps, SEED))
    return env, check_against_planes(env, rew, term, trunc, f"{kind} open loop {knobs or ''}", t0)


def closed_loop(kind, n_steps=K, num_envs=B, **knobs):
    t0 = time.perf_counter()
    env = make(kind, num_envs, **knobs)
    install_controller(env)
    env.reset(seed=SEED)
    out = env.rollout_controller(n_steps, store=("rew", "term", "trunc"))
    return env, check_against_planes(env, out["rew"], out["term"], out["trunc"], f"{kind} closed loop {knobs or ''}", t0)


# ------------------------------------------------------------------ a. stored planes, small ----
OPEN = ["rocksample", "heavenhell", "anttag_vector", "anttag_index", "taxi_philox", "taxi_numpy", "crooms_philox",
        "crooms_numpy", "carflag", "pomdp_m5", "pomdp_m37", "grid_philox"]
CLOSED = ["rocksample", "heavenhell", "anttag_index", "taxi_philox", "crooms_philox", "pomdp_m5", "pomdp_m37",
          "grid_philox"]


@pytest.mark.parametrize("kind", OPEN)
def test_open_loop_rollout(kind, gpu_device):
    env, want = open_loop(kind)
    assert want["env_steps"] == K * B


@pytest.mark.parametrize("kind,knobs", [("taxi_numpy", dict(taxi_npg_min=1 << 30)),
                                        ("crooms_numpy", dict(xg_min_envs=4096))], ids=["taxi", "crooms"])
def test_open_loop_numpy_one_workgroup(kind, knobs, gpu_device):
    """The numpy walkers' one-workgroup kernels (B = 1,027 is past their default crossover of 1,024 envs)."""
    open_loop(kind, **knobs)


@pytest.mark.parametrize("kind", CLOSED)
def test_closed_loop_rollout(kind, gpu_device):
    env, want = closed_loop(kind)
    assert want["env_steps"] == K * B
    # deterministic for a given B and launch sequence: a second handle reports the same bits
    twin, _ = closed_loop(kind)
    assert twin.metrics() == env.metrics()


def _belief_env(name, num_envs=B, rewards=None, n_vectors=6, **knobs):
    from test_belief_policy_gpu import vectors
    env = make(f"pomdp_{name}", num_envs, rewards, **knobs)
    env.reset(seed=SEED)
    with knobs_ctx(knobs):
        env.enable_belief()
    alpha, va = vectors(env.n_states, env.n_actions, n_vectors, seed=env.n_states + n_vectors)
    env.set_belief_policy(alpha, va)
    return env


def test_belief_rollout(gpu_device):
    t0 = time.perf_counter()
    env = _belief_env("m5")
    out = env.rollout_belief(K, store=("rew", "term", "trunc"))
    check_against_planes(env, out["rew"], out["term"], out["trunc"], "pomdp_m5 belief rollout", t0)


def test_population_metrics_beside_the_scores(gpu_device):
    """The population kernel adds every reward twice: into gp_metrics and into its group's score. Both keep the bound,
    and the groups' return_sum adds up to the batch's within it."""
    from population_oracle import population_scores
    t0 = time.perf_counter()
    G = 1024
    env = make("grid_philox")
    n_obs, A = controller_shape(env)
    probs = np.stack([random_probs(2, n_obs, A, seed=50 + p) for p in range(2)])
    env.set_controller_population(thresholds=population_thresholds(probs), group_envs=G, gamma=0.95)
    env.reset(seed=SEED)
    out = env.rollout_controller(K, store=("rew", "term", "trunc"))
    want = check_against_planes(env, out["rew"], out["term"], out["trunc"], "grid population", t0)
    got = env.metrics()
    scores = env.controller_scores()
    ws = population_scores(host(out["rew"]), host(out["term"]), host(out["trunc"]), np.zeros(B, np.int64), G, 0.95)
    for f in ("episodes", "length_sum", "env_steps"):
        assert np.array_equal(scores[f], ws[f]) and int(scores[f].sum()) == got[f]
    assert np.all(np.abs(scores["return_sum"] - ws["return_sum"]) <= ws["return_bound"])
    assert abs(got["return_sum"] - float(scores["return_sum"].sum())) <= want["bound"]


LOOPING = ["rocksample", "heavenhell", "anttag_index", "taxi_philox", "crooms_philox", "pomdp_m5", "carflag"]


@pytest.mark.parametrize("kind", LOOPING)
def test_blocks_looping_over_two_tiles(kind, gpu_device):
    """persist_bpc = 1: one block per CU; with B = 2 * tile * CUs + 5 every block takes two tiles and block 0 a third,
    ragged one, so a thread's sum runs on across tiles. Closed loop where the kind has it; 13 steps under a time limit of
    5."""
    import torch
    cus = torch.cuda.get_device_properties(gpu_device).multi_processor_count
    tile = 512 if kind.startswith("crooms") else 1024
    nb = 2 * tile * cus + 5
    run = open_loop if kind == "carflag" else closed_loop
    env, want = run(kind, mr.K_LOOP, nb, time_limit=5, persist_bpc=1)
    assert env.query("persist_blocks") == cus and -(-nb // tile) == 2 * cus + 1
    assert want["env_steps"] == mr.K_LOOP * nb


# ------------------------------------------------------------------ b. the numpy-exact grid kernels ----
@pytest.mark.parametrize("name,knobs,wgrid", [("windowed_4096", dict(wg_block_envs=4096), 1), ("windowed_512", {}, 1),
                                              ("fused", dict(wg_kmax=0), 0)])
def test_grid_numpy_count_based_epilogues(name, knobs, wgrid, gpu_device):
    """The windowed and the fused kernel count goal, wall and plain steps and multiply once per launch: in float64,
    reduced in float64. Launches of 1, 7 and 12 steps; the reference is the device's own rew plane."""
    import torch
    t0 = time.perf_counter()
    nb = mr.B_GRID
    env = make("grid_numpy", nb, time_limit=9, **knobs)
    if wgrid:
        assert env.query("wgrid") == 1 and env.query("wgrid_block_envs") == knobs.get("wg_block_envs", 512)
    else:
        assert env.query("wgrid_kmax") == 0 and env.query("fused_blocks") > 0
    env.reset(seed=SEED)
    rng = np.random.default_rng(SEED)
    planes = []
    for n_steps in mr.GRID_CHUNKS:
        acts = torch.as_tensor(rng.integers(0, 4, (n_steps, nb)).astype(np.int32), device=gpu_device)
        planes.append([x.clone() for x in env.rollout(acts)[1:]])
    rew, term, trunc = (torch.cat([p[i] for p in planes]) for i in range(3))
    want = check_against_planes(env, rew, term, trunc, f"grid numpy {name}", t0)
    assert want["env_steps"] == sum(mr.GRID_CHUNKS) * nb
    paid = set(np.unique(host(rew)))
    assert {F32(mr.STEP), F32(mr.WALL)} <= paid <= {F32(mr.STEP), F32(mr.WALL), F32(mr.GOAL)}


# ------------------------------------------------------------------ c. long launches, nothing stored ----
def _long_env(kind, rewards=None):
    if kind == "belief":
        return _belief_env("m5", rewards=rewards)
    env = make(kind, rewards=rewards)
    install_controller(env)
    env.reset(seed=SEED)
    return env


def _roll(env, kind, n_steps, store):
    return env.rollout_belief(n_steps, store=store) if kind == "belief" else env.rollout_controller(n_steps, store=store)


@pytest.mark.parametrize("kind", ["rocksample", "heavenhell", "pomdp_m5", "belief"])
def test_long_launch_of_a_constant_reward(kind, gpu_device):
    """K = 65,536 closed-loop steps in one launch with store=(): the path metrics() alone reads. Every reward is
    float32(0.1), so the exact return is B K float64(float32(0.1)) whatever the trajectory. The integers: a twin of the
    same seed runs the K steps as 64 launches of 1,024, storing only its flags, counted on the device in int64."""
    n_steps, v = mr.K_LONG, mr.CONSTANT_REWARD
    t0 = time.perf_counter()
    env = _long_env(kind, rewards=v)
    assert _roll(env, kind, n_steps, ()) == {}
    got = env.metrics()
    t1 = time.perf_counter()
    twin = _long_env(kind, rewards=v)
    count = mr.EpisodeCounter(B, gpu_device)
    part = n_steps // mr.LONG_PARTS
    for _ in range(mr.LONG_PARTS):
        out = _roll(twin, kind, part, ("term", "trunc"))
        count.add(out["term"], out["trunc"])
    want = count.result()
    exact = B * n_steps * float(v)
    want.update(return_sum=exact, bound=B * n_steps * 2.0 ** -52 * abs(exact))
    print(f"{kind}: the {n_steps}-step launch and metrics() {t1 - t0:.3f} s, the twin {time.perf_counter() - t1:.3f} s")
    mr.assert_metrics(got, want, f"{kind} K={n_steps} store=()")
    assert want["episodes"] >= B * (n_steps // TL)  # the time limit alone ends that many
    # the twin's own metrics: 64 launches, the same integers, the same bound
    mr.assert_metrics(twin.metrics(), want, f"{kind} {mr.LONG_PARTS} launches of {part}")
    env.check()
    twin.check()


def test_long_launch_of_varying_rewards(gpu_device):
    """K = 16,384 on the tabular model with its varying rewards, only rew / term / trunc stored (67 MB + 2 x 17 MB):
    the reference is the plane summed in float64 on the device, whose own error (a tree sum: about 24 roundings deep)
    is far inside the bound."""
    t0 = time.perf_counter()
    env = _long_env("pomdp_m37")
    out = env.rollout_controller(mr.K_LONG_VARYING, store=("rew", "term", "trunc"))
    want = check_against_planes(env, out["rew"], out["term"], out["trunc"], "pomdp_m37 K=16384", t0)
    assert want["env_steps"] == mr.K_LONG_VARYING * B


# ------------------------------------------------------------------ d. many short launches ----
@pytest.mark.parametrize("kind", ["heavenhell", "pomdp_m5", "taxi_numpy", "grid_numpy"])
def test_many_single_steps(kind, gpu_device):
    """300 step() calls, each a launch that adds a block's float64 total into its slot (plain +=, or atomically in the
    grid-wide and numpy-exact kernels)."""
    import torch
    t0 = time.perf_counter()
    nb = mr.B_GRID if kind == "grid_numpy" else B
    env = make(kind, nb)
    env.reset(seed=SEED)
    acts = torch.as_tensor(random_actions(env, mr.N_SINGLE_STEPS, SEED), device=gpu_device)
    steps = [env.step(acts[k])[1:4] for k in range(mr.N_SINGLE_STEPS)]
    rew, term, trunc = (torch.stack([s[i] for s in steps]) for i in range(3))
    check_against_planes(env, rew, term, trunc, f"{kind} 300 single steps", t0)
