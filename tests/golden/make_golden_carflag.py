"""Record the Car-Flag golden fixtures from the reference (gym_po.envs.car_flag, loaded by refload.load()).

    python tests/golden/make_golden_carflag.py

Writes tests/golden/carflag_*.npz and tests/golden/carflag_index.json: DATA only (seeds, the action recipe, the
reference's per-step outputs, its final state and final PCG64 state, and the draws its resets took). The draws
are recorded by running a second numpy Generator from the same seed through the same calls and checking that it
reproduces the reference's reset values. A fixture that lacks one of the event classes it is meant to pin is
refused.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import refload  # noqa: E402
from carflag_oracle import make_actions, reset_position  # noqa: E402
from fixtures import digest  # noqa: E402

CASES = {
    "carflag_f32_b64": dict(env="CarVecEnv", num_envs=64, steps=400, time_limit=160, seed=11, action_seed=1,
                            recipe="bias", period=50, action_dtype="float32"),
    "carflag_f32_tl40_b63": dict(env="CarVecEnv", num_envs=63, steps=200, time_limit=40, seed=12, action_seed=2,
                                 recipe="bias", period=50, action_dtype="float32"),
    "carflag_f64_b64": dict(env="CarVecEnv", num_envs=64, steps=400, time_limit=160, seed=11, action_seed=1,
                            recipe="bias", period=50, action_dtype="float64"),
    "carflag_disc5_b64": dict(env="DiscreteActionCarVecEnv", num_envs=64, steps=300, time_limit=160, seed=13,
                              action_seed=3, recipe="held", period=40, action_dtype="int64", num_actions=5),
}


def rng_meta(gen):
    st = gen.bit_generator.state
    return {"state": str(st["state"]["state"]), "inc": str(st["state"]["inc"]), "has_uint32": int(st["has_uint32"]),
            "uinteger": int(st["uinteger"])}


def record(name, meta, car_flag):
    B, T = meta["num_envs"], meta["steps"]
    if meta["env"] == "CarVecEnv":
        env = car_flag.CarVecEnv(B, time_limit=meta["time_limit"])
    else:
        env = car_flag.DiscreteActionCarVecEnv(meta["num_actions"], B, time_limit=meta["time_limit"])
    shadow = np.random.default_rng(meta["seed"])  # the same stream, drawn through the same calls
    acts = make_actions(meta)
    k53 = np.zeros((T + 1, B), np.uint64)
    hidx = np.zeros((T + 1, B), np.int8)
    pidx = np.zeros((T + 1, B), np.int8)

    def shadow_draw(row, mask):
        b = int(mask.sum())
        if b == 0:
            return
        k = (shadow.random(b) * float(1 << 53)).astype(np.uint64)
        h, p = shadow.choice(2, b), shadow.choice(2, b)
        assert np.array_equal(reset_position(k), env.s[mask, 0]), "shadow stream: reset position"
        assert np.array_equal(np.where(h > 0, 1, -1), env.heavens[mask]), "shadow stream: heavens"
        assert np.array_equal(np.where(p > 0, 0.5, -0.5), env.priests[mask]), "shadow stream: priests"
        k53[row, mask], hidx[row, mask], pidx[row, mask] = k, h, p

    obs0, _ = env.reset(seed=meta["seed"])
    obs0 = obs0.copy()
    shadow_draw(0, np.ones(B, bool))
    obs = np.zeros((T, B, 3), np.float32)
    rew = np.zeros((T, B), np.float32)
    term = np.zeros((T, B), bool)
    trunc = np.zeros((T, B), bool)
    for t in range(T):
        o, r, d, tr, _ = env.step(acts[t].reshape(B, 1) if meta["env"] == "CarVecEnv" else acts[t])
        obs[t], rew[t], term[t], trunc[t] = o, r, d, tr
        shadow_draw(t + 1, d | tr)
    assert env.np_random.bit_generator.state == shadow.bit_generator.state
    assert obs.dtype == np.float32 and env.s.dtype == np.float32
    # every event class this fixture is meant to pin
    events = {"term_plus": int(((rew > 0) & term).sum()), "term_minus": int(((rew < 0) & term).sum()),
              "trunc_only": int((trunc & ~term).sum()), "dir_plus": int((obs[:, :, 2] > 0).sum()),
              "dir_minus": int((obs[:, :, 2] < 0).sum())}
    if meta["recipe"] == "bias":
        events["clipped_actions"] = int((np.abs(acts) > 1).sum())
    for k, v in events.items():
        if v == 0:
            raise SystemExit(f"{name}: no {k} event in the recording; not written")
    np.savez_compressed(os.path.join(HERE, name + ".npz"), obs0=obs0, obs=obs, rew=rew, term=term, trunc=trunc,
                        final_s=env.s, final_heavens=env.heavens, final_priests=env.priests,
                        final_elapsed=env.elapsed.astype(np.int64), k53=k53, hidx=hidx, pidx=pidx)
    out = dict(meta)
    out.update(file=name + ".npz", events=events, final_rng=rng_meta(env.np_random),
               digest={"obs": str(digest(obs)), "rew": str(digest(rew)), "term": str(digest(term)),
                       "trunc": str(digest(trunc)), "actions": str(digest(acts))})
    return out


def record_render(car_flag):
    """8 frames of env 0 with the state they were drawn from."""
    env = car_flag.CarVecEnv(2, time_limit=160, render_mode="rgb_array")
    env.reset(seed=21)
    rng = np.random.default_rng(5)
    frames, s0, hv, pr = [], [], [], []
    taken = {}  # (direction shown, heaven side) -> frames so far: two of each of the four combinations
    t = 0
    while len(frames) < 8:
        if t % 60 == 0:
            bias = rng.choice([-1.0, 1.0], 2)
        env.step(np.clip(bias + rng.uniform(-1, 1, 2), -1, 1).astype(np.float32))
        t += 1
        key = (bool(env.s[0, 2] != 0), bool(env.heavens[0] > 0))
        if taken.get(key, 0) < 2 and t % 7 == 0:
            taken[key] = taken.get(key, 0) + 1
            frames.append(env.render().copy())
            s0.append(env.s[0].copy())
            hv.append(env.heavens[0])
            pr.append(env.priests[0])
        if t > 20000:
            raise SystemExit(f"carflag_render: only {taken} after {t} steps; not written")
    hv = np.array(hv, np.float32)
    np.savez_compressed(os.path.join(HERE, "carflag_render.npz"), frames=np.stack(frames), s0=np.stack(s0),
                        heavens=hv, priests=np.array(pr, np.float64))
    return dict(file="carflag_render.npz", frames=8, seed=21)


def main():
    refload.load()
    import gym_po.envs.car_flag as car_flag
    cases = {name: record(name, meta, car_flag) for name, meta in CASES.items()}
    index = {"numpy_version": np.__version__, "cases": cases, "carflag_render": record_render(car_flag)}
    with open(os.path.join(HERE, "carflag_index.json"), "w") as f:
        json.dump(index, f, indent=1, sort_keys=True)
        f.write("\n")
    for name, c in cases.items():
        print(name, c["events"])


if __name__ == "__main__":
    main()
