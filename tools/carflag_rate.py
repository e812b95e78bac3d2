"""Throughput of Car-Flag (csrc/carflag.hip): steady K = 128 fused launches at 2M envs in philox mode (beside
Ant-Tag's philox rollout on the same build, the kernel of the same streaming shape), and the seed-identical numpy
mode at 64K and 2M envs over 192 steps (time_limit 160: the lockstep truncation burst at step 160, when every env
that never reached an end resets at once, lies inside the timed window).

Usage (GPU box): python tools/carflag_rate.py [out.json] -> one JSON line per measurement (also written to out.json).
Philox rows carry `frac_hbm`: algorithmic bytes per env-step (actions in, obs + reward + 2 flags out) over the
kernel time (hipEvent pairs around each launch), as a fraction of 8 TB/s.
"""
import json
import os
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")  # as bench.py
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gym-po-taxi_amd"))
import torch  # noqa: E402

from gym_po_amd import AntTagGridEnv, CarVecEnv  # noqa: E402

HBM = 8e12


def philox_rollout(name, env, acts, bytes_per_env_step, reps=5):
    K, B = acts.shape[0], acts.shape[1]
    env.reset(seed=0)
    run, _ = env.rollout_plan(acts)
    for _ in range(2):
        run()
    torch.cuda.synchronize()
    env.set_profiling(True)
    env.profile_read()
    t0 = time.perf_counter()
    for _ in range(reps):
        run()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    ms, n = env.profile_read()
    env.set_profiling(False)
    us_kernel = ms * 1e3 / (n * K)
    return {"what": name, "mode": "philox", "num_envs": B, "K": K, "launches": n, "us_per_step_kernel": us_kernel,
            "us_per_step_wall": wall / (reps * K) * 1e6, "bytes_per_env_step": bytes_per_env_step,
            "frac_hbm": bytes_per_env_step * B / (us_kernel * 1e-6) / HBM, "persist_blocks": env.query("persist_blocks"),
            "episodes": env.metrics()["episodes"]}


def numpy_steps(B, T=192):
    env = CarVecEnv(B, rng_mode="numpy")
    env.reset(seed=0)
    g = torch.Generator(device=env.device).manual_seed(1)
    # a held push of -1 / 0 / +1 per env plus noise: pushed envs end at a flag every ~55 steps, the third without
    # a push wander and truncate together at step 160
    acts = (torch.randint(0, 3, (1, B), device=env.device, generator=g) - 1
            + torch.rand((T, B), device=env.device, generator=g) * 2 - 1).float() * 0.45
    out = env._alloc_outputs()
    env.step_raw(acts[0], *out)
    env.reset(seed=0)
    torch.cuda.synchronize()
    env.set_profiling(True)
    env.profile_read(), env.profile_read_resolver()
    t0 = time.perf_counter()
    for t in range(T):
        env.step_raw(acts[t], *out)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    (ms1, n1), (ms2, n2) = env.profile_read(), env.profile_read_resolver()
    m = env.metrics()
    return {"what": "carflag", "mode": "numpy", "num_envs": B, "steps": T, "us_per_step_wall": wall / T * 1e6,
            "us_per_step_step_kernel": ms1 * 1e3 / n1, "us_per_step_resolver": ms2 * 1e3 / n2,
            "env_steps_per_s": B * T / wall, "episodes": m["episodes"]}


def main():
    rows = []
    B, K = 1 << 21, 128
    dev = torch.device("cuda", torch.cuda.current_device())
    g = torch.Generator(device=dev).manual_seed(0)
    acts = (torch.rand((K, B), device=dev, generator=g) * 3 - 1.5).float()
    rows.append(philox_rollout("carflag_f32", CarVecEnv(B, rng_mode="philox"), acts, 4 + 12 + 4 + 2))
    del acts
    acts = torch.randint(0, 5, (K, B), device=dev, generator=g, dtype=torch.int32)
    rows.append(philox_rollout("anttag", AntTagGridEnv(B), acts, 4 + 16 + 4 + 2))
    del acts
    for b in (1 << 16, 1 << 21):
        rows.append(numpy_steps(b))
    for r in rows:
        print(json.dumps(r), flush=True)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
