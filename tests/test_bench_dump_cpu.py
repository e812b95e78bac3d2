"""bench.py --dump-outputs (CPU; dump_outputs works on any torch tensors): the files hold row k_last - 1 of the
(obs, reward, terminated, truncated) buffers as float32 (float64 for 64-bit outputs), an array above DUMP_MAX_ELEMS
elements as the same seeded sample in every run, at most 64 MB in all; k_last for the ways the timed steps split into
launches; importing bench leaves the process's environment and sys.path alone; bench.py offers --full /
--dump-outputs."""
import os
import sys

import numpy as np
import pytest

NAMES = ("obs", "reward", "terminated", "truncated")


@pytest.fixture(scope="module")
def bench():
    """bench.py as a module, imported with no trace left in this process: the GPU tests that run after this file
    must see the HIP runtime settings and the sys.path they would see without it."""
    env, path = dict(os.environ), list(sys.path)
    import bench as b
    assert dict(os.environ) == env, "importing bench changed the environment"
    sys.path[:] = path
    return b


def _buffers(K, B, obs_tail=(), obs_dtype=None):
    import torch
    g = torch.Generator().manual_seed(5)
    obs = torch.randint(0, 200, (K, B) + obs_tail, generator=g).to(obs_dtype or torch.int32)
    rew = torch.rand((K, B), generator=g, dtype=torch.float32)
    term = torch.randint(0, 2, (K, B), generator=g).to(torch.uint8)
    trunc = torch.randint(0, 2, (K, B), generator=g).to(torch.uint8)
    return obs, rew, term, trunc


def test_dump_is_the_last_launch_row_exact(bench, tmp_path):
    out = _buffers(7, 33, (4,))
    bench.dump_outputs(str(tmp_path / "d"), out, 3)  # the last launch ran 3 steps: row 2
    assert sorted(os.listdir(tmp_path / "d")) == sorted(n + ".npy" for n in NAMES)
    for n, o in zip(NAMES, out):
        x = np.load(tmp_path / "d" / (n + ".npy"))
        assert x.dtype == np.float32
        np.testing.assert_array_equal(x, o[2].reshape(-1).numpy().astype(np.float32))


@pytest.mark.parametrize("dtype", ["float64", "int64"])
def test_dump_64_bit_outputs_are_float64(bench, tmp_path, dtype):
    import torch
    out = _buffers(2, 9, (2,), getattr(torch, dtype))
    out[0][1, 0, 0] = 2**40 + 1  # not a float32
    bench.dump_outputs(str(tmp_path), out, 2)
    x = np.load(tmp_path / "obs.npy")
    assert x.dtype == np.float64 and x[0] == 2**40 + 1
    np.testing.assert_array_equal(x, out[0][1].reshape(-1).numpy().astype(np.float64))
    assert np.load(tmp_path / "reward.npy").dtype == np.float32


def test_dump_large_array_is_a_fixed_sample(bench, tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_ELEMS", 100)
    out = _buffers(2, 101, (3,))  # obs row: 303 elements (sampled); the others: 101 (sampled too)
    bench.dump_outputs(str(tmp_path / "a"), out, 1)
    bench.dump_outputs(str(tmp_path / "b"), out, 1)
    idx = np.sort(np.random.default_rng(0).integers(0, 303, 100))
    a = np.load(tmp_path / "a" / "obs.npy")
    assert a.shape == (100,)
    np.testing.assert_array_equal(a, out[0][0].reshape(-1).numpy()[idx].astype(np.float32))
    for n in NAMES:
        np.testing.assert_array_equal(np.load(tmp_path / "a" / (n + ".npy")), np.load(tmp_path / "b" / (n + ".npy")))


def test_dump_of_the_largest_outputs_stays_below_64_mb(bench, tmp_path):
    """Every array above the cap and the widest dtypes the buffers can have (64-bit obs; reward float32 and the
    flags uint8 by the output layout): the files written are measured, not computed."""
    import torch
    n = bench.DUMP_MAX_ELEMS + 3
    out = (torch.zeros((1, n), dtype=torch.int64), torch.zeros((1, n), dtype=torch.float32),
           torch.zeros((1, n), dtype=torch.uint8), torch.zeros((1, n), dtype=torch.uint8))
    bench.dump_outputs(str(tmp_path), out, 1)
    assert sum(os.path.getsize(tmp_path / f) for f in os.listdir(tmp_path)) <= 64 * 10**6
    assert np.load(tmp_path / "obs.npy").shape == (bench.DUMP_MAX_ELEMS,)


@pytest.mark.parametrize("steps,C,k_last", [(20, 20, 20), (2000, 64, 16), (128, 64, 64), (5, 128, 5), (130, 128, 2),
                                            (1, 1, 1), (129, 128, 1)])
def test_last_launch_steps(bench, steps, C, k_last):
    assert bench.last_launch_steps(steps, C) == k_last
    # as the timed loop issues them: launches of min(C, what is left)
    done = k = 0
    while done < steps:
        k = min(C, steps - done)
        done += k
    assert k == k_last


def test_options_exist(bench, capsys, monkeypatch):
    env = dict(os.environ)
    monkeypatch.setattr("sys.argv", ["bench.py", "--help"])
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 0 and dict(os.environ) == env
    text = capsys.readouterr().out
    assert "--full" in text and "--dump-outputs DIR" in text and "--steps" in text and "--warmup" in text
