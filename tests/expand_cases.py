"""TEST INFRASTRUCTURE — the inputs shared by tests/test_expand_cpu.py, tests/test_expand_gpu.py and
tests/test_expand_paths_gpu.py: the models of tests/pbvi_cases.py plus a hand-made one with dead
candidates, the special points and reference sets of the parity tests, and the oracle's expansion of each, made once
and left unchanged.
"""
import numpy as np

import belief_oracle as bo
import expand_oracle as xo
import pbvi_cases as pc

F = np.float32
cached = pc.cached
bits = pc.bits
OUTPUTS = ("succ", "dist", "actions", "obs", "mass")


def hand_tables():
    """Three states, state 2 terminal and absorbing; two actions; three obs of which obs 2 never occurs. From state 1
    every action ends the episode: a point on states 1 and 2 alone has no live candidate. Action 1 from state 0 stays
    in 0 and is seen as obs 0 or 1 with equal probability: two candidates with the same successor (a tie over o)."""
    T = np.zeros((3, 2, 3))
    T[0, 0] = [0.5, 0.25, 0.25]
    T[0, 1] = [1.0, 0.0, 0.0]
    T[1, :, 2] = 1.0
    T[2, :, 2] = 1.0
    Z = np.zeros((2, 3, 3))
    Z[0, 0] = [0.75, 0.25, 0.0]
    Z[0, 1] = [0.25, 0.75, 0.0]
    Z[0, 2] = [1.0, 0.0, 0.0]
    Z[1, :, :2] = 0.5
    R = np.zeros((3, 2, 3), dtype=F)
    return T, Z, R, np.array([1.0, 0.0, 0.0]), np.array([False, False, True]), np.array([[1.0, 0, 0]] * 3)


def tables(name):
    return cached(("xtables", name), hand_tables) if name == "hand" else pc.tables(name)


def spec(name):
    if name != "hand":
        return pc.spec(name)

    def make():
        from gym_po_amd import row_thresholds
        from pomdp_oracle import Spec
        T, Z, R, start, terminal, reset_obs = tables(name)
        return Spec(row_thresholds(T), row_thresholds(Z), row_thresholds(start), row_thresholds(reset_obs), R, terminal,
                    7)
    return cached(("xspec", name), make)


def laws(name):
    return cached(("xlaws", name), lambda: bo.Laws(spec(name)))


def points(name, P):
    """Points [P, S] in the manner of pbvi_cases.special_inputs (row 0 and row 1 one-hot, sparse rows, every fifth row
    from row 2 unnormalised); on the hand model row 1 sits on the states that only end the episode (no live candidate),
    and on Tiger row 0 is the uniform belief, whose two successors under listen are mirror images (a tie over o when
    the reference set is symmetric)."""
    def make():
        S = laws(name).S
        rng = np.random.default_rng(31 * P + S)
        b = rng.random((P, S)) * (rng.random((P, S)) > 0.5)
        b[np.arange(P), rng.integers(0, S, P)] += 0.1
        b = b / b.sum(-1, keepdims=True)
        b[0] = 0.0
        b[0, 0] = 1.0  # one-hot
        if P > 1:
            b[1] = 0.0
            b[1, S - 1] = 1.0  # (on (5,2,3): obs 2 has probability zero from here under action 0)
        b[2::5] *= 3.0  # unnormalised
        if name == "hand" and P > 1:
            b[1] = [0.0, 0.25, 0.75]
        if name == "tiger":
            b[0] = 0.5
        return b.astype(F)
    return cached(("xpoints", name, P), make)


def ref_set(name, Q):
    """A reference set [Q, S]: random sparse rows, some unnormalised; row Q - 1 repeats row 0 and (Q >= 4) row 2 repeats
    row 1 (duplicates change no minimum). On Tiger rows 0 and 1 are the corners (1, 0) and (0, 1): symmetric about the
    uniform belief."""
    def make():
        S = laws(name).S
        rng = np.random.default_rng(77 * Q + S)
        q = rng.random((Q, S)) * (rng.random((Q, S)) > 0.4)
        q[np.arange(Q), rng.integers(0, S, Q)] += 0.1
        q = q / q.sum(-1, keepdims=True)
        q[3::7] *= 2.0
        if name == "tiger":
            q[:] = 0.5  # (every row is symmetric on Tiger: the tie of the uniform point survives any Q)
            q[0] = [1.0, 0.0]
            if Q > 1:
                q[1] = [0.0, 1.0]
        if Q >= 4:
            q[2] = q[1]
        q[Q - 1] = q[0]
        return q.astype(F)
    return cached(("xref", name, Q), make)


def reference(name, P, Q):
    """(points, ref or None, the oracle's expansion). Q = None: the points are their own reference set."""
    def make():
        b = points(name, P)
        q = None if Q is None else ref_set(name, Q)
        return b, q, xo.expand(laws(name), b, q)
    return cached(("xreference", name, P, Q), make)


# the oracle's cost P Q S A O stays below 2 10^8 per case; every P in {1, 3, 67, 257} and every Q in {1, 64, 65, 257,
# 1027} occurs on a model in LDS (tiger, m5, hand) and on one in global memory (m37, m300); None: ref = NULL
CASES = [("tiger", 1, 1), ("tiger", 3, None), ("tiger", 67, 65), ("tiger", 257, 1027), ("tiger", 257, None),
         ("hand", 3, 64), ("hand", 67, None), ("hand", 257, 257), ("hand", 1, 1027),
         ("m5", 1, 64), ("m5", 3, 1027), ("m5", 67, 257), ("m5", 257, 65), ("m5", 257, None), ("m5", 67, 1),
         ("m37", 1, 1027), ("m37", 3, 65), ("m37", 67, 64), ("m37", 257, 1), ("m37", 67, None), ("m37", 257, 257),
         ("m37", 257, 1027),
         ("m300", 1, 257), ("m300", 3, 1027), ("m300", 67, 65), ("m300", 257, 1), ("m300", 3, None), ("m300", 67, 64)]
