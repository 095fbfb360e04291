"""Batched tabular Q-learning / SARSA, the parts that need no GPU: the stream-4 words, the CPU restatement learning the optimal
policy, the greedy-policy conversion and the library's new symbols."""
import subprocess

import numpy as np
import pytest

from griduniverse_amd import _lib, rng
from griduniverse_amd.algorithms.temporal_difference import greedy_policy
from griduniverse_amd.envs.griduniverse_env import GridUniverseEnv
from oracle import c_oracle as C
from oracle import gu_rng as R

from . import _td_oracle as O
from ._walks import _bfs_lengths, _greedy_walk_lengths


def test_epsilon_greedy_words_equal_the_oracle_across_the_epoch_boundary():
    envs = np.array([0, 1, 7, 4095, 2 ** 31 + 5], np.uint64)
    for t0 in (0, 2 ** 28 - 2, 2 ** 32 - 3):
        got = rng.epsilon_greedy_words(11, envs, t0, 6)
        for i in range(6):
            t = t0 + i
            want = [R.word(11, int(e), 4, t & 0xFFFFFFFF, epoch=t >> 32) for e in envs]
            assert got[i].tolist() == want
            assert np.array_equal(got[i], O.words(11, envs, np.full(len(envs), t, np.uint64)))
    # per-env start counts, and a different stream than the uniform actions'
    t0 = np.array([5, 2 ** 32 - 1], np.uint64)
    got = rng.epsilon_greedy_words(3, [2, 9], t0, 2)
    assert got[1, 1] == R.word(3, 9, 4, 0, epoch=1) and got[0, 0] == R.word(3, 2, 4, 5)
    assert got[0, 0] != R.word(3, 2, 0, 5)


@pytest.mark.parametrize('W,H,T', [(4, 4, 3000), (8, 8, 12000)])
def test_oracle_q_learning_learns_the_shortest_paths(W, H, T):
    grid = C.Grid.from_lists(W, H)
    L = 64
    o = O.TdOracle(grid, 5, L)
    o.reset()
    o.run(T, O.Q_LEARNING, 0.1, 0.9, int(round(0.2 * 65536)))
    dist = _bfs_lengths(grid)
    for e in range(L):  # every learner's greedy policy walks every start cell to the goal on a shortest path
        walk = _greedy_walk_lengths(grid, o.q[e])
        assert np.array_equal(walk[grid.starts], dist[grid.starts]), (e, walk.reshape(H, W), dist.reshape(H, W))


def test_oracle_sarsa_learns_a_path_to_the_goal():
    grid = C.Grid.from_lists(4, 4)
    o = O.TdOracle(grid, 2, 16)
    o.reset()
    o.run(3000, O.SARSA, 0.1, 0.9, int(round(0.1 * 65536)))
    for e in range(16):
        assert _greedy_walk_lengths(grid, o.q[e])[0] == _bfs_lengths(grid)[0]


def test_greedy_policy_follows_the_references_tie_and_terminal_rules():
    env = GridUniverseEnv((4, 4), lava_states=[5])
    grid = C.Grid.from_env(env)
    S = grid.S
    s = np.repeat(np.arange(S, dtype=np.int32), 4)
    a = np.tile(np.arange(4, dtype=np.int32), S)
    nxt, rew, _ = C.look_step_ahead(grid, s, a, True)
    for gamma, v in ((1.0, np.zeros(S)), (0.9, np.arange(S, dtype=np.float64) / 3.0), (0.99, np.random.RandomState(0).randn(S))):
        q = (0.0 + (rew + gamma * v[nxt])).reshape(S, 4)  # utils.py:66
        got = greedy_policy(q, env)
        want = C.greedy_policy(grid, gamma, v)
        assert got.tobytes() == want.tobytes(), gamma
    # by hand: ties after rounding to 8 decimals share, terminal rows (goal 15, lava 5) are zero
    q = np.zeros((S, 4))
    q[0] = [1.0, 1.0 + 1e-10, 0.0, 1.0]
    q[1] = [0.0, 2.0, 0.0, 0.0]
    q[5] = [9.0, 0.0, 0.0, 0.0]
    q[15] = [0.0, 3.0, 0.0, 0.0]
    pi = greedy_policy(q, env)
    assert pi[0].tolist() == [1 / 3, 1 / 3, 0.0, 1 / 3]
    assert pi[1].tolist() == [0.0, 1.0, 0.0, 0.0]
    assert pi[2].tolist() == [0.25] * 4
    assert not pi[5].any() and not pi[15].any()
    with pytest.raises(ValueError):
        greedy_policy(np.zeros((S, 3)), env)


def test_library_exports_the_td_entry_points():
    syms = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], stdout=subprocess.PIPE, check=True).stdout.decode()
    for name in ('gu_td_init', 'gu_td_run', 'gu_td_get_q', 'gu_td_set_q'):
        assert ' T ' + name + '\n' in syms, name
        assert name in _lib.SIGNATURES
