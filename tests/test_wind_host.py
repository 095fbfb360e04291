"""Wind, the parts that need no GPU: the wind plane, the rule on Sutton & Barto's grid, the CPU restatement against the calm C oracle,
the gust draws and the argument checks."""
import subprocess

import numpy as np
import pytest

import griduniverse_amd as gua
from griduniverse_amd import _lib, rng
from griduniverse_amd.grid import wind_plane
from oracle import c_oracle as C

from . import _wind_oracle as O
from ._tabular_cases import GRIDS, _grid, _spec


def test_wind_plane_shapes_and_errors():
    W, H = 10, 7
    per_column = wind_plane(W, H, O.BOOK_STRENGTH)
    assert per_column.dtype == np.uint8 and per_column.shape == (70,)
    assert np.array_equal(per_column.reshape(H, W), np.tile(O.BOOK_STRENGTH << 2, (H, 1)))  # direction 'up' is code 0
    full = np.arange(70).reshape(H, W) % 4
    assert np.array_equal(wind_plane(W, H, full, 'left'), ((full << 2) | 3).reshape(70))
    assert np.array_equal(wind_plane(W, H, full, 2), ((full << 2) | 2).reshape(70))
    dirs = (np.arange(70).reshape(H, W) // 3) % 4
    assert np.array_equal(wind_plane(W, H, full, dirs), ((full << 2) | dirs).reshape(70))
    assert np.array_equal(wind_plane(W, H, full, np.arange(W) % 4), ((full << 2) | (np.arange(W) % 4)[None, :]).reshape(70))
    for name, code in (('up', 0), ('right', 1), ('down', 2), ('left', 3)):
        assert np.array_equal(wind_plane(3, 2, np.ones(3, int), name), np.full(6, 4 | code, np.uint8))
    for bad in (dict(strength=np.full(W, 4)), dict(strength=np.full(W, -1)), dict(strength=np.zeros(W + 1, int)), dict(strength=np.zeros((W, H), int)),
                dict(strength=np.zeros(W)), dict(strength=1), dict(strength=np.zeros(W, int), direction='north'),
                dict(strength=np.zeros(W, int), direction=4), dict(strength=np.zeros(W, int), direction=np.zeros(H, int)),
                dict(strength=np.zeros(W, int), direction=np.full(W, -1))):
        with pytest.raises(ValueError):
            wind_plane(W, H, **bad)


def test_the_books_grid_shortest_path_is_10_and_62_cells_are_reachable():
    """An agent cannot be blown across a terminal cell, so the goal is nearer than under the book's vector-sum rule (15)."""
    grid = _grid(O.BOOK)
    dist = O.bfs(grid, wind_plane(O.BOOK_W, O.BOOK_H, O.BOOK_STRENGTH), O.BOOK['starts'][0])
    assert dist[O.BOOK['goals'][0]] == 10
    assert len(dist) == 62
    calm = O.bfs(grid, np.zeros(70, np.uint8), O.BOOK['starts'][0])
    assert calm[O.BOOK['goals'][0]] == 7 and len(calm) == 70


def test_the_oracle_with_strength_zero_equals_the_calm_c_oracle():
    g = GRIDS['maze11']()
    grid, N, T, seed = _grid(g), 64, 200, 9
    for auto in (True, False):
        for gust in (0, O.GUST_THIRDS):
            o = O.WindOracle(grid, seed, N, wind=wind_plane(g['W'], g['H'], np.zeros(g['W'], int), 'right'), gust_q16=gust)
            st = C.State(N)
            assert np.array_equal(o.reset(), C.reset(grid, seed, st))
            got = o.rollout(T, 'uniform', auto_reset=auto)
            want = C.rollout(grid, seed, st, T, auto, stats=True)
            for k in ('obs', 'reward', 'done', 'ret', 'episodes'):
                assert np.asarray(got[k]).astype(np.int64).tobytes() == np.asarray(want[k]).astype(np.int64).tobytes(), (k, auto, gust)
            assert np.array_equal(o.state.pos, st.pos) and np.array_equal(o.state.done, st.done)
            assert np.array_equal(o.state.episode, st.episode) and np.array_equal(o.state.tcount, st.tcount)


def test_gust_counts_and_words():
    """Of the 65 536 draws of seed 7, envs 0 .. 63, t 0 .. 1023 at gust 2/3: 21 843 keep k, 21 963 add one, 21 730 take one --
    each within 5 sigma = 604 of a third (sigma = sqrt(65536 * 1/3 * 2/3) = 120.7)."""
    envs = np.arange(64, dtype=np.uint64)[None, :]
    t = np.arange(1024, dtype=np.uint64)[:, None]
    w = O.gust_words(7, envs, t)
    assert np.array_equal(w, rng.wind_words(7, envs, t))
    k = O.gusted(np.full(w.shape, 2), w, O.GUST_THIRDS)
    counts = [int((k == v).sum()) for v in (2, 3, 1)]
    assert counts == [21843, 21963, 21730]
    for c in counts:
        assert abs(c - 65536 / 3) <= 604
    assert np.array_equal(O.gusted(np.zeros(w.shape, int), w, 65536), np.zeros(w.shape, int))  # calm cells never gust
    assert np.array_equal(O.gusted(np.full(w.shape, 3), w, 0), np.full(w.shape, 3))
    up = O.gusted(np.full(w.shape, 3), w, 65536)
    assert set(np.unique(up).tolist()) == {2, 4}
    # the epoch is hashed behind the seed, as for stream 4, and the stream is its own
    t_hi = np.array([2 ** 32 + 5], np.uint64)
    assert rng.wind_words(7, [3], t_hi)[0] == rng.words(7, [3], 9, 5, 1)[0] != rng.words(7, [3], 9, 5)[0]
    assert rng.wind_words(7, [3], [5])[0] != rng.epsilon_greedy_words(7, [3], 5, 1)[0, 0]


class _NoEngine(object):
    """Stands in for Engine: any call on it is a library call that must not have been made."""

    def __init__(self, *a, **kw):
        self.calls = []

    def __getattr__(self, name):
        def call(*a, **kw):
            self.calls.append(name)
        return call


def test_bad_arguments_are_value_errors_raised_before_any_library_call():
    vec = gua.VecGridUniverse(4, template=_spec(O.BOOK), engine_factory=_NoEngine)
    for kw in (dict(gust=1.5), dict(gust=-0.1), dict(gust=float('nan'))):
        with pytest.raises(ValueError):
            vec.set_wind(O.BOOK_STRENGTH, **kw)
    with pytest.raises(ValueError):
        vec.set_wind(None, gust=1.5)
    with pytest.raises(ValueError):
        vec.set_wind(np.full(10, 4))
    with pytest.raises(ValueError):
        vec.set_wind(O.BOOK_STRENGTH, 'sideways')
    assert vec.engine.calls == []
    vec.set_wind(O.BOOK_STRENGTH, gust=2 / 3)
    vec.set_wind(None)
    assert vec.engine.calls == ['set_wind', 'set_wind']
    from griduniverse_amd.algorithms.temporal_difference import q_learning, sarsa
    for learn in (q_learning, sarsa):
        with pytest.raises(ValueError):
            learn(None, 10, wind=O.BOOK_STRENGTH, gust=1.5)


def test_library_exports_the_wind_entry_points_and_kernels():
    syms = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], stdout=subprocess.PIPE, check=True).stdout.decode()
    for name in ('gu_set_wind', 'gu_get_wind'):
        assert ' T ' + name + '\n' in syms, name
        assert name in _lib.SIGNATURES
    blob = open(_lib.LIB_PATH, 'rb').read()
    assert b'gu_wind_step_kernel' in blob and b'gu_wind_rollout_kernel' in blob
