"""Grids and helpers shared by the device tests of the tabular learners (test_gpu_td.py, test_gpu_dyna.py)."""
import numpy as np

import griduniverse_amd as gua
from griduniverse_amd.grid import GridSpec
from oracle import c_oracle as C

from . import _golden as G


def _level(name):
    sp = G.load_json('levels.json')[name]
    return dict(W=sp['W'], H=sp['H'], starts=sp['starts'], goals=sp['goals'], lava=sp['lava'], walls=sp['walls'])


def _traj_grid(name):
    meta, _ = G.load_traj(name)
    return dict(W=meta['W'], H=meta['H'], starts=meta['starts'], goals=meta['goals'], lava=meta['lava'], walls=meta['walls'],
                reward=meta['reward'])


GRIDS = {
    'default4x4': lambda: dict(W=4, H=4, starts=[0], goals=[15], lava=[], walls=[]),
    'test_env': lambda: _level('test_env.txt'),
    'open8x8': lambda: _traj_grid('c2_open8x8'),
    'maze11': lambda: _level('maze_11x11.txt'),
    'lava32': lambda: _traj_grid('c4_lava32'),
}


def spread_grid(W, H):
    """A grid for test_gpu_learners_at_scale.py (never one of GRIDS: those run at N = 4096): three starts, at the top, in the middle
    and at the bottom of the index range, a goal two cells to the side of each, a lava cell in the row above the top start and in the
    row below the middle one (above it where that is the last row; a single row: two cells to the other side of it) and two walls."""
    S = W * H
    mid = S // 2 + 7
    lava = [S - 1 - W, mid + W if mid + W < S else mid - W] if H > 1 else [mid - 2]
    return dict(W=W, H=H, starts=[S - 1, mid, 0], goals=[S - 3, mid + 2, 2], lava=lava, walls=[5, S - 7])


def _spec(g):
    return GridSpec(g['W'], g['H'], g['starts'], g['goals'], g['lava'], g['walls'], g.get('reward'))


def _grid(g):
    return C.Grid.from_lists(g['W'], g['H'], walls=g['walls'], goals=g['goals'], lava=g['lava'], starts=g['starts'], reward=g.get('reward'))


def _eps(epsilon):
    return int(round(epsilon * 65536))


def _same(got, want, keys=('obs', 'reward', 'done', 'ret', 'episodes')):
    for k in keys:
        assert np.asarray(got[k]).astype(np.int64).tobytes() == np.asarray(want[k]).astype(np.int64).tobytes(), k


def _pair(oracle_cls, g, N, seed, q0=0.0):
    """A batch of N learners on grid g with tables of q0 and the oracle_cls restatement of it, both reset."""
    vec = gua.VecGridUniverse(N, template=_spec(g), seed=seed)
    vec._ensure_q(q0)
    o = oracle_cls(_grid(g), seed, N, q0=q0)
    assert np.array_equal(vec.reset(), o.reset())
    return vec, o


def _random_grids(n, W, H, seed):
    out = []
    for k in range(n):
        wall, start, goal = C.generate_maze(seed, k, W, H)
        out.append(dict(W=W, H=H, starts=[start], goals=[goal], lava=[], walls=np.flatnonzero(wall).tolist()))
    return out
