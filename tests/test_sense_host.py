"""The agent's sensors on the host: the class rule against the reference viewer's tiles (tests/golden/arrows.json), the numpy
mirror (griduniverse_amd.grid) against the one-cell-at-a-time restatement (tests/_sense_oracle.py), view_features, and the N = 1
facade.  No GPU."""
import numpy as np
import pytest

import griduniverse_amd as gua
from griduniverse_amd import grid as GR
from griduniverse_amd.algorithms import view_features
from griduniverse_amd.grid import GridSpec
from oracle import render as R

from . import _golden as G
from . import _sense_oracle as O
from ._tabular_cases import GRIDS, _spec, _traj_grid

HOST_GRIDS = dict(default4x4=GRIDS['default4x4'], test_env=GRIDS['test_env'], maze11=GRIDS['maze11'],
                  grid1x1=lambda: _traj_grid('grid1x1'), grid1x9=lambda: _traj_grid('grid1x9'), grid9x1=lambda: _traj_grid('grid9x1'))
RADII = (0, 1, 2, 7)
KIND = {'ground': 0, 'wall': 1, 'lava': 2, 'goal': 3}


def test_class_rule_is_the_reference_viewers_tile_rule():
    cases = G.load_json('arrows.json')['cases']
    assert len(cases) >= 4
    for case in cases:
        S = case['W'] * case['H']
        g = dict(W=case['W'], H=case['H'], goals=case['goals'], lava=case['lava'], walls=case['walls'])
        want = [KIND[k] for k in R.tile_kinds(S, case['goals'], case['lava'], case['walls'])]
        assert [KIND[k] for k in case['tiles']] == want, case['name']
        spec = GridSpec(case['W'], case['H'], case['starts'], case['goals'], case['lava'], case['walls'], case['reward'])
        assert GR.cell_classes(spec).dtype == np.uint8
        assert GR.cell_classes(spec).tolist() == want, case['name']
        assert O.classes(g) == want, case['name']
    quirk = next(c for c in cases if c['name'] == 'quirk6x4')  # goal+lava, goal+wall, lava+wall
    spec = GridSpec(quirk['W'], quirk['H'], quirk['starts'], quirk['goals'], quirk['lava'], quirk['walls'], quirk['reward'])
    assert GR.cell_classes(spec)[[7, 13, 9]].tolist() == [3, 3, 2]


@pytest.mark.parametrize('name', sorted(HOST_GRIDS))
def test_host_mirror_equals_the_restatement(name):
    g = HOST_GRIDS[name]()
    spec, W, H = _spec(g), g['W'], g['H']
    cls = O.classes(g)
    for r in RADII:
        table = GR.view_table(spec, r)
        assert table.dtype == np.uint8 and table.shape == (W * H, 2 * r + 1, 2 * r + 1)
        for s in range(W * H):
            assert np.array_equal(table[s], O.ego(cls, W, H, s, r)), (name, r, s)
    assert np.array_equal(GR.view_table(spec, 0).reshape(-1), cls)
    for s in range(W * H):
        view = GR.grid_view(spec, s)
        assert view.dtype == np.uint8 and view.shape == (H, W)
        assert np.array_equal(view, O.whole(cls, W, H, s)), (name, s)


@pytest.mark.parametrize('level, cells, distinct', [('default_env', 16, (12, 16, 16)), ('test_env', 21, (17, 21, 21)),
                                                    ('maze_11x11', 49, (27, 48, 49)), ('maze_21x21', 201, (39, 190, 201))])
def test_distinct_views_over_the_non_wall_cells(level, cells, distinct):
    sp = G.load_json('levels.json')[level + '.txt']
    spec = GridSpec(sp['W'], sp['H'], sp['starts'], sp['goals'], sp['lava'], sp['walls'])
    free = np.flatnonzero(~spec.wall)
    assert len(free) == cells
    cls = O.classes(sp)
    for r, want in zip((1, 2, 3), distinct):
        table = GR.view_table(spec, r)
        assert len({table[s].tobytes() for s in free}) == want, (level, r)
        assert len({O.ego(cls, sp['W'], sp['H'], s, r).tobytes() for s in free}) == want, (level, r)


@pytest.mark.parametrize('name', ['default4x4', 'test_env', 'maze11', 'grid1x9'])
def test_view_features(name):
    g = HOST_GRIDS[name]()
    spec, W, H = _spec(g), g['W'], g['H']
    cls = O.classes(g)
    for r in (0, 1, 2, 3, 7):
        phi, F = view_features(spec, r)
        assert phi.dtype == np.int32 and phi.shape == (W * H, 1)
        views = [O.ego(cls, W, H, s, r).tobytes() for s in range(W * H)]
        for s in range(W * H):
            for t in range(s):
                assert (views[s] == views[t]) == (phi[s, 0] == phi[t, 0]), (name, r, s, t)
        assert F == len(set(views)) == int(phi.max()) + 1
        seen = -1
        for s in range(W * H):  # first-appearance order: a new id is always the next integer
            assert phi[s, 0] <= seen + 1
            seen = max(seen, int(phi[s, 0]))
        if r >= max(W, H) - 1:  # the border of class 4 places the agent
            assert sorted(phi[:, 0].tolist()) == list(range(W * H))
            assert phi[:, 0].tolist() == list(range(W * H))


def test_view_features_reads_a_facade_env():
    env = gua.GridUniverseEnv(custom_world_fp=G.level_path('maze_11x11.txt'))
    phi, F = view_features(env, 1)
    want, wantF = view_features(GridSpec.from_env(env), 1)
    assert np.array_equal(phi, want) and F == wantF
    free = np.flatnonzero(np.asarray(env.wall_grid) != 1)
    assert len(set(phi[free, 0].tolist())) == 27


def test_facade_sense_follows_in_place_edits():
    env = gua.GridUniverseEnv(grid_shape=(5, 4), initial_state=6, goal_states=[19], lava_states=[2], walls=[7, 11])

    def g():
        return dict(W=5, H=4, goals=list(env.goal_states), lava=list(env.lava_states),
                    walls=np.flatnonzero(np.asarray(env.wall_grid) == 1).tolist())

    for r in RADII:
        assert np.array_equal(env.sense(r), O.ego(O.classes(g()), 5, 4, 6, r))
    assert np.array_equal(env.sense(), env.sense(radius=1, mode='ego'))
    assert env.sense(1).tolist() == [[0, 0, 2], [0, 0, 1], [0, 1, 0]]
    assert np.array_equal(env.sense(mode='grid'), O.whole(O.classes(g()), 5, 4, 6))
    env.goal_states.append(5)       # in place
    assert env.sense(1)[1, 0] == 3
    env.wall_grid[1] = 1            # in place
    assert env.sense(1)[0, 1] == 1
    env.goal_states.append(7)       # goal + wall is goal
    assert env.sense(1)[1, 2] == 3
    assert np.array_equal(env.sense(2), O.ego(O.classes(g()), 5, 4, 6, 2))
    env.current_state = 5           # onto the new goal
    assert env.sense(0).tolist() == [[3]]
    assert np.array_equal(env.sense(mode='grid'), O.whole(O.classes(g()), 5, 4, 5))
    assert env.sense(mode='grid')[1, 0] == 3 + 8


@pytest.mark.parametrize('kw', [dict(radius=-1), dict(radius=8), dict(radius=1.5), dict(radius=None), dict(radius=True),
                                dict(mode='egocentric'), dict(mode=0)])
def test_bad_arguments_raise_value_error(kw):
    env = gua.GridUniverseEnv()
    with pytest.raises(ValueError):
        env.sense(**kw)
    spec = GridSpec.from_env(env)
    if 'radius' in kw:
        with pytest.raises(ValueError):
            GR.view_table(spec, kw['radius'])
        with pytest.raises(ValueError):
            view_features(spec, kw['radius'])
    with pytest.raises(ValueError):
        GR.grid_view(spec, 16)
