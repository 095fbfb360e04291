"""Structural invariants of recursive-backtracker mazes, checked (a) on mazes captured from the REFERENCE
generator and (b) on the CPU restatement of the on-device generator -- the two draw from different RNGs, so
they are compared by structure, not cell by cell."""
import numpy as np
import pytest

from oracle import c_oracle as C
from tests import _golden as G
from tests._mazes import check_maze_structure


@pytest.mark.parametrize('key', sorted(G.load_json('mazes.json')))
def test_reference_mazes_have_the_structure(key):
    m = G.load_json('mazes.json')[key]
    wall = np.array([[c == '#' for c in row] for row in m['rows']])
    check_maze_structure(wall, m['start'][0], m['goal'][0])
    assert wall.sum() == m['n_walls']


@pytest.mark.parametrize('W,H', [(8, 8), (11, 11), (7, 5), (5, 7), (32, 32), (64, 64), (21, 13), (4, 1), (1, 6)])
def test_restated_device_generator_has_the_structure(W, H):
    counts = set()
    for gid in range(12):
        wall, start, goal = C.generate_maze(77, gid, W, H)
        check_maze_structure(wall.reshape(H, W), start, goal)
        counts.add(int(wall.sum()))
    ref = {m['n_walls'] for k, m in G.load_json('mazes.json').items() if (m['W'], m['H']) == (W, H)}
    if ref and W % 2 == 0 and H % 2 == 0:
        assert counts == ref  # even sizes: the wall count does not depend on the origin (32x32 -> 513, 64x64 -> 2049)


def test_generator_is_keyed_by_seed_and_grid_id():
    a = C.generate_maze(1, 0, 16, 16)
    assert all(np.array_equal(x, y) for x, y in zip(a, C.generate_maze(1, 0, 16, 16)))
    assert not np.array_equal(a[0], C.generate_maze(1, 1, 16, 16)[0])
    assert not np.array_equal(a[0], C.generate_maze(2, 0, 16, 16)[0])
    with pytest.raises(ValueError):
        C.generate_maze(1, 0, 2, 2)
