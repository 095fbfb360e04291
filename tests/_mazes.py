"""Grids for the engine-level tests: random specs with their oracle grids, and the structure every generated maze must have."""
import numpy as np

from griduniverse_amd.grid import GridSpec
from oracle import c_oracle as C


def check_maze_structure(wall, start, goal):
    """wall: bool[H, W].  Rooms = open cells sharing the parity of some origin; every open cell is a room or a
    passage between two rooms two apart; the open cells form a tree (|open| = 2*|rooms| - 1, connected)."""
    H, W = wall.shape
    open_cells = np.argwhere(~wall)
    assert len(open_cells) >= 2 and start != goal and not wall.ravel()[start] and not wall.ravel()[goal], (
        'fewer than two open cells, or start %d / goal %d equal or walled' % (start, goal))
    parities = {}
    for py in (0, 1):
        for px in (0, 1):
            rooms = [(y, x) for y, x in open_cells if y % 2 == py and x % 2 == px]
            others = [(y, x) for y, x in open_cells if not (y % 2 == py and x % 2 == px)]
            if all((y % 2 == py) != (x % 2 == px) for y, x in others) and len(open_cells) == 2 * len(rooms) - 1:
                parities[(py, px)] = rooms
    assert parities, 'open cells are not rooms of one parity class plus single passages'
    # connectivity by flood fill over 4-neighbours
    seen, todo = set(), [tuple(open_cells[0])]
    while todo:
        y, x = todo.pop()
        if (y, x) in seen:
            continue
        seen.add((y, x))
        for dy, dx in ((1, 0), (-1, 0), (0, 1), (0, -1)):
            ny, nx = y + dy, x + dx
            if 0 <= ny < H and 0 <= nx < W and not wall[ny, nx] and (ny, nx) not in seen:
                todo.append((ny, nx))
    assert len(seen) == len(open_cells), 'maze is not connected'
    # every reachable room of the parity class was carved (the DFS exhausts them)
    (py, px), rooms = next(iter(parities.items()))
    assert len(rooms) == len(range(py, H, 2)) * len(range(px, W, 2)), 'a room of parity (%d, %d) was not carved' % (py, px)


def oracle_grid(spec):
    return C.Grid(spec.W, spec.H, spec.wall, spec.lava, spec.goal, spec.reward, spec.starts)


def random_specs(rs, n, W, H):
    S, specs = W * H, []
    for _ in range(n):
        pick = lambda k: [int(x) for x in rs.choice(S, size=int(k), replace=False)]  # noqa: E731
        specs.append(GridSpec(W, H, pick(rs.randint(1, 4)), pick(rs.randint(1, 3)), pick(rs.randint(0, 5)), pick(rs.randint(0, S // 4))))
    return specs
