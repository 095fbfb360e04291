"""The sensor rule (include/gu.h: gu_sense) restated one cell at a time, for tests/test_sense_host.py and tests/test_gpu_sense.py.

Nothing here goes through griduniverse_amd.grid: no padding, no windows.  A grid is a dict with W, H and the lists goals, lava,
walls (tests/_tabular_cases.py: GRIDS); the class of a cell is the reference viewer's tile rule (core/envs/rendering.py:119-133)."""
import numpy as np

GROUND, WALL, LAVA, GOAL, OUTSIDE, AGENT = 0, 1, 2, 3, 4, 8


def classes(g):
    """[S] ints: goal -> 3, else lava -> 2, else wall -> 1, else ground -> 0."""
    goals, lava, walls = set(g['goals']), set(g['lava']), set(g['walls'])
    out = []
    for s in range(g['W'] * g['H']):
        if s in goals:
            out.append(GOAL)
        elif s in lava:
            out.append(LAVA)
        elif s in walls:
            out.append(WALL)
        else:
            out.append(GROUND)
    return out


def classes_from_flags(flags):
    """The same from the cell flags of a device-generated maze (one goal, no lava, the goal never on a wall): bit 4 terminal,
    bit 6 reward -10, bit 7 wall."""
    out = []
    for f in flags:
        f = int(f)
        if f & 0x10:
            out.append(LAVA if f & 0x40 else GOAL)
        else:
            out.append(WALL if f & 0x80 else GROUND)
    return out


def ego(cls, W, H, pos, r):
    """uint8[K, K]: the view of radius r from cell pos."""
    y, x = divmod(int(pos), W)
    K = 2 * r + 1
    view = np.empty((K, K), np.uint8)
    for dy in range(K):
        for dx in range(K):
            yy, xx = y + dy - r, x + dx - r
            view[dy, dx] = cls[yy * W + xx] if 0 <= yy < H and 0 <= xx < W else OUTSIDE
    return view


def whole(cls, W, H, pos):
    """uint8[H, W]: every cell's class, plus 8 on the agent's."""
    view = np.empty((H, W), np.uint8)
    for y in range(H):
        for x in range(W):
            s = y * W + x
            view[y, x] = cls[s] + (AGENT if s == int(pos) else 0)
    return view


def views(cls, W, H, positions, r=None):
    """The views of an array of positions of any shape, [..., K, K] (r given) or [..., H, W] (r None); equal positions are
    restated once."""
    positions = np.asarray(positions)
    memo = {}
    for p in np.unique(positions):
        memo[int(p)] = whole(cls, W, H, p) if r is None else ego(cls, W, H, p, r)
    shape = (H, W) if r is None else (2 * r + 1, 2 * r + 1)
    out = np.empty(positions.shape + shape, np.uint8)
    for idx in np.ndindex(positions.shape):
        out[idx] = memo[int(positions[idx])]
    return out
