"""Path lengths on a grid, by search and by walking a table's greedy policy: what the host and device tests of the learners measure
a learned table against."""
from collections import deque

import numpy as np

from oracle import c_oracle as C


def _bfs_lengths(grid):
    """Shortest number of steps from every cell to a terminal cell (backwards BFS over the move rule); -1 unreachable."""
    S = grid.S
    s = np.repeat(np.arange(S, dtype=np.int32), 4)
    a = np.tile(np.arange(4, dtype=np.int32), S)
    nxt, _, _ = C.look_step_ahead(grid, s, a, True)
    term = (grid.goal | grid.lava).astype(bool)
    dist = np.full(S, -1)
    dist[term] = 0
    pred = [[] for _ in range(S)]
    for i in range(S * 4):
        if nxt[i] != s[i]:
            pred[nxt[i]].append(s[i])
    q = deque(np.flatnonzero(term).tolist())
    while q:
        c = q.popleft()
        for p in pred[c]:
            if dist[p] < 0 and not term[p]:
                dist[p] = dist[c] + 1
                q.append(p)
    return dist


def _greedy_walk_lengths(grid, q):
    S = grid.S
    out = np.full(S, -1)
    for s0 in range(S):
        s, n = s0, 0
        while not (grid.goal[s] or grid.lava[s]) and n <= S:
            nxt, _, _ = C.look_step_ahead(grid, np.array([s], np.int32), np.array([int(np.argmax(q[s]))], np.int32), True)
            s, n = int(nxt[0]), n + 1
        out[s0] = n if grid.goal[s] else -1
    return out


def _shortest_from_start(grid):
    S = grid.S
    s = np.repeat(np.arange(S, dtype=np.int32), 4)
    a = np.tile(np.arange(4, dtype=np.int32), S)
    nxt = C.look_step_ahead(grid, s, a, True)[0].reshape(S, 4)
    dist = {int(grid.starts[0]): 0}
    frontier = [int(grid.starts[0])]
    while frontier:
        nf = []
        for c in frontier:
            if grid.goal[c] or grid.lava[c]:
                continue
            for b in range(4):
                n = int(nxt[c, b])
                if n not in dist:
                    dist[n] = dist[c] + 1
                    nf.append(n)
        frontier = nf
    return min(v for k, v in dist.items() if grid.goal[k])


def _greedy_walk(grid, q):
    s, n = int(grid.starts[0]), 0
    while not (grid.goal[s] or grid.lava[s]) and n <= grid.S:
        nxt, _, _ = C.look_step_ahead(grid, np.array([s], np.int32), np.array([int(np.argmax(q[s]))], np.int32), True)
        s, n = int(nxt[0]), n + 1
    return n if grid.goal[s] else -1
