"""Greedy evaluation of learned Q tables on the device (include/gu.h: gu_td_evaluate; csrc/gu_eval.hip): every learner walks test
episodes on its own table with the move rule it learned under, the overlay's included, and nothing learns.  This is the learners'
side of a comparison whose other side `VecGridUniverse.shortest_paths()` gives: how many reach the goal, and how many on a
shortest path.

`evaluate` takes the tables that `q_learning(...)`, `fa_q_table()` and the other learners return, `success` turns a result into
the share of test episodes that ended well per learner, and `learning_curve` alternates training launches of a batch with
evaluations of it.  A pair of Double Q-learning tables or actor-critic preferences can be folded into one table first.
"""
import numpy as np

from ..vec_env import VecGridUniverse, check_evaluate_args
from .temporal_difference import overlay_installer

KEYS = ('ret', 'length', 'outcome', 'end', 'word', 'discounted')


def evaluate(env, q, episodes=1, max_steps=None, discount_factor=1.0, seed=0, wind=None, gust=0.0, fruit=None, doors=None, boxes=None,
             errands=None, first_state=None):
    """Greedy test episodes of the tables `q` -- float64 [S', 4] for one learner or [L, S', 4] for L of them, S' the rows the learner
    had (S, or S << bits under fruit, doors, boxes and errands) -- on the grid of `env`, learner e in env e of a batch seeded with
    `seed`, under the overlay that the keywords name as `q_learning` takes them.  `episodes`, `max_steps`, `discount_factor` and
    `first_state` as VecGridUniverse.evaluate takes them.  Returns its dict, of [episodes, L] arrays, or of [episodes] arrays for one
    table."""
    q = np.asarray(q, np.float64)
    if q.ndim not in (2, 3) or q.shape[-1] != 4:
        raise ValueError('q must have shape (S, 4) or (L, S, 4), got {}'.format(q.shape))
    one = q.ndim == 2
    tables = q[None] if one else q
    if tables.shape[0] < 1:
        raise ValueError('q must hold at least one table')
    install = overlay_installer(wind, gust, fruit, doors, boxes, errands)
    if first_state is not None and one:
        first_state = np.asarray(first_state).reshape(-1, 1)
    check_evaluate_args(episodes, max_steps, discount_factor, first_state, tables.shape[0], None)
    vec = VecGridUniverse(tables.shape[0], template=env, seed=seed)
    try:
        install(vec)
        vec.set_q_table(tables)
        out = vec.evaluate(episodes, max_steps, discount_factor, first_state)
    finally:
        vec.close()
    return {k: v[:, 0] for k, v in out.items()} if one else out


def success(result):
    """float64 per learner: the share of its test episodes that reached a goal (outcome 1) or that the overlay ended (outcome 3: boxes
    solved, errand completed)."""
    o = np.asarray(result['outcome'])
    return ((o == 1) | (o == 3)).mean(axis=0)


def learning_curve(vec, launch, total_steps, every, **evaluate_kwargs):
    """Train and measure in turn: `launch(vec, every)` (for instance lambda vec, T: vec.td_run(T)) and then
    vec.evaluate(**evaluate_kwargs), until `total_steps` steps are trained (the last launch may be shorter).  Returns a dict with
    `steps` int64[P], the steps trained before each measurement, and every array of evaluate() stacked as [P, episodes, N]."""
    total_steps, every = int(total_steps), int(every)
    if total_steps < 1 or every < 1:
        raise ValueError('total_steps and every must be at least 1')
    steps, points = [], []
    done = 0
    while done < total_steps:
        T = min(every, total_steps - done)
        launch(vec, T)
        done += T
        steps.append(done)
        points.append(vec.evaluate(**evaluate_kwargs))
    out = {k: np.stack([p[k] for p in points]) for k in KEYS}
    out['steps'] = np.array(steps, np.int64)
    return out
