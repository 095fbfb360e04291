"""The learner batch behind every function of this package that learns on the device: L learners on the grid of a facade
`GridUniverseEnv`, learner e in env e of a `VecGridUniverse`, advanced in launches of bounded length.  A function supplies what is its
own -- how the batch is prepared, what one launch is, what is read at the end -- and the argument checks it shares with the others
are here too.
"""
from ..vec_env import VecGridUniverse
from ..vec_env import _unit as unit  # unit(name, x): x lies in [0, 1] (ValueError), the facade's own check and message

_CHUNK = 100000  # steps per launch (the launch limit is 1e8; shorter launches keep the device responsive)


def need_learners(num_learners):
    """int(num_learners), at least 1 (ValueError)."""
    L = int(num_learners)
    if L < 1:
        raise ValueError('num_learners must be at least 1')
    return L


def need_steps(num_steps):
    if int(num_steps) < 0:
        raise ValueError('num_steps must not be negative')


def need_finite(**values):
    """Every keyword's value is finite, reported in the order given (ValueError)."""
    for name, x in values.items():
        if not float('-inf') < float(x) < float('inf'):
            raise ValueError('{} must be finite'.format(name))


def learn(env, num_learners, seed, num_steps, chunk, prepare, launch, read=lambda vec: vec.q_table()):
    """`num_steps` real steps of L = num_learners learners on the grid of `env`: `prepare(vec)` makes the fresh batch ready (tables,
    models, features, an overlay), every env is reset, `launch(vec, T)` runs T steps at a time, at most `chunk`, and `read(vec)`
    gives the result: an array [L, ...] or a tuple of them.  Returns it for L > 1 and its entry 0 (of each array) for L = 1."""
    L = int(num_learners)
    vec = VecGridUniverse(L, template=env, seed=seed)
    try:
        prepare(vec)
        vec.reset()
        left = int(num_steps)
        while left > 0:
            T = min(left, chunk)
            launch(vec, T)
            left -= T
        out = read(vec)
    finally:
        vec.close()
    if L > 1:
        return out
    return tuple(a[0] for a in out) if isinstance(out, tuple) else out[0]
