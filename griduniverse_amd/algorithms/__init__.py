"""Algorithms on the engine.  The modules mirror the reference's core.algorithms and add the build-defined learners; import them by
name (`from griduniverse_amd.algorithms import dyna`).  `rollout_search`, `ucb_q_learning` and `thompson_q_learning` are also
reachable here."""


def __getattr__(name):  # lazy: the learner modules import the ctypes binding
    if name == 'rollout_search':
        from .search import rollout_search
        return rollout_search
    if name in ('ucb_q_learning', 'thompson_q_learning'):
        from . import exploration
        return getattr(exploration, name)
    raise AttributeError(name)
