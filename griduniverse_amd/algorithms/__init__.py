"""Algorithms on the engine.  The modules mirror the reference's core.algorithms and add the build-defined learners; import them by
name (`from griduniverse_amd.algorithms import dyna`).  `rollout_search`, `tree_search`, `uct_tables`, `ucb_q_learning`,
`thompson_q_learning`, `off_policy_mc_control`, `ratio_table`, `view_features` and `prioritized_sweeping` are also reachable here."""


def __getattr__(name):  # lazy: the learner modules import the ctypes binding
    if name in ('rollout_search', 'tree_search', 'uct_tables'):
        from . import search
        return getattr(search, name)
    if name in ('ucb_q_learning', 'thompson_q_learning'):
        from . import exploration
        return getattr(exploration, name)
    if name in ('off_policy_mc_control', 'ratio_table'):
        from . import off_policy
        return getattr(off_policy, name)
    if name == 'prioritized_sweeping':
        from . import dyna
        return dyna.prioritized_sweeping
    if name == 'view_features':
        from . import function_approximation
        return function_approximation.view_features
    raise AttributeError(name)
