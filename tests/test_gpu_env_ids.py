"""Every learner entry point on an engine that is a shard: its first env has a global id other than 0 (VecGridUniverse(..., env_id0=),
gu_create).  Every RNG stream is keyed by env_id0 + e and every per-env store is indexed by the local e; TabLane::begin
(csrc/gu_tabular.hpp) derives the env key of streams 1 and 4, and gu_dyna.hip, gu_search.hip and gu_mcts.hip key streams 5, 6 and 8
by it.  A kernel that dropped the offset, indexed a store by the global id, or sign-extended an id above 2^31 passes every other test
of the learners: they all run at env_id0 = 0.

1 -- every learner of tests/_learners.py::LEARNERS against its CPU restatement built at the same id (_against_restatement: two
launches, rows, statistics, env state and every store by bytes) at the ids of _learners.env_ids: 77, 2^31 - 40 (the batch straddles
bit 31) and 2^32 - 1 - N (the highest gu_create admits).  The grid is GRIDS['test_env'], 3 x 8 with two starts and three lava cells:
episodes end within a few steps and the start draw matters.  N = 130: three waves, the last partial.  Each case asserts on the
restatement alone that it compared something (_a_shard_worth_comparing; tests/test_env_ids_host.py holds the same without a device).
2 -- the shard property, with no restatement: one engine of 192 envs at 2^31 - 96 equals three engines of 64 envs at 2^31 - 96,
2^31 - 32 and 2^31 + 32, slice by slice.
3 -- setters and getters take local env indices on a shard."""
import functools

import numpy as np
import pytest

from ._learners import (LEARNERS, _a_shard_worth_comparing, _against_restatement, _launch, _open, _restated, _same_state, _same_stores,
                        _tables_for_setter, env_ids)
from ._tabular_cases import GRIDS, _grid, _same

pytestmark = pytest.mark.gpu

N, SEED = 130, 3
KEYS = ('obs', 'reward', 'done', 'ret', 'episodes')


def _g():
    return GRIDS['test_env']()


@functools.lru_cache(maxsize=None)
def _at_id_0(name):
    """The restatement of learner `name` at env_id0 = 0: what the rows at another id must differ from."""
    return _restated(LEARNERS[name], _g(), N, SEED, 0)


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize('env_id0', env_ids(N))
@pytest.mark.parametrize('name', sorted(LEARNERS))
def test_a_learner_on_a_shard_equals_its_restatement_at_the_same_ids(name, env_id0):
    assert env_id0 + N <= 0xFFFFFFFF
    ran = _against_restatement(LEARNERS[name], _g(), N, SEED, env_id0)
    _a_shard_worth_comparing(LEARNERS[name], _g(), ran, _at_id_0(name))


# ---------------------------------------------------------------------------------------------------------------- 2
def _ran_on_a_shard(learner, n, env_id0):
    """Everything the launches of learner.T leave on an engine of n envs at env_id0; the stores in groups of 64 envs."""
    vec = _open(n, _g(), SEED, learner, env_id0)
    try:
        out = dict(first=np.array(vec.reset()), rows=[])
        for T in learner.T:
            got = _launch(vec, learner, T, trajectory=True, stats=True)
            out['rows'].append(dict((k, np.array(got[k])) for k in KEYS))
        out['state'] = dict((k, np.array(v)) for k, v in vec.get_state().items())
        out['stores'] = [learner.got(vec, e0, 64) for e0 in range(0, n, 64)]
        return out
    finally:
        vec.close()


@pytest.mark.parametrize('name', sorted(LEARNERS))
def test_one_engine_equals_its_three_shards(name):
    learner, base = LEARNERS[name], 2 ** 31 - 96
    whole = _ran_on_a_shard(learner, 192, base)
    assert len(set(whole['first'].tolist())) > 1 and sum(int(r['episodes'].sum()) for r in whole['rows']) > 0
    for k in range(3):
        cols = slice(64 * k, 64 * k + 64)
        shard = _ran_on_a_shard(learner, 64, base + 64 * k)
        assert np.array_equal(whole['first'][cols], shard['first']), k
        for a, b in zip(whole['rows'], shard['rows']):
            for key in KEYS:
                assert a[key][..., cols].tobytes() == b[key].tobytes(), (k, key)
        for key in ('pos', 'done', 'episode', 'tcount'):
            assert np.array_equal(whole['state'][key][cols], shard['state'][key]), (k, key)
        _same_stores(whole['stores'][k], shard['stores'][0], k)


# ---------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize('name', sorted(name for name, learner in LEARNERS.items() if learner.install is not None))
def test_setters_and_getters_take_local_env_indices_on_a_shard(name):
    """Tables for 100 envs installed at env0 = 3 of the engine at 2^31 - 40, read back, and learned on."""
    learner, env_id0, env0, width = LEARNERS[name], 2 ** 31 - 40, 3, 100
    vec = _open(N, _g(), SEED, learner, env_id0)
    try:
        o = learner.oracle(_grid(_g()), SEED, N, env_id0)
        assert np.array_equal(vec.reset(), o.reset())
        _same(_launch(vec, learner, learner.T[0], trajectory=True, stats=True), learner.restate(o, learner.T[0]))
        tables = dict((k, t[:width]) for k, t in _tables_for_setter(learner, o).items())  # (env e of the tables goes to env e + 3)
        learner.install(vec, tables, env0)
        learner.restate_install(o, tables, env0)
        got = learner.got(vec, env0, width)
        for k, t in tables.items():
            assert got[k].tobytes() == np.asarray(t).astype(got[k].dtype, copy=False).tobytes(), k
        _same_stores(learner.got(vec, 0, N), learner.want(o), 'installed')
        _same(_launch(vec, learner, learner.T[1], trajectory=True, stats=True), learner.restate(o, learner.T[1]))
        _same_stores(learner.got(vec, 0, N), learner.want(o), 'after the setter')
        _same_state(vec.get_state(), o, 0, 'after the setter')
    finally:
        vec.close()
