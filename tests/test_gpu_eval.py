"""Batched greedy evaluation on the device (gu_td_evaluate, csrc/gu_eval.hip) against the CPU restatement tests/_eval_oracle.py: all
six arrays compared as bytes.  The cases of the main matrix, their tables and the conditions that keep them from being vacuous are
tests/_eval_cases.py's; tests/test_eval_host.py holds those conditions without a device."""
import numpy as np
import pytest

import griduniverse_amd as gua
from griduniverse_amd.algorithms import evaluation
from griduniverse_amd.engine import Engine
from griduniverse_amd.grid import GridSpec
from oracle import c_oracle as C

from . import _eval_cases as EC
from . import _eval_oracle as EO
from . import _overlay_starts as OS
from . import _td_oracle as TD
from ._overlays import overlay
from ._tabular_cases import _grid, _random_grids, _spec, code, open_grid
from ._walks import _greedy_walk_lengths, _shortest_from_start

pytestmark = pytest.mark.gpu

K, L, GAMMA, N, SEED = EC.K, EC.L, EC.GAMMA, EC.N, EC.SEED
RIGHT = 1


def _os_spec(name):
    g = OS.grid_dict(name)
    return GridSpec(g['W'], g['H'], g['starts'], g['goals'], g['lava'], g['walls'])


def _batch(kind, name, env_id0, n=N):
    vec = gua.VecGridUniverse(n, template=_os_spec(name), seed=SEED, env_id0=env_id0)
    if kind is not None:
        overlay(kind).install(vec.engine, OS.plane(kind, name), *OS.extra(kind, name))
    return vec


def _install_tables(vec, q):
    if isinstance(q, EO.Shared):
        for e in range(vec.num_envs):  # one table at a time: the batch's tables never stand on the host together
            vec.set_q_table(q.table(e), env0=e)
    else:
        vec.set_q_table(q)


# ---- the main matrix ----
@pytest.mark.parametrize('env_id0', EC.IDS)
@pytest.mark.parametrize('kind,grid', EC.CASES)
def test_evaluation_equals_the_oracle(kind, grid, env_id0):
    vec = _batch(kind, grid, env_id0)
    try:
        _install_tables(vec, EC.table(kind, grid, env_id0))
        log = EO.new_log()
        EO.same(vec.evaluate(K, L, GAMMA), EC.restate(kind, grid, env_id0, None, log))
        first = EC.first_states(kind, grid)
        if first is not None:
            EO.same(vec.evaluate(K, L, GAMMA, first), EC.restate(kind, grid, env_id0, first, log))
        EC.not_vacuous(kind, grid, log)
    finally:
        vec.close()


def test_one_env_ends_at_step_1_while_its_wave_runs_to_L():
    g = open_grid(8, 8)
    grid, n, early = _grid(g), N, 70  # env 70: the second wave
    q = np.zeros((n, 64, 4))
    q[early, 62, RIGHT] = 1.0  # beside the goal, towards it; every other row: UP for ever
    first = np.zeros((K, n), np.int32)
    first[:, early] = 62
    vec = gua.VecGridUniverse(n, template=_spec(g), seed=SEED)
    try:
        vec.set_q_table(q)
        got = vec.evaluate(K, L, GAMMA, first)
        EO.same(got, EO.evaluate_calm(grid, SEED, n, 0, q, K, L, GAMMA, first))
        others = np.arange(n) != early
        assert (got['length'][:, early] == 1).all() and (got['outcome'][:, early] == 1).all() and (got['length'][:, others] == L).all()
    finally:
        vec.close()


# ---- several grids, calm ----
def _trained(grids, seed, group, steps=200):
    """One restated learner group per grid (envs k * group ..), trained from small random integers."""
    rs = np.random.RandomState(11)
    out = []
    for k, g in enumerate(grids):
        o = TD.TdOracle(g, seed, group, env_id0=k * group)
        o.q[:] = rs.randint(0, 3, o.q.shape)
        o.reset()
        o.run(steps, TD.Q_LEARNING, 0.5, 0.9, EC.EPS_Q16)
        out.append(o)
    return out


def _side_by_side(learners, seed, group, Kk, Ll):
    parts = [EO.evaluate_calm(o.grid, seed, group, k * group, o.q, Kk, Ll, GAMMA) for k, o in enumerate(learners)]
    return {key: np.concatenate([p[key] for p in parts], axis=1) for key in EO.KEYS}


@pytest.mark.parametrize('n_grids,n,W', [(4, 256, 9), (130, 130, 7)])  # groups of 64 (LDS-staged maps), one grid per env (global maps)
def test_multigrid_evaluation_equals_the_oracle(n_grids, n, W):
    dicts = _random_grids(n_grids, W, W, 17)
    learners = _trained([_grid(g) for g in dicts], SEED, n // n_grids)
    vec = gua.VecGridUniverse(n, templates=[_spec(g) for g in dicts], seed=SEED)
    try:
        vec.set_q_table(np.concatenate([o.q for o in learners]))
        got = vec.evaluate(K, L, GAMMA)
        EO.same(got, _side_by_side(learners, SEED, n // n_grids, K, L))
        assert {0, 1} <= set(got['outcome'].ravel().tolist())
    finally:
        vec.close()


def test_device_maze_evaluation_equals_the_oracle_on_the_grids_read_back():
    n, W = 130, 8
    vec = gua.VecGridUniverse(n, grid_shape=(W, W), device_mazes=n, maze_seed=31, seed=SEED)
    try:
        grids = []
        for k in range(n):
            flags, reward, starts = vec.engine.get_cells(k)
            term, goal = (flags & 0x10) != 0, reward > 0
            grids.append(C.Grid(W, W, (flags & 0x80) != 0, term & ~goal, term & goal, reward.astype(np.int32), starts))
        learners = _trained(grids, SEED, 1)
        vec.set_q_table(np.concatenate([o.q for o in learners]))
        got = vec.evaluate(K, L, GAMMA)
        EO.same(got, _side_by_side(learners, SEED, 1, K, L))
        assert {0, 1} <= set(got['outcome'].ravel().tolist())
    finally:
        vec.close()


# ---- first_state ----
def test_first_state_walks_one_table_from_every_cell():
    g = EC.OS.grid_dict('starts8')
    grid, S = OS.c_grid('starts8'), 64
    q = EC.table(None, 'starts8', 0)[3]
    tables = np.repeat(q[None], S, axis=0)
    first = np.arange(S, dtype=np.int32)[None]
    vec = gua.VecGridUniverse(S, template=_os_spec('starts8'), seed=SEED)
    try:
        vec.set_q_table(tables)
        got = vec.evaluate(1, S, GAMMA, first)
        EO.same(got, EO.evaluate_calm(grid, SEED, S, 0, tables, 1, S, GAMMA, first))
        walks = _greedy_walk_lengths(grid, q)
        reached = got['outcome'][0] == 1
        assert reached.any() and np.array_equal(got['length'][0][reached], walks[reached]) and (walks[~reached] == -1).all()
        one = evaluation.evaluate(_os_spec('starts8'), q, episodes=1, max_steps=S, discount_factor=GAMMA, seed=SEED, first_state=[5])
        assert all(one[k].shape == (1,) and one[k][0] == got[k][0, 5] for k in EO.KEYS)
    finally:
        vec.close()
    assert g['goals']


# ---- nothing is disturbed ----
def _everything(vec, kind):
    out = dict(q=vec.q_table().tobytes(), done=vec.engine.done_indices().tobytes(), stores=vec.engine.stores())
    out.update({k: v.tobytes() for k, v in vec.get_state().items()})
    if kind is not None:
        masks = overlay(kind).masks(vec.engine)
        out['masks'] = None if masks is None else masks.tobytes()
    return out


@pytest.mark.parametrize('kind,grid,run', [(None, 'starts8', 'td'), (None, 'starts8', 'nstep'), (None, 'starts8', 'lambda'), ('fruit', 'starts8', 'td')])
def test_an_evaluation_between_two_launches_disturbs_nothing(kind, grid, run):
    launch = {'td': lambda v, T: v.td_run(T, 'sarsa', alpha=0.25, discount_factor=0.9, epsilon=0.3, trajectory=True, stats=True),
              'nstep': lambda v, T: v.nstep_run(T, n=4, method='sarsa', alpha=0.25, discount_factor=0.9, epsilon=0.3, trajectory=True, stats=True),
              'lambda': lambda v, T: v.lambda_run(T, alpha=0.25, discount_factor=0.9, epsilon=0.3, trajectory=True, stats=True)}[run]
    results = []
    for evaluate in (False, True):
        vec = _batch(kind, grid, 0)
        try:
            vec.reset()
            first = launch(vec, 70)
            if evaluate:
                before = _everything(vec, kind)
                got = vec.evaluate(K, L, GAMMA)
                assert (got['length'] > 0).any()
                after = _everything(vec, kind)
                assert before == after
            second = launch(vec, 50)
            results.append((first, second, _everything(vec, kind)))
        finally:
            vec.close()
    (a1, a2, a_end), (b1, b2, b_end) = results
    for a, b in ((a1, b1), (a2, b2)):
        assert sorted(a) == sorted(b) and all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a)
    assert a_end == b_end


def test_the_test_episodes_of_one_start_without_gusts_are_equal():
    g = open_grid(4, 4)
    o = _trained([_grid(g)], SEED, N, steps=300)[0]
    vec = gua.VecGridUniverse(N, template=_spec(g), seed=SEED)
    try:
        vec.set_q_table(o.q)
        got = vec.evaluate(4, L, GAMMA)
        for key in EO.KEYS:
            assert (got[key] == got[key][0]).all(), key
        assert {0, 1} <= set(got['outcome'][0].tolist())  # (the learners differ: some walks reach the goal, others loop)
    finally:
        vec.close()


# ---- errors ----
def _raw(eng, Kk, Ll, gamma, first, out):
    p = gua._lib.ptr
    return eng.lib.gu_td_evaluate(eng._h, Kk, Ll, gamma, p(first), *(p(out[k]) for k in ('ret', 'len', 'outcome', 'end', 'word', 'disc')))


def test_errors_leave_the_callers_arrays_alone():
    g = open_grid(8, 8)
    n = 8
    out = {k: np.full((2, n), 77, np.int32) for k in ('ret', 'len', 'outcome', 'end')}
    out['word'], out['disc'] = np.full((2, n), 77, np.uint32), np.full((2, n), 77.0)
    with Engine(n, _spec(g)) as eng:
        assert _raw(eng, 2, 5, 0.9, None, out) == -4 and 'gu_td_init' in gua._lib.last_error()  # GU_ERR_STATE: no tables
        eng.td_init(0.0)
        bad = np.zeros((2, n), np.int32)
        bad[1, 3] = 64
        for args, fragment in (((0, 5, 0.9, None), 'K 0'), ((2, 0, 0.9, None), 'L 0'), ((2, 50000001, 0.9, None), '1e8'),
                               ((65536, 1, 0.9, None), 'test episodes'), ((2, 5, float('nan'), None), 'gamma'), ((2, 5, float('inf'), None), 'gamma'),
                               ((2, 5, 0.9, bad), 'first_state[1][3] = 64'), ((2, 5, 0.9, bad - 1), 'first_state[0][0] = -1')):
            assert _raw(eng, *args, out) == -1, args
            assert fragment in gua._lib.last_error(), (args, gua._lib.last_error())
        assert all((v == 77).all() for v in out.values())
        assert _raw(eng, 2, 5, 0.9, None, dict(out, ret=None, word=None, disc=None)) == 0  # any output may be NULL
        assert (out['len'] == 5).all() and (out['ret'] == 77).all() and (out['disc'] == 77.0).all()
    with Engine(1 << 20, _spec(g)) as eng:
        eng.td_init(0.0)
        assert code(lambda: eng.td_evaluate(17, 5)) == -1 and 'test episodes' in gua._lib.last_error()  # 17 x 2^20 > 2^24
        assert (eng.td_evaluate(16, 2)['len'] == 2).all()  # ... and 2^24 of them run


# ---- the learning claim (tests/_eval_oracle.py: CLAIM_*) ----
def test_every_learner_of_64_mazes_walks_a_shortest_path():
    dicts = EO.claim_grids()
    assert len({tuple(g['walls']) for g in dicts}) == EO.CLAIM_LEVELS  # 64 distinct levels
    vec = gua.VecGridUniverse(EO.CLAIM_LEVELS, templates=[_spec(g) for g in dicts], seed=0)
    try:
        vec.reset()
        vec.td_run(EO.CLAIM_STEPS, 'q_learning', alpha=EO.CLAIM_ALPHA, discount_factor=EO.CLAIM_GAMMA, epsilon=EO.CLAIM_EPS_Q16 / 65536.0)
        got = vec.evaluate()
        best = np.array([_shortest_from_start(_grid(g)) for g in dicts])
        assert (got['outcome'][0] == 1).all() and np.array_equal(got['length'][0], best)
        assert evaluation.success(got).tolist() == [1.0] * EO.CLAIM_LEVELS
        paths, _ = vec.engine.shortest_paths()
        assert [len(p) for p in paths] == best.tolist()
    finally:
        vec.close()
