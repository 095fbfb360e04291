"""Wind on the device (gu_set_wind; csrc/gu_wind.hip and the windy gu_td_kernel instantiations) against the CPU restatement
tests/_wind_oracle.py: step, rollout and td_run compared byte for byte, and the calm plane against the calm engine.  (The calls
that have no windy form: tests/test_gpu_overlay.py.)"""
import functools

import numpy as np
import pytest

import griduniverse_amd as gua
from griduniverse_amd import _lib
from griduniverse_amd.algorithms.temporal_difference import q_learning
from griduniverse_amd.grid import wind_plane
from oracle import c_oracle as C

from . import _golden as G
from . import _td_oracle as TD
from . import _wind_oracle as O
from ._overlays import METHODS, policy_table as _policy_table, same_state, scatter as _scatter
from ._tabular_cases import GRIDS, _eps, _grid, _same, _spec, counts_near_2_32

pytestmark = pytest.mark.gpu

GUSTS = [0, O.GUST_THIRDS]
_same_state = functools.partial(same_state, kind='wind')


@functools.lru_cache(maxsize=None)
def _case(name):
    """(grid dict, wind plane uint8[S]).  'book': Sutton & Barto's grid.  'maze11': the 11 x 11 maze with lava on some corridor cells and
    random directions and strengths up to 3 -- walls stop pushes, agents are blown into lava.  'open150': 150 x 150 cells without
    walls, three starts, lava sprinkled: two planes fit 64 KiB of LDS there and three (67 536 bytes) do not -- the L2 kernels."""
    if name == 'book':
        return dict(O.BOOK), wind_plane(O.BOOK_W, O.BOOK_H, O.BOOK_STRENGTH)
    rs = np.random.RandomState(5)
    if name == 'maze11':
        g = GRIDS['maze11']()
        free = [s for s in range(g['W'] * g['H']) if s not in set(g['walls']) | set(g['starts']) | set(g['goals'])]
        g['lava'] = free[4::9]
    else:
        W = H = 150
        S = W * H
        g = dict(W=W, H=H, starts=[0, 75 * W + 75, 20 * W + 140], goals=[S - 1, 76 * W + 80], lava=list(range(7, S - 1, 97)), walls=[])
        assert 2 * ((S + 15) & ~15) <= 65536 < 3 * ((S + 15) & ~15) == 67536
    shape = (g['H'], g['W'])
    return g, wind_plane(g['W'], g['H'], rs.randint(0, 4, shape), rs.randint(0, 4, shape))


CASES = ['book', 'maze11', 'open150']


def _pair(name, N, seed, gust_q16, q0=None, wind=True):
    """A batch of N envs on the case's grid under its wind and the oracle of it, both reset and then scattered over the grid."""
    g, plane = _case(name)
    vec = gua.VecGridUniverse(N, template=_spec(g), seed=seed)
    o = O.WindOracle(_grid(g), seed, N, wind=plane if wind else None, gust_q16=gust_q16, q0=q0)
    if wind:
        vec.engine.set_wind(plane, gust_q16)
    if q0 is not None:
        vec._ensure_q(q0)
    assert np.array_equal(vec.reset(), o.reset())
    vec.set_state(pos=_scatter(g, N))
    o.state.pos[:] = _scatter(g, N)
    return vec, o


def test_set_wind_and_wind_round_trip():
    g, plane = _case('maze11')
    vec = gua.VecGridUniverse(8, template=_spec(g))
    try:
        assert vec.wind() is None and vec.engine.get_wind() is None
        vec.set_wind((plane.reshape(11, 11) >> 2) & 3, plane.reshape(11, 11) & 3, gust=2 / 3)
        w = vec.wind()
        assert np.array_equal(w['strength'], (plane.reshape(11, 11) >> 2) & 3) and np.array_equal(w['direction'], plane.reshape(11, 11) & 3)
        assert w['gust'] == O.GUST_THIRDS / 65536.0 and vec.engine.get_wind()[1] == O.GUST_THIRDS
        assert np.array_equal(vec.engine.get_wind()[0], plane)
        eng = vec.engine
        for bad, gust in ((plane | 16, 0), (plane | 128, 0), (plane, 65537)):
            with pytest.raises(gua.GuError) as err:
                eng.set_wind(bad, gust)
            assert err.value.code == -1
        assert np.array_equal(eng.get_wind()[0], plane)  # a refused plane changes nothing
        vec.set_wind(None)
        assert vec.wind() is None
    finally:
        vec.close()


@pytest.mark.parametrize('gust', GUSTS)
@pytest.mark.parametrize('auto', [True, False])
@pytest.mark.parametrize('case', CASES)
def test_step_and_step_device_equal_the_oracle(case, auto, gust):
    N, T = 200, 32
    vec, o = _pair(case, N, 4, gust)
    try:
        vec.auto_reset = auto
        acts = np.random.RandomState(11).randint(-4, 4, (T, N)).astype(np.int32)
        for i in range(T):
            a = acts[i].copy()
            if i == 10:
                a[17] = 7  # rejected: env 17 does not step, reset or draw; the others do
                with pytest.raises(gua.GuError) as err:
                    vec.step(a)
                assert err.value.code == -1
                o.step(a, auto)
                _same_state(vec, o)
                continue
            obs, rew, don, _ = vec.step(a)
            w_obs, w_rew, w_don, rejected = o.step(a, auto)
            assert not rejected.any()
            assert np.array_equal(obs, w_obs) and np.array_equal(rew, w_rew) and np.array_equal(don, w_don != 0), i
        _same_state(vec, o)
        # the same rows from the device-resident stream
        vec.seed(4)
        o2 = O.WindOracle(o.grid, 4, N, wind=o.wind, gust_q16=gust)
        assert np.array_equal(vec.reset(), o2.reset())
        vec.engine.upload_actions(acts)
        for i in range(T):
            vec.engine.step_device(i, auto)
            obs, rew, don = vec.engine.read_outputs()
            w_obs, w_rew, w_don, _ = o2.step(acts[i], auto)
            assert np.array_equal(obs, w_obs) and np.array_equal(rew, w_rew) and np.array_equal(don != 0, w_don != 0), i
        _same_state(vec, o2)
    finally:
        vec.close()


@pytest.mark.parametrize('gust', GUSTS)
@pytest.mark.parametrize('auto', [True, False])
@pytest.mark.parametrize('policy', ['uniform', 'stream', 'greedy', 'sample'])
@pytest.mark.parametrize('case', CASES)
def test_rollout_equals_the_oracle(case, policy, auto, gust):
    N, T = 200, 100  # three full waves and a partial one
    vec, o = _pair(case, N, 6, gust)
    try:
        S = o.grid.S
        pi = _policy_table(S) if policy in ('greedy', 'sample') else None
        acts = np.random.RandomState(2).randint(0, 4, (T, N)).astype(np.int32) if policy == 'stream' else None
        if pi is not None:
            vec.engine.vi_set(np.zeros(S), pi)
        want = o.rollout(T, policy, auto, actions=acts, pi=pi)
        if case != 'book' and policy == 'uniform' and auto:
            assert (want['reward'] == -10).any()  # agents are blown into lava
        # two launches of 50 ...
        halves = [vec.rollout(50, policy, actions=None if acts is None else acts[k * 50:(k + 1) * 50], auto_reset=auto, stats=True) for k in range(2)]
        for k in ('obs', 'reward', 'done'):
            assert np.array_equal(np.concatenate([h[k] for h in halves]), want[k]), k
        assert np.array_equal(halves[0]['ret'] + halves[1]['ret'], want['ret'])
        assert np.array_equal(halves[0]['episodes'] + halves[1]['episodes'], want['episodes'])
        _same_state(vec, o)
        # ... equal one of 100
        vec.seed(6)
        vec.reset()
        vec.set_state(pos=_scatter(_case(case)[0], N))
        _same(vec.rollout(T, policy, actions=acts, auto_reset=auto, stats=True), want)
        _same_state(vec, o)
        with pytest.raises(gua.GuError) as err:  # packed rows are refused under wind
            vec.engine.rollout(10, 'uniform', auto, 'packed')
        assert err.value.code == -6 and 'wind' in str(err.value)
    finally:
        vec.close()


@pytest.mark.parametrize('gust', GUSTS)
@pytest.mark.parametrize('N', [1, 63, 256])
@pytest.mark.parametrize('method', ['q_learning', 'sarsa'])
@pytest.mark.parametrize('case', CASES)
def test_td_run_tables_rows_and_stats_equal_the_oracle(case, method, N, gust):
    T = 300
    vec, o = _pair(case, N, 3, gust, q0=0.0 if N != 63 else 0.5)
    try:
        got = vec.td_run(T, method, alpha=0.25, discount_factor=0.9, epsilon=0.2, trajectory=True, stats=True)
        _same(got, o.td_run(T, METHODS[method], 0.25, 0.9, _eps(0.2)))
        assert vec.q_table().tobytes() == o.q.tobytes()
        _same_state(vec, o)
    finally:
        vec.close()


@pytest.mark.parametrize('gust', GUSTS)
def test_sarsa_split_in_two_carries_its_action_and_set_wind_drops_it(gust):
    vec, o = _pair('maze11', 130, 8, gust, q0=0.0)
    try:
        plane = o.wind
        for T in (150, 150):  # the second launch starts with the first one's a'
            got = vec.td_run(T, 'sarsa', alpha=0.5, discount_factor=0.95, epsilon=0.3, trajectory=True, stats=True)
            _same(got, o.td_run(T, O.SARSA, 0.5, 0.95, _eps(0.3)))
        assert o.carry_valid and (o.carry >= 0).any()
        vec.engine.set_wind(plane, gust)  # the same wind again: tables, state and counts stay, the carry goes
        o.set_wind(plane, gust)
        got = vec.td_run(100, 'sarsa', alpha=0.5, discount_factor=0.95, epsilon=0.3, trajectory=True, stats=True)
        _same(got, o.td_run(100, O.SARSA, 0.5, 0.95, _eps(0.3)))
        assert vec.q_table().tobytes() == o.q.tobytes()
        _same_state(vec, o)
    finally:
        vec.close()


@pytest.mark.parametrize('method', ['q_learning', 'sarsa'])
def test_the_gust_epoch_changes_inside_a_launch(method):
    N = 96
    vec, o = _pair('book', N, 12, O.GUST_THIRDS, q0=0.0)
    try:
        tc = counts_near_2_32(vec, o, N, 2 ** 32 - 20)
        got = vec.td_run(60, method, alpha=0.2, discount_factor=0.9, epsilon=0.5, trajectory=True, stats=True)
        _same(got, o.td_run(60, METHODS[method], 0.2, 0.9, _eps(0.5)))
        assert vec.q_table().tobytes() == o.q.tobytes()
        # ... and inside a rollout (streams 0, 2 and 9 re-keyed in the same step)
        vec.set_state(tcount=tc)
        o.set_state(tcount=tc)
        pi = _policy_table(o.grid.S)
        vec.engine.vi_set(np.zeros(o.grid.S), pi)
        for policy in ('uniform', 'sample'):
            _same(vec.rollout(40, policy, auto_reset=True, stats=True), o.rollout(40, policy, True, pi=pi))
        _same_state(vec, o)
    finally:
        vec.close()


@pytest.mark.parametrize('case', ['maze11', 'open150'])
def test_wind_of_strength_zero_gives_the_bytes_of_the_calm_engine(case):
    g, plane = _case(case)
    N, seed = 200, 9
    calm_plane = plane & 3  # directions without strength
    grid = _grid(g)
    vec = gua.VecGridUniverse(N, template=_spec(g), seed=seed)
    ref = gua.VecGridUniverse(N, template=_spec(g), seed=seed)  # the calm engine
    try:
        vec.engine.set_wind(calm_plane, O.GUST_THIRDS)
        st = C.State(N)
        first = C.reset(grid, seed, st)
        assert np.array_equal(vec.reset(), first) and np.array_equal(ref.reset(), first)
        acts = np.random.RandomState(3).randint(0, 4, (8, N)).astype(np.int32)
        for i in range(8):
            a, b = vec.step(acts[i]), ref.step(acts[i])
            assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3]))
        C.rollout(grid, seed, st, 8, False, actions=acts)
        for auto in (True, False):
            got, calm = vec.rollout(100, 'uniform', auto_reset=auto, stats=True), ref.rollout(100, 'uniform', auto_reset=auto, stats=True)
            _same(got, calm)
            _same(got, C.rollout(grid, seed, st, 100, auto, stats=True))
        for method in ('q_learning', 'sarsa'):
            kw = dict(alpha=0.3, discount_factor=0.9, epsilon=0.2, trajectory=True, stats=True)
            _same(vec.td_run(120, method, **kw), ref.td_run(120, method, **kw))
            assert vec.q_table().tobytes() == ref.q_table().tobytes()
        a, b = vec.get_state(), ref.get_state()
        assert all(np.array_equal(a[k], b[k]) for k in ('pos', 'done', 'episode', 'tcount'))
    finally:
        vec.close()
        ref.close()


def test_a_calmed_engine_takes_the_original_kernels_again(gu_option):
    """Under wind a launch keeps no store schedule; after set_wind(None) the same launch is the calm engine's, and the store-pacing
    report counts it."""
    gu_option('rollout_pace', None)
    meta, _ = G.load_traj('c3_maze32')
    N, T, seed = 65536, 300, 9  # 236 MB of rows per launch: paced on the calm engine
    g = dict(W=meta['W'], H=meta['H'], starts=meta['starts'], goals=meta['goals'], lava=meta['lava'], walls=meta['walls'], reward=meta['reward'])
    vec = gua.VecGridUniverse(N, template=_spec(g), seed=seed, auto_reset=True)
    try:
        eng = vec.engine
        eng.set_wind(wind_plane(g['W'], g['H'], np.ones(g['W'], int)), 0)
        vec.reset()
        eng.reserve_trajectory(T)
        eng.rollout(T, 'uniform', True, True)
        assert eng.rollout_pacing() is None and eng.rollout_pacing_totals()['kinds_paced'] == 0
        vec.set_wind(None)
        vec.seed(seed)
        vec.reset()
        eng.rollout(T, 'uniform', True, True, stats=True)
        info = eng.rollout_pacing()
        assert info is not None and info['evaluated'] == 1 and eng.rollout_pacing_totals()['kinds_paced'] == 1
        grid, st = C.Grid.from_lists(**meta), C.State(2048)
        C.reset(grid, seed, st)
        want = C.rollout(grid, seed, st, T, True)
        tr = eng.read_trajectory(0, T)
        assert all(np.array_equal(tr[k][:, :2048], want[k]) for k in ('obs', 'reward', 'done'))
    finally:
        vec.close()


def _greedy_path(grid, wind, q, start, limit):
    """Moves of the greedy policy of q from `start` to the goal under calm gusts (None: not within `limit`)."""
    s, one = int(start), lambda x: np.array([x], np.int32)  # noqa: E731
    for n in range(1, limit + 1):
        c = int(wind[s])
        s = int(O.push(grid, one(s), one(int(np.argmax(q[s]))), one((c >> 2) & 3), one(c & 3))[0][0])
        if grid.goal[s]:
            return n
    return None


def test_q_learning_end_to_end_on_the_books_grid():
    """64 learners, 8000 steps, alpha 0.5, epsilon 0.1, gamma 0.99, calm gusts: the tables equal the oracle's, at least half of the
    greedy paths reach the goal within 20 moves and none in fewer than the 10 of the shortest path.  (A plain numpy Q-learner with
    these settings reached it in 10 to 16 moves in 32 of 32 runs.)"""
    L, T, seed = 64, 8000, 1
    env = gua.GridUniverseEnv(grid_shape=(O.BOOK_W, O.BOOK_H), initial_state=O.BOOK['starts'][0], goal_states=O.BOOK['goals'])
    q = q_learning(env, T, alpha=0.5, discount_factor=0.99, epsilon=0.1, num_learners=L, seed=seed, wind=O.BOOK_STRENGTH)
    grid, plane = _grid(O.BOOK), wind_plane(O.BOOK_W, O.BOOK_H, O.BOOK_STRENGTH)
    o = O.WindOracle(grid, seed, L, wind=plane, q0=0.0)
    o.reset()
    o.td_run(T, O.Q_LEARNING, 0.5, 0.99, _eps(0.1))
    assert q.tobytes() == o.q.tobytes()
    lengths = [_greedy_path(grid, plane, q[e], O.BOOK['starts'][0], 20) for e in range(L)]
    reached = [n for n in lengths if n is not None]
    assert len(reached) * 2 >= L, lengths
    assert min(reached) >= 10, lengths
