"""Wind on the device (gu_set_wind; csrc/gu_wind.hip and the windy gu_td_kernel instantiations) against the CPU restatement
tests/_wind_oracle.py: step, rollout and td_run compared byte for byte, the calm plane against the calm engine, and every call
that has no windy form refused while wind is set."""
import functools

import numpy as np
import pytest

import griduniverse_amd as gua
from griduniverse_amd import _lib
from griduniverse_amd.algorithms.exploration import ucb_tables
from griduniverse_amd.algorithms.temporal_difference import q_learning
from griduniverse_amd.grid import wind_plane
from oracle import c_oracle as C

from . import _golden as G
from . import _td_oracle as TD
from . import _wind_oracle as O
from ._tabular_cases import GRIDS, _eps, _grid, _same, _spec, counts_near_2_32

pytestmark = pytest.mark.gpu

GUSTS = [0, O.GUST_THIRDS]
METHODS = {'q_learning': O.Q_LEARNING, 'sarsa': O.SARSA}


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


def _scatter(g, N):
    """N cells of the grid that are neither wall nor terminal: where the tests put the envs, so that a batch with one start cell
    (and a deterministic policy) still walks the whole grid."""
    taken = set(g['walls']) | set(g['goals']) | set(g['lava'])
    free = np.array([s for s in range(g['W'] * g['H']) if s not in taken], np.int32)
    return free[np.random.RandomState(N).randint(0, len(free), N)]


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


def _same_state(vec, o):
    st = vec.get_state()
    assert np.array_equal(st['pos'], o.state.pos) and np.array_equal(st['done'] != 0, o.state.done != 0)
    assert np.array_equal(st['episode'], o.state.episode) and np.array_equal(st['tcount'], o.state.tcount)


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


def _policy_table(S):
    pi = np.random.RandomState(1).dirichlet(np.ones(4), S)
    pi[::7] = np.eye(4)[np.arange(len(pi[::7])) % 4]  # one-hot rows: thresholds that no word reaches
    return pi


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


def test_calls_without_a_windy_form_are_refused_while_wind_is_set():
    g, plane = _case('maze11')
    N, S = 64, 121
    vec = gua.VecGridUniverse(N, template=_spec(g), seed=1)
    try:
        eng = vec.engine
        vec.reset()
        eng.upload_actions(np.zeros((4, N), np.int32))
        eng.vi_set(np.zeros(S), np.full((S, 4), 0.25))
        eng.reserve_trajectory(8)
        vec.set_exploration(*ucb_tables(1.0, 16))
        vec.set_features(np.arange(S, dtype=np.int32)[:, None])
        cdf = np.tile(np.array([0.25, 0.5, 0.75, 1.0]), (S, 1))
        u = np.random.RandomState(0).rand(256)
        start = g['starts'][0]
        calls = {
            'gu_step_graph': lambda: eng.step_graph(0, 4),
            'gu_dyna_run': lambda: vec.dyna_run(5, planning_steps=2),
            'gu_search_run': lambda: vec.search_run(3, simulations=1, depth=2),
            'gu_explore_run': lambda: vec.explore_run(5),
            'gu_mcts_run': lambda: vec.tree_search_run(3, simulations=2, tree_depth=2, depth=2),
            'gu_nstep_run': lambda: vec.nstep_run(5),
            'gu_lambda_run': lambda: vec.lambda_run(5),
            'gu_ac_run': lambda: vec.actor_critic_run(5),
            'gu_reinforce_run': lambda: vec.reinforce_run(5),
            'gu_is_run': lambda: vec.off_policy_mc_run(5),
            'gu_fa_run': lambda: vec.fa_run(5),
            'gu_look_step_ahead': lambda: eng.look_step_ahead([start], [1]),
            'gu_vi_sweep': lambda: eng.vi_sweep(0.9, 1),
            'gu_vi_run': lambda: eng.vi_run(0.9, 1e-3, 3),
            'gu_vi_eval_run': lambda: eng.vi_eval_run(0.9, 1e-3, 3),
            'gu_vi_greedy': lambda: eng.vi_greedy(0.9),
            'gu_vi_sweep_step': lambda: eng.vi_sweep_step(0.9),
            'gu_vi_sweep_step_run': lambda: eng.vi_sweep_step_run(0.9, 2),
            'gu_mc_walk_lengths': lambda: eng.mc_walk_lengths(u, 8, [start], 16, cdf),
            'gu_mc_walk_episodes': lambda: eng.mc_walk_episodes(u, cdf, np.zeros(N, np.int64), np.full(N, start, np.int32), 16, 8),
            'gu_shortest_paths': lambda: eng.shortest_paths(),
        }
        # the tables the learners need exist before the wind is set (the inits are not refused either way)
        vec._ensure_q()
        vec._ensure_model()
        vec._ensure_counts()
        vec._ensure_tree()
        vec._ensure_ac()
        vec._ensure_is()
        eng.set_wind(plane, O.GUST_THIRDS)
        for name, call in calls.items():
            with pytest.raises(gua.GuError) as err:
                call()
            assert err.value.code == -6 and 'wind' in str(err.value), name
        with pytest.raises(gua.GuError) as err:  # the trail refuses while wind is set
            eng.trail_enable(16)
        assert err.value.code == -6 and 'wind' in str(err.value)
        # what reads rows or state only is unaffected
        vec.rollout(8, 'uniform', auto_reset=True)
        eng.mc_evaluate(8, np.full(N, start, np.int32), 0.9 ** np.arange(8), np.ones(8, bool))
        eng.vi_get()
        vec.sense(radius=1)
        vec.get_state()
        vec.set_wind(None)
        for name, call in calls.items():  # the same calls succeed once the wind is gone
            call()
        # wind refuses while the trail is on
        eng.trail_enable(16)
        with pytest.raises(gua.GuError) as err:
            eng.set_wind(plane, 0)
        assert err.value.code == -6 and 'trail' in str(err.value)
        eng.trail_enable(0)
        eng.set_wind(plane, 0)
        assert eng.get_wind() is not None
        eng.set_grid(_spec(g))  # a new grid drops the wind
        assert eng.get_wind() is None
        eng.look_step_ahead([start], [1])
    finally:
        vec.close()
    grids = [_spec(g), _spec(g)]
    multi = gua.VecGridUniverse(N, templates=grids, seed=1)
    try:
        with pytest.raises(gua.GuError) as err:  # wind is a property of a single-grid engine
            multi.engine.set_wind(plane, 0)
        assert err.value.code == -6 and 'wind' in str(err.value)
        multi.engine.set_grid(_spec(g))
        multi.engine.set_wind(plane, 0)
        multi.engine.set_grids(grids)  # ... and several grids drop it
        assert multi.engine.get_wind() is None
        multi.engine.set_grid(_spec(g))
        multi.engine.set_wind(plane, 0)
        multi.engine.generate_mazes(2, 11, 11, 5)  # ... as device mazes do
        assert multi.engine.get_wind() is None
    finally:
        multi.close()


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
