"""How the tests drive each batched learner: one adapter per entry point (its CPU restatement of tests/_*_oracle.py, its stores on
the device and in the restatement, one launch of each), the registry LEARNERS of all of them, and the harnesses that compare a learner
with its restatement: on an engine whose first env has any global id (_against_restatement; on a shared grid beyond LDS,
_shared_grid_beyond_lds) and on per-env stores across 2^32 bytes.  Used by test_gpu_learners_at_scale.py and test_gpu_env_ids.py
(which say what the cases are for), test_gpu_double.py, test_learner_harness_host.py and test_env_ids_host.py."""
import numpy as np
import pytest

import griduniverse_amd as gua
from griduniverse_amd.algorithms import exploration as X
from griduniverse_amd.algorithms.function_approximation import one_hot

from . import _ac_oracle as AO
from . import _double_oracle as DB
from . import _dyna_oracle as DO
from . import _explore_oracle as EO
from . import _fa_oracle as FO
from . import _is_oracle as IO
from . import _lambda_oracle as LO
from . import _mcts_oracle as MO
from . import _nstep_oracle as NO
from . import _reinforce_oracle as RO
from . import _search_oracle as SO
from . import _sweep_oracle as SW
from . import _td_oracle as TD
from ._tabular_cases import _eps, _grid, _same, _spec, spread_grid

ERR_INVALID, ERR_NOMEM = -1, -3
METHODS = {'q_learning': TD.Q_LEARNING, 'sarsa': TD.SARSA}
Q0, H0, V0, W0 = 0.5, 0.5, -0.25, 0.5  # the fills: non-zero wherever the learner offers one
ALPHA, GAMMA, EPS = 0.25, 0.9, 0.3


def big182():
    return spread_grid(182, 182)


def sweep128():
    return spread_grid(128, 128)


def no_way_out():
    """5 x 5 with its only goal walled in (cell 23 behind 18, 22 and 24): no episode ends, so an episode buffer fills to L."""
    return dict(W=5, H=5, starts=[0], goals=[23], lava=[], walls=[18, 22, 24])


# ---------------------------------------------------------------------------------------------------------------- the learners
class Learner(object):
    """One learner entry point: its restatement, its stores on the device and in the restatement, and one launch of each."""
    T = (40, 25)   # Part A: two launches, the second continues the first
    install = None  # (vec, tables, env0): install `tables` (name -> array, as learned() names them) for envs env0 .. on the device
    restate_install = None  # (o, tables, env0): the same in the restatement, env0 counted from its first env

    def oracle(self, grid, seed, n, env_id0):
        raise NotImplementedError

    def prepare(self, vec):
        """The learner's stores on the device, at their fills."""
        vec._ensure_q(Q0)

    def device(self, vec, T, **kw):
        raise NotImplementedError

    def restate(self, o, T):
        raise NotImplementedError

    def got(self, vec, env0, n):
        """Every store the learner owns, of envs env0 .. env0+n-1: name -> array."""
        return dict(q=vec.q_table(env0, n))

    def want(self, o):
        return dict(q=o.q)

    def learned(self, o):
        """(name, table, fill) of the tables a launch must have changed."""
        return [('q', o.q, Q0)]


def _flat(prefix, d):
    return dict((prefix + '.' + k, v) for k, v in d.items())


class Td(Learner):
    def __init__(self, method):
        self.method = method

    def oracle(self, grid, seed, n, env_id0):
        return TD.TdOracle(grid, seed, n, env_id0, Q0)

    def device(self, vec, T, **kw):
        return vec.td_run(T, self.method, alpha=ALPHA, discount_factor=GAMMA, epsilon=EPS, **kw)

    def restate(self, o, T):
        return o.run(T, METHODS[self.method], ALPHA, GAMMA, _eps(EPS))

    @staticmethod
    def install(vec, tables, env0):
        vec.set_q_table(tables['q'], env0=env0)

    @staticmethod
    def restate_install(o, tables, env0):
        o.set_q(tables['q'], env0)


class Nstep(Td):
    T, n = (37, 23), 4  # not multiples of n: the window crosses the launch boundary

    def oracle(self, grid, seed, n, env_id0):
        return NO.NstepOracle(grid, seed, n, env_id0, Q0)

    def device(self, vec, T, **kw):
        return vec.nstep_run(T, self.n, self.method, alpha=ALPHA, discount_factor=GAMMA, epsilon=EPS, **kw)

    def restate(self, o, T):
        return o.nstep(T, METHODS[self.method], self.n, ALPHA, GAMMA, _eps(EPS))

    def got(self, vec, env0, n):
        return dict(_flat('window', vec.nstep_window(env0, n)), q=vec.q_table(env0, n))

    def want(self, o):
        return dict(_flat('window', o.window()), q=o.q)


class Lambda(Td):
    T, K, lam = (37, 23), 8, 0.9

    def oracle(self, grid, seed, n, env_id0):
        return LO.LambdaOracle(grid, seed, n, env_id0, Q0)

    def device(self, vec, T, **kw):
        return vec.lambda_run(T, self.lam, self.K, self.method, alpha=ALPHA, discount_factor=GAMMA, epsilon=EPS, **kw)

    def restate(self, o, T):
        return o.lam(T, METHODS[self.method], self.K, self.lam, ALPHA, GAMMA, _eps(EPS))

    def got(self, vec, env0, n):
        return dict(window=vec.lambda_window(env0, n), q=vec.q_table(env0, n))

    def want(self, o):
        return dict(window=o.window(), q=o.q)


class Dyna(Learner):
    T, P = (30, 20), 5

    def oracle(self, grid, seed, n, env_id0):
        return DO.DynaOracle(grid, seed, n, env_id0, Q0)

    def prepare(self, vec):
        vec._ensure_q(Q0)
        vec._ensure_model()

    def device(self, vec, T, **kw):
        return vec.dyna_run(T, self.P, alpha=ALPHA, discount_factor=GAMMA, epsilon=EPS, **kw)

    def restate(self, o, T):
        return o.dyna(T, self.P, ALPHA, GAMMA, _eps(EPS))

    def got(self, vec, env0, n):
        return dict(_flat('model', vec.model(env0, n)), q=vec.q_table(env0, n))

    def want(self, o):
        return dict(_flat('model', o.model()), q=o.q)

    def learned(self, o):
        return [('q', o.q, Q0), ('model.next', o.next, -1), ('model.list', o.list, -1)]


class Sweep(Dyna):
    T, P, theta = (12, 8), 4, 1e-4

    def oracle(self, grid, seed, n, env_id0):
        return SW.SweepOracle(grid, seed, n, env_id0, Q0)

    def prepare(self, vec):
        vec._ensure_q(Q0)
        vec._ensure_queue()

    def device(self, vec, T, **kw):
        return vec.sweep_run(T, self.P, theta=self.theta, alpha=ALPHA, discount_factor=GAMMA, epsilon=EPS, **kw)

    def restate(self, o, T):
        return o.sweep(T, self.P, self.theta, ALPHA, GAMMA, _eps(EPS))

    def got(self, vec, env0, n):
        out = dict(_flat('model', vec.model(env0, n)), q=vec.q_table(env0, n))
        out.update(_flat('queue', vec.priority_queue(env0, n)))
        self.raw = vec.engine.diag_sweep_heap(env0, n)  # (checked for its shape by _heap_is_a_heap_of: the restatement keeps no heap)
        return out

    def want(self, o):
        return dict(_flat('model', o.model()), q=o.q, **_flat('queue', o.queue()))


class Explore(Learner):
    def __init__(self, rule):
        self.rule = rule
        self.tables = X.ucb_tables(1.0, 64) if rule == 'ucb' else X.thompson_tables(3.0, 64)

    def oracle(self, grid, seed, n, env_id0):
        o = EO.ExploreOracle(grid, seed, n, env_id0, Q0)
        o.set_tables(*self.tables)
        return o

    def prepare(self, vec):
        vec._ensure_q(Q0)
        vec.set_exploration(*self.tables)
        vec._ensure_counts()

    def device(self, vec, T, **kw):
        return vec.explore_run(T, self.rule, alpha=ALPHA, discount_factor=GAMMA, epsilon=0.2, **kw)

    def restate(self, o, T):
        return o.explore(T, {'ucb': EO.UCB, 'thompson': EO.THOMPSON}[self.rule], ALPHA, GAMMA, _eps(0.2))

    def got(self, vec, env0, n):
        return dict(q=vec.q_table(env0, n), counts=vec.visit_counts(env0, n))

    def want(self, o):
        return dict(q=o.q, counts=o.counts)

    def learned(self, o):
        return [('q', o.q, Q0), ('counts', o.counts, 0)]

    @staticmethod
    def install(vec, tables, env0):
        vec.set_q_table(tables['q'], env0=env0)
        vec.set_visit_counts(tables['counts'], env0=env0)

    @staticmethod
    def restate_install(o, tables, env0):
        o.set_q(tables['q'], env0)
        o.set_counts(tables['counts'], env0)


class Search(Learner):
    T, M, D, eps_sim = (30, 15), 2, 5, 65536

    def oracle(self, grid, seed, n, env_id0):
        return SO.SearchOracle(grid, seed, n, env_id0, Q0)

    def device(self, vec, T, **kw):
        return vec.search_run(T, self.M, self.D, alpha=ALPHA, discount_factor=GAMMA, epsilon=EPS, rollout_epsilon=self.eps_sim / 65536.0, **kw)

    def restate(self, o, T):
        return o.search(T, self.M, self.D, ALPHA, GAMMA, _eps(EPS), self.eps_sim)

    def got(self, vec, env0, n):
        return dict(_flat('search', vec.search_scores(env0, n)), q=vec.q_table(env0, n))

    def want(self, o):
        return {'search.score': o.score, 'search.sim_steps': o.sim_steps, 'q': o.q}


class Mcts(Learner):
    T, M, H, D, eps_sim = (20, 10), 8, 4, 4, 65536

    def __init__(self, max_sims=None):
        self.max_sims = max_sims  # the pool asked for ahead of the first launch (None: the first launch makes one of M)

    def oracle(self, grid, seed, n, env_id0):
        o = MO.MctsOracle(grid, seed, n, env_id0, Q0)
        if self.max_sims:
            o.pool(self.max_sims)
        return o

    def prepare(self, vec):
        vec._ensure_q(Q0)
        if self.max_sims:
            vec.engine.mcts_init(self.max_sims)

    def device(self, vec, T, **kw):
        return vec.tree_search_run(T, self.M, self.H, self.D, alpha=ALPHA, discount_factor=GAMMA, epsilon=EPS,
                                   rollout_epsilon=self.eps_sim / 65536.0, **kw)

    def restate(self, o, T):
        return o.tree_search(T, self.M, self.H, self.D, ALPHA, GAMMA, _eps(EPS), self.eps_sim)

    def got(self, vec, env0, n):
        return dict(_flat('root', vec.tree_search_roots(env0, n)), q=vec.q_table(env0, n), **_flat('tree', vec.tree_search_tree(env0, n)))

    def want(self, o):
        root = dict(w=o.root_w, visits=o.root_visits, nodes=o.count, sim_steps=o.sim_steps)
        tree = dict(state=o.t_state, parent=o.t_parent, child=o.t_child, visits=o.t_visits, w=o.t_w, count=o.count)
        return dict(_flat('root', root), q=o.q, **_flat('tree', tree))

    def learned(self, o):
        return [('q', o.q, Q0), ('tree.state', o.t_state, -1)]


class Is(Learner):
    L, w_cap, eps = 16, 2.0 ** 64, EPS

    def oracle(self, grid, seed, n, env_id0):
        return IO.IsOracle(grid, seed, n, env_id0, Q0)

    def prepare(self, vec):
        vec._ensure_q(Q0)
        vec._ensure_is()

    def device(self, vec, T, **kw):
        return vec.off_policy_mc_run(T, self.L, discount_factor=GAMMA, epsilon=self.eps, w_cap=self.w_cap, **kw)

    def restate(self, o, T):
        return o.is_run(T, self.L, GAMMA, _eps(self.eps), self.w_cap)

    def got(self, vec, env0, n):
        return dict(_flat('buffer', vec.off_policy_episode_buffer(env0, n)), q=vec.q_table(env0, n), c=vec.importance_weights(env0, n))

    def want(self, o):
        return dict(_flat('buffer', dict(sa=o.buf_sa, reward=o.buf_r, cls=o.buf_c, count=o.buf_cnt)), q=o.q, c=o.c)

    def learned(self, o):
        return [('q', o.q, Q0), ('c', o.c, 0.0)]

    @staticmethod
    def install(vec, tables, env0):
        vec.set_q_table(tables['q'], env0=env0)
        vec.set_importance_weights(tables['c'], env0=env0)

    @staticmethod
    def restate_install(o, tables, env0):
        o.set_q(tables['q'], env0)
        o.set_c(tables['c'], env0)


class Ac(Learner):
    aa, ab = 0.2, 0.3

    def oracle(self, grid, seed, n, env_id0):
        return AO.AcOracle(grid, seed, n, env_id0, h0=H0, v0=V0)

    def prepare(self, vec):
        vec._ensure_ac(H0, V0)

    def device(self, vec, T, **kw):
        return vec.actor_critic_run(T, actor_lr=self.aa, critic_lr=self.ab, discount_factor=GAMMA, **kw)

    def restate(self, o, T):
        return o.ac(T, self.aa, self.ab, GAMMA)

    def got(self, vec, env0, n):
        return dict(h=vec.preferences(env0, n), v=vec.state_values(env0, n))

    def want(self, o):
        return dict(h=o.h, v=o.v)

    def learned(self, o):
        return [('h', o.h, H0), ('v', o.v, V0)]

    @staticmethod
    def install(vec, tables, env0):
        vec.set_actor_critic(tables['h'], tables['v'], env0=env0)

    @staticmethod
    def restate_install(o, tables, env0):
        o.set_ac(tables['h'], tables['v'], env0)


class Reinforce(Ac):
    L, aa, ab = 16, 0.05, 0.3
    install = restate_install = None

    def oracle(self, grid, seed, n, env_id0):
        return RO.ReinforceOracle(grid, seed, n, env_id0, h0=H0, v0=V0)

    def device(self, vec, T, **kw):
        return vec.reinforce_run(T, self.L, actor_lr=self.aa, baseline_lr=self.ab, discount_factor=GAMMA, **kw)

    def restate(self, o, T):
        return o.reinforce(T, self.L, self.aa, self.ab, GAMMA)

    def got(self, vec, env0, n):
        return dict(_flat('buffer', vec.episode_buffer(env0, n)), h=vec.preferences(env0, n), v=vec.state_values(env0, n))

    def want(self, o):
        return dict(_flat('buffer', dict(sa=o.buf_sa, reward=o.buf_r, count=o.buf_cnt)), h=o.h, v=o.v)


class Fa(Learner):
    """One-hot features: F = S, the weights are a table [N][S][4] behind gu_fa.hip's own index arithmetic."""

    def __init__(self, method):
        self.method = method

    def oracle(self, grid, seed, n, env_id0):
        phi, F = one_hot(grid.S)
        return FO.FaOracle(grid, seed, n, phi, F, W0, env_id0)

    def prepare(self, vec):
        phi, F = one_hot(vec.spec.S)
        vec.set_features(phi, F, W0)

    def device(self, vec, T, **kw):
        return vec.fa_run(T, self.method, alpha=ALPHA, discount_factor=GAMMA, epsilon=EPS, **kw)

    def restate(self, o, T):
        return o.run(T, METHODS[self.method], ALPHA, GAMMA, _eps(EPS))

    def got(self, vec, env0, n):
        return dict(w=vec.weights(env0, n), q=vec.fa_q_table(env0, n))

    def want(self, o):
        return dict(w=o.w, q=o.q_tables())

    def learned(self, o):
        return [('w', o.w, W0)]

    @staticmethod
    def install(vec, tables, env0):
        vec.set_weights(tables['w'], env0=env0)

    @staticmethod
    def restate_install(o, tables, env0):
        o.set_w(tables['w'], env0)


class ExpectedSarsa(Learner):
    def oracle(self, grid, seed, n, env_id0):
        return DB.EsarsaOracle(grid, seed, n, env_id0, 0.5)

    def device(self, vec, T, **kw):
        return vec.expected_sarsa_run(T, alpha=0.25, discount_factor=0.9, epsilon=0.3, **kw)

    def restate(self, o, T):
        return o.esarsa(T, 0.25, 0.9, _eps(0.3))


class DoubleQ(Learner):
    def oracle(self, grid, seed, n, env_id0):
        return DB.DoubleOracle(grid, seed, n, env_id0, 0.5)

    def prepare(self, vec):
        vec._ensure_pairs(0.5)

    def device(self, vec, T, **kw):
        return vec.double_q_run(T, alpha=0.25, discount_factor=0.9, epsilon=0.3, **kw)

    def restate(self, o, T):
        return o.run(T, 0.25, 0.9, _eps(0.3))

    def got(self, vec, env0, n):
        return dict(q=vec.double_q_tables(env0, n))

    @staticmethod
    def install(vec, tables, env0):
        vec.set_double_q_tables(tables['q'], env0)

    @staticmethod
    def restate_install(o, tables, env0):
        if len(tables['q']):
            o.set_q(tables['q'], env0)


# every learner entry point of the engine has an adapter here (test_learner_harness_host.py holds the two sets equal)
LEARNERS = {
    'td-q_learning': Td('q_learning'), 'td-sarsa': Td('sarsa'),
    'nstep-q_learning': Nstep('q_learning'), 'nstep-sarsa': Nstep('sarsa'),
    'lambda-q_learning': Lambda('q_learning'), 'lambda-sarsa': Lambda('sarsa'),
    'dyna': Dyna(), 'explore-ucb': Explore('ucb'), 'explore-thompson': Explore('thompson'),
    'search': Search(), 'mcts': Mcts(), 'is': Is(), 'ac': Ac(), 'reinforce': Reinforce(),
    'fa-q_learning': Fa('q_learning'), 'fa-sarsa': Fa('sarsa'),
    'sweep': Sweep(), 'expected_sarsa': ExpectedSarsa(), 'double_q': DoubleQ(),
}


# ---------------------------------------------------------------------------------------------------------------- comparisons
def _same_stores(got, want, where):
    assert sorted(got) == sorted(want), where
    for k in sorted(got):
        g, w = got[k], np.asarray(want[k])
        assert g.shape == w.shape and g.tobytes() == w.astype(g.dtype, copy=False).tobytes(), (where, k)


def _same_state(st, o, env0, where):
    for k in ('pos', 'done', 'episode', 'tcount'):
        assert np.array_equal(st[k][env0:env0 + o.n], getattr(o.state, k)), (where, k)


def _open(N, g, seed, learner, env_id0=0):
    """N envs on grid g, the shard that starts at global env id env_id0, with the learner's stores at their fills; the test skips
    where the library finds no room for them."""
    vec = gua.VecGridUniverse(N, template=_spec(g), seed=seed, env_id0=env_id0)
    try:
        learner.prepare(vec)
    except gua.GuError as err:
        vec.close()
        if err.code == ERR_NOMEM:
            pytest.skip(str(err))
        raise
    except BaseException:
        vec.close()
        raise
    return vec


def _launch(vec, learner, T, **kw):
    try:
        return learner.device(vec, T, **kw)
    except gua.GuError as err:  # (a store allocated on first use, such as the episode buffers)
        if err.code == ERR_NOMEM:
            pytest.skip(str(err))
        raise


def _against_restatement(learner, g, N, seed, env_id0, bar=None):
    """Two launches of learner.T with rows and statistics on the engine whose first env has the global id env_id0; rows, statistics,
    env state and every store, whole, by bytes, against the restatement built at that id.  And so that the case cannot pass empty: an
    episode ended, the tables left their fill and, where `bar` is given, some env stood on a cell >= bar.  Returns what _restated
    returns: the restatement, its first reset and its rows."""
    grid = _grid(g)
    vec = _open(N, g, seed, learner, env_id0)
    try:
        o = learner.oracle(grid, seed, N, env_id0)
        first = o.reset()
        assert np.array_equal(vec.reset(), first)
        top, rows = int(o.state.pos.max()), []
        for T in learner.T:
            got = _launch(vec, learner, T, trajectory=True, stats=True)
            want = learner.restate(o, T)
            _same(got, want)
            _same_stores(learner.got(vec, 0, N), learner.want(o), T)
            top = max(top, int(want['obs'].max()))
            rows.append(want)
        _same_state(vec.get_state(), o, 0, 'state')
        ran = dict(o=o, first=first, rows=rows)
        _ran_something(learner, ran)
        assert bar is None or top >= bar
        return ran
    finally:
        vec.close()


def _restated(learner, g, N, seed, env_id0, launches=None):
    """The restatement's side of _against_restatement alone: dict(o=, first=, rows=) after the launches of learner.T."""
    o = learner.oracle(_grid(g), seed, N, env_id0)
    first = o.reset()
    return dict(o=o, first=first, rows=[learner.restate(o, T) for T in (launches or learner.T)])


def _ran_something(learner, ran):
    """An episode ended and the tables left their fill."""
    assert sum(int(want['episodes'].sum()) for want in ran['rows']) > 0
    for name, table, fill in learner.learned(ran['o']):
        assert (table != fill).any(), name


def env_ids(N):
    """The first env ids of the shards the tests run at: one whose low bits disagree with the lane index, one whose batch of N envs
    straddles bit 31, and the highest gu_create admits (env_id0 + num_envs <= 0xFFFFFFFF)."""
    return (77, 2 ** 31 - 40, 2 ** 32 - 1 - N)


def _a_shard_worth_comparing(learner, g, ran, ran0):
    """The conditions under which a comparison at env_id0 != 0 says something, on the restatement alone (`ran` at the id under test,
    `ran0` the same at id 0): an episode ended, every table left its fill, the first reset put envs on every start cell (two at
    least), and the rows differ from those at id 0 -- a kernel that ignored the id would not pass."""
    _ran_something(learner, ran)
    assert len(g['starts']) > 1 and set(ran['first'].tolist()) == set(g['starts'])
    assert any(not np.array_equal(a['obs'], b['obs']) for a, b in zip(ran['rows'], ran0['rows']))


def _shared_grid_beyond_lds(learner, g, bar, seed=3, N=130):
    """Part A of test_gpu_learners_at_scale.py: _against_restatement on a grid beyond LDS, where some env stood on a cell >= bar."""
    assert _grid(g).S > 32767  # gu_lds_block returns 0: the L2 instantiation, the arithmetic deltas
    _against_restatement(learner, g, N, seed, 0, bar)


def _tables_for_setter(learner, o):
    """Tables unlike any the launches made, a different one for every env: the restatement's, scaled and shifted by the env."""
    out = {}
    for name, table, _ in learner.learned(o):
        shift = np.arange(o.n).reshape((-1,) + (1,) * (table.ndim - 1))
        out[name] = (table // 2 + shift.astype(table.dtype)) if table.dtype.kind in 'iu' else table * 0.5 + 0.125 * shift
    return out


def _stores_past_a_boundary(learner, g, N, crossings, launches, seed=5, width=128, before=None, after=None):
    """Part B and Part C: N envs, groups of `width` envs -- the first, the last and those around each env of `crossings` -- each
    against a restatement at the group's first env id.  `before(vec, e0, o)`: what a group needs ahead of the first launch;
    `after(tag, e0, o, got)`: a further check per launch and group."""
    assert N % 64 != 0  # the last wave is partial
    half = width // 2
    for e in crossings:
        assert half <= e and e + half <= N, (e, N)  # the group around the crossing lies inside the batch
    starts = sorted(set([0, N - width] + [e - half for e in crossings]))
    grid = _grid(g)
    vec = _open(N, g, seed, learner)
    try:
        oracles = [(e0, learner.oracle(grid, seed, width, e0)) for e0 in starts]
        first = vec.reset()
        for e0, o in oracles:
            assert np.array_equal(first[e0:e0 + width], o.reset()), e0
            if before is not None:
                before(vec, e0, o)

        def launch_and_compare(T, tag):
            got = _launch(vec, learner, T, trajectory=False, stats=True)
            st = vec.get_state()
            for e0, o in oracles:
                want = learner.restate(o, T)
                for k in ('ret', 'episodes'):
                    assert np.array_equal(np.asarray(got[k][e0:e0 + width], np.int64), np.asarray(want[k], np.int64)), (tag, e0, k)
                _same_state(st, o, e0, (tag, e0))
                stores = learner.got(vec, e0, width)
                _same_stores(stores, learner.want(o), (tag, e0))
                if after is not None:
                    after(tag, e0, o, stores)

        for k, T in enumerate(launches):
            launch_and_compare(T, 'launch %d' % k)
        for e0, o in oracles:  # the high envs' own tables left their fill (by the bytes above, the low envs' carry their own writes only)
            for name, table, fill in learner.learned(o):
                assert (table != fill).any(), (e0, name)
        if learner.install is not None:
            for e in crossings:  # tables installed across the crossing, read back, and learned on
                e0, o = [(e0, o) for e0, o in oracles if e0 == e - half][0]
                tables = _tables_for_setter(learner, o)
                learner.install(vec, tables, e0)
                for f0, p in oracles:  # (every restatement gets the envs it shares with this group: groups may overlap, and a call
                    lo = max(e0, f0)   # that installs tables of no env of a group still ends what that group carried)
                    hi = max(lo, min(e0, f0) + width)
                    learner.restate_install(p, dict((k, t[lo - e0:hi - e0]) for k, t in tables.items()), lo - f0 if lo < hi else 0)
                _same_stores(learner.got(vec, e0, width), learner.want(o), ('installed', e0))
            launch_and_compare(launches[-1], 'after the setter')
    finally:
        vec.close()


def _crossing(bytes_per_env, N, at=2 ** 32):
    """The env in whose store byte `at` of a learner-major store lies; the store of N envs reaches past it."""
    assert bytes_per_env * N > at
    return at // bytes_per_env
