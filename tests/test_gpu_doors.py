"""Doors, keys and levers on the device (gu_set_doors; csrc/gu_doors.hip and the door gu_td_kernel instantiations) against the CPU
restatement tests/_doors_oracle.py: step, rollout and td_run compared byte for byte -- rows, statistics, positions, masks, tables --,
twins on engines without doors that do not rest on the restatement, every reset path, and the engine after the doors have been
taken away against one that never had any.  (The calls that have no door form: tests/test_gpu_overlay.py.)

Every comparison with the restatement also asserts on the restatement's own log that the run met a bump on a closed door, a passage
through an open one, a key pick-up, a lever pulled open and a lever pulled shut.  Env 0 sees to that: it is placed on the case's
`anchor` cell with all doors shut, from where a few moves (`tour`) meet all five -- handed to it as actions (step, stream), as rows of
the policy table (greedy, sample), or found by the seed (uniform, td_run: the seeds below were searched with the restatement alone)."""
import functools

import numpy as np
import pytest

import griduniverse_amd as gua
from griduniverse_amd.algorithms.temporal_difference import q_learning
from griduniverse_amd.grid import door_plane

from . import _doors_oracle as O
from ._overlays import METHODS, same_state, scatter as _scatter
from ._tabular_cases import GRIDS, _eps, _grid, _same, _spec

pytestmark = pytest.mark.gpu

_same_state = functools.partial(same_state, kind='doors')
UP, RIGHT, DOWN, LEFT = 0, 1, 2, 3


@functools.lru_cache(maxsize=None)
def _case(name):
    """(grid dict, door plane uint8[S], anchor cell, tour).  'default4x4': door of slot 0 at 14 in front of the goal, its key at 3, a
    lever of slot 1 at 5 with its door at 10.  'maze11': three slots along the corridor that leaves the start -- key, lever, a slot
    with two door cells.  'open150': 150 x 150 cells without walls -- two planes fit 64 KiB of LDS there and three (67 536 bytes) do
    not: the L2 kernels -- with four slots near the start.  'full8': an open 8 x 8 grid with a door row of 8 slots behind a row of their
    openers, a key for slot 0 and levers for slots 1 .. 7."""
    if name == 'default4x4':
        g = GRIDS['default4x4']()
        plane = door_plane(4, 4, {0: 14, 1: 10}, keys={0: 3}, levers={1: 5})
        # 2 -> 3 (key) -> 7 -> 6 -> 5 (lever open) -> 9 -> 10 (passage) -> 6 -> 5 (lever shut) -> 9 -> bump on 10
        return g, plane, 2, (RIGHT, DOWN, LEFT, LEFT, DOWN, RIGHT, UP, LEFT, DOWN, RIGHT)
    if name == 'maze11':
        g = GRIDS['maze11']()
        plane = door_plane(11, 11, {0: 45, 1: 23, 2: [67, 102]}, keys={0: 13, 2: 100}, levers={1: 12, 2: 34})
        # 14 (the start) -> 13 (key) -> 12 (lever open) -> 23 (passage) -> 12 (lever shut) -> bump on 23
        return g, plane, 14, (LEFT, LEFT, DOWN, UP, DOWN)
    if name == 'open150':
        W = H = 150
        S = W * H
        g = dict(W=W, H=H, starts=[0], goals=[S - 1, 3 * W + 3], lava=[2 * W + 5], walls=[])
        assert 2 * ((S + 15) & ~15) <= 65536 < 3 * ((S + 15) & ~15) == 67536
        plane = door_plane(W, H, {0: 2 * W, 1: 3, 2: 2 * W + 1, 3: W + 2}, keys={0: 1, 1: W}, levers={2: W + 1, 3: 2})
        return g, plane, 0, ()
    g = dict(W=8, H=8, starts=[0], goals=[63], lava=[], walls=[])
    plane = door_plane(8, 8, {k: 24 + k for k in range(8)}, keys={0: 8}, levers={k: 8 + k for k in range(1, 8)})
    return g, plane, 0, ()


def _tour_rows(name, pi):
    """`pi` with one-hot rows along the case's tour: a greedy (or sampling) env on the anchor with all doors shut walks the tour."""
    g, plane, anchor, tour = _case(name)
    o = O.DoorsOracle(_grid(g), 0, 1, plane, q0=None)
    o.state.pos[0] = anchor
    rows = {}
    for a in tour:
        s = int(o.state.pos[0])
        assert rows.setdefault(s, a) == a  # (the tour asks one action of a cell)
        o._move(np.array([a], np.int32))
    assert o.saw_everything()
    for s, a in rows.items():
        pi[s] = np.eye(4)[a]
    return pi


def _mappings(plane):
    """The plane as VecGridUniverse.set_doors takes it: dict(doors=, keys=, levers=) of mappings slot -> cells."""
    out = {}
    for name, kind in (('doors', O.DOOR), ('keys', O.KEY), ('levers', O.LEVER)):
        cells = np.flatnonzero(O.kinds_of(plane) == kind)
        out[name] = {int(k): cells[O.slots_of(plane)[cells] == k].tolist() for k in np.unique(O.slots_of(plane)[cells])}
    return out


def _place(name, vec, o, scatter=True):
    """Positions scattered over the free cells and masks drawn at random per env; env 0 on the anchor with all doors shut."""
    g, plane, anchor, _ = _case(name)
    N = o.n
    pos = _scatter(g, N) if scatter else np.full(N, g['starts'][0], np.int32)
    pos[0] = anchor
    masks = np.random.RandomState(N + 1).randint(0, 1 << o.D, N).astype(np.uint32)
    masks[0] = 0
    vec.set_state(pos=pos)
    o.state.pos[:] = pos
    vec.set_doors_open(masks)
    o.set_open(masks)


def _pair(name, N, seed, q0=None, scatter=True):
    """A batch of N envs on the case's grid under its doors and the oracle of it, both reset and then placed."""
    g, plane, _, _ = _case(name)
    vec = gua.VecGridUniverse(N, template=_spec(g), seed=seed)
    o = O.DoorsOracle(_grid(g), seed, N, plane, q0=q0)
    vec.set_doors(**_mappings(plane))
    assert np.array_equal(vec.engine.get_doors(), plane)
    if q0 is not None:
        vec._ensure_q(q0)
    assert np.array_equal(vec.reset(), o.reset())
    _place(name, vec, o, scatter)
    return vec, o


def _with_byte(plane, cell, byte):
    p = plane.copy()
    p[cell] = byte
    return p


# ---- 1: round trip and errors ----
def test_set_doors_round_trip_and_errors():
    g, plane, _, _ = _case('maze11')
    vec = gua.VecGridUniverse(8, template=_spec(g))
    try:
        eng = vec.engine
        assert vec.doors() is None and eng.get_doors() is None
        for call in (lambda: vec.doors_open(), lambda: eng.set_doors_state(np.zeros(8, np.uint32))):
            with pytest.raises(gua.GuError) as err:  # GU_ERR_STATE while no doors are set
                call()
            assert err.value.code == -4
        vec.set_doors({0: 45, 1: 23, 2: [102, 67]}, keys={0: 13, 2: 100}, levers={1: 12, 2: 34})
        got = vec.doors()
        assert sorted(got) == ['doors', 'keys', 'levers']
        assert {k: v.tolist() for k, v in got['doors'].items()} == {0: [45], 1: [23], 2: [67, 102]}
        assert {k: v.tolist() for k, v in got['keys'].items()} == {0: [13], 2: [100]}
        assert {k: v.tolist() for k, v in got['levers'].items()} == {1: [12], 2: [34]}
        assert np.array_equal(eng.get_doors(), plane)
        assert np.array_equal(vec.doors_open(), np.zeros(8, np.uint32)) and vec.doors_open(2, 3).shape == (3,)
        vec.set_doors_open([5, 7, 1], env0=2)
        assert np.array_equal(vec.doors_open(), np.array([0, 0, 5, 7, 1, 0, 0, 0], np.uint32))
        with pytest.raises(gua.GuError) as err:  # a bit at or above D
            eng.set_doors_state(np.array([8], np.uint32), 0)
        assert err.value.code == -1
        wall, goal = g['walls'][0], g['goals'][0]
        free = [s for s in O.free_cells(g) if not plane[s]]
        bad_planes = [_with_byte(plane, 45, 16 | 128), _with_byte(plane, 45, 16 | 64), _with_byte(plane, 45, 16 | 8), _with_byte(plane, 45, 5),  # bits 7, 6, 3; kind 0 with a slot
                      _with_byte(_with_byte(_with_byte(_with_byte(plane, 67, 16 | 3), 102, 16 | 3), 100, 32 | 3), 34, 48 | 3),  # slot 2 missing (0, 1, 3 in use)
                      _with_byte(plane, 23, 0),  # slot 1 without a door
                      _with_byte(plane, 12, 0),  # slot 1 without a key or lever
                      _with_byte(_with_byte(plane, free[0], 16 | 8), free[1], 32 | 8),  # a ninth slot
                      _with_byte(plane, wall, 16), _with_byte(plane, wall, 32), _with_byte(plane, goal, 48), np.zeros(121, np.uint8)]
        for i, bad in enumerate(bad_planes):
            with pytest.raises(gua.GuError) as err:
                eng.set_doors(bad)
            assert err.value.code == -1, i
        assert np.array_equal(eng.get_doors(), plane) and np.array_equal(vec.doors_open()[2:5], [5, 7, 1])  # a refused call changes nothing
        vec.set_doors({0: 45, 1: 23, 2: 67}, keys={0: 13, 2: 100}, levers={1: 12})  # set_doors clears every mask
        assert not vec.doors_open().any()
        vec.set_doors(None)
        assert vec.doors() is None
    finally:
        vec.close()


# ---- 2: step and step_device ----
@pytest.mark.parametrize('N', [1, 63, 256])
@pytest.mark.parametrize('auto', [True, False])
@pytest.mark.parametrize('case', ['default4x4', 'maze11'])
def test_step_and_step_device_equal_the_oracle(case, auto, N):
    T = 60
    vec, o = _pair(case, N, 4)
    try:
        g, plane, anchor, tour = _case(case)
        vec.auto_reset = auto
        acts = np.random.RandomState(11).randint(-4, 4, (T, N)).astype(np.int32)
        acts[:len(tour), 0] = tour
        lever = int(np.flatnonzero(O.kinds_of(plane) == O.LEVER)[0])
        beside = next(c for c in O._neighbours(g, lever) if c not in g['walls'] and O.kinds_of(plane)[c] != O.DOOR)
        toward = {-g['W']: UP, 1: RIGHT, g['W']: DOWN, -1: LEFT}[lever - beside]
        for i in range(T):
            a = acts[i].copy()
            if i == 30:
                # env 0 stands beside a lever and is given a rejected action: it does not step, and its mask and position stay
                pos = vec.get_state()['pos']
                pos[0] = beside
                vec.set_state(pos=pos, done=np.zeros(N, np.int32))
                o.state.pos[:], o.state.done[:] = pos, 0
                before = vec.doors_open()
                a[0] = 7
                with pytest.raises(gua.GuError) as err:
                    vec.step(a)
                assert err.value.code == -1
                o.step(a, auto)
                _same_state(vec, o)
                assert vec.doors_open(0, 1)[0] == before[0] and vec.get_state()['pos'][0] == beside
                acts[i + 1, 0] = toward  # ... and the valid action behind it pulls the lever
                continue
            obs, rew, don, _ = vec.step(a, zero_copy=(i % 2 == 1))
            w_obs, w_rew, w_don, rejected = o.step(a, auto)
            assert not rejected.any()
            assert np.array_equal(obs, w_obs) and np.array_equal(rew, w_rew) and np.array_equal(don, w_don != 0), i
            if i == 31:
                assert obs[0] == lever and (o.open[0] ^ before[0]) == 1 << (int(plane[lever]) & 7)
        assert o.saw_everything(), o.log
        _same_state(vec, o)
        # the same rows from the device-resident stream
        vec.seed(4)
        o2 = O.DoorsOracle(o.grid, 4, N, plane, q0=None)
        assert np.array_equal(vec.reset(), o2.reset())
        assert not vec.doors_open().any()
        _place(case, vec, o2)
        vec.engine.upload_actions(acts)
        for i in range(T):
            vec.engine.step_device(i, auto)
            obs, rew, don = vec.engine.read_outputs()
            w_obs, w_rew, w_don, _ = o2.step(acts[i], auto)
            assert np.array_equal(obs, w_obs) and np.array_equal(rew, w_rew) and np.array_equal(don != 0, w_don != 0), i
        assert o2.saw_everything(), o2.log
        _same_state(vec, o2)
    finally:
        vec.close()


# ---- 3: rollout ----
def _policy_table(case, S):
    pi = np.random.RandomState(1).dirichlet(np.ones(4), S)
    pi[::7] = np.eye(4)[np.arange(len(pi[::7])) % 4]  # one-hot rows: thresholds that no word reaches
    return _tour_rows(case, pi)


# uniform rollouts of one env: the seeds at which the restatement's env 0 meets all five events within 50 steps from the anchor
UNIFORM_SEED_N1 = {('default4x4', True): 8, ('default4x4', False): 8, ('maze11', True): 4, ('maze11', False): 4}


@pytest.mark.parametrize('N', [200, 1])
@pytest.mark.parametrize('auto', [True, False])
@pytest.mark.parametrize('policy', ['uniform', 'stream', 'greedy', 'sample'])
@pytest.mark.parametrize('case', ['default4x4', 'maze11'])
def test_rollout_equals_the_oracle(case, policy, auto, N):
    T = 50
    seed = UNIFORM_SEED_N1[(case, auto)] if (N == 1 and policy == 'uniform') else 6
    vec, o = _pair(case, N, seed)
    try:
        S = o.grid.S
        pi = _policy_table(case, S) if policy in ('greedy', 'sample') else None
        acts = None
        if policy == 'stream':
            acts = np.random.RandomState(2).randint(0, 4, (T, N)).astype(np.int32)
            tour = _case(case)[3]
            acts[:len(tour), 0] = tour
        if pi is not None:
            vec.engine.vi_set(np.zeros(S), pi)
        want = o.rollout(T, policy, auto, actions=acts, pi=pi)
        assert o.saw_everything(), o.log
        # two launches of 25 ...
        halves = [vec.rollout(25, policy, actions=None if acts is None else acts[k * 25:(k + 1) * 25], auto_reset=auto, stats=True) for k in range(2)]
        assert vec.engine.rollout_last_form()['family'] == 'doors'
        for k in ('obs', 'reward', 'done'):
            assert np.array_equal(np.concatenate([h[k] for h in halves]), want[k]), k
        assert np.array_equal(halves[0]['ret'] + halves[1]['ret'], want['ret'])
        assert np.array_equal(halves[0]['episodes'] + halves[1]['episodes'], want['episodes'])
        _same_state(vec, o)
        # ... equal one of 50
        o2 = O.DoorsOracle(o.grid, seed, N, o.door, q0=None)
        vec.seed(seed)
        assert np.array_equal(vec.reset(), o2.reset())
        _place(case, vec, o2)
        got = vec.rollout(T, policy, actions=acts, auto_reset=auto, stats=True)
        _same(got, want)
        _same_state(vec, o)
        # statistics alone
        vec.seed(seed)
        vec.reset()
        _place(case, vec, o2)
        only = vec.rollout(T, policy, actions=acts, auto_reset=auto, trajectory=False, stats=True)
        assert np.array_equal(only['ret'], want['ret']) and np.array_equal(only['episodes'], want['episodes'])
        _same_state(vec, o)
    finally:
        vec.close()


# ---- 4: twins that do not rest on the oracle ----
def _twin_pair(g, plane, twin_g, N, seed, mask, scatter):
    vec = gua.VecGridUniverse(N, template=_spec(g), seed=seed)
    twin = gua.VecGridUniverse(N, template=_spec(twin_g), seed=seed)
    vec.set_doors(**_mappings(plane))
    assert np.array_equal(vec.reset(), twin.reset())
    if scatter:
        free = np.array([s for s in O.free_cells(twin_g) if not plane[s]], np.int32)  # (no env starts on a door: the twin has a wall there)
        pos = free[np.random.RandomState(N).randint(0, len(free), N)]
        vec.set_state(pos=pos)
        twin.set_state(pos=pos)
    vec.set_doors_open(np.full(N, mask, np.uint32))
    return vec, twin


@pytest.mark.parametrize('policy', ['uniform', 'greedy'])
@pytest.mark.parametrize('kind', ['walled_in', 'all_open'])
@pytest.mark.parametrize('case', ['default4x4', 'maze11'])
def test_rollout_twins_on_engines_without_doors(case, kind, policy):
    N, T = 200, 60
    if kind == 'walled_in':  # the keys cannot be reached and the masks are 0: the doors are walls
        g, plane, twin_g = O.walled_in_case(GRIDS[case]())
        mask, autos = 0, (True, False)
    else:  # keys only and every mask all ones, never reset: the doors are free cells
        g, plane = O.keys_only_case(GRIDS[case]())
        twin_g, mask, autos = g, 3, (False,)
    for auto in autos:
        vec, twin = _twin_pair(g, plane, twin_g, N, 5, mask, scatter=True)
        try:
            if policy == 'greedy':
                pi = np.random.RandomState(3).dirichlet(np.ones(4), g['W'] * g['H'])
                for v in (vec, twin):
                    v.engine.vi_set(np.zeros(len(pi)), pi)
            got = vec.rollout(T, policy, auto_reset=auto, stats=True)
            assert vec.engine.rollout_last_form()['family'] == 'doors'
            _same(got, twin.rollout(T, policy, auto_reset=auto, stats=True))
            assert twin.engine.rollout_last_form()['family'] != 'doors'
            a, b = vec.get_state(), twin.get_state()
            assert all(np.array_equal(a[k], b[k]) for k in ('pos', 'done', 'episode', 'tcount'))
            assert (vec.doors_open() == mask).all()
            door_cells = np.flatnonzero(O.kinds_of(plane) == O.DOOR)
            assert np.isin(got['obs'], door_cells).any() == (kind == 'all_open')
        finally:
            vec.close()
            twin.close()


@pytest.mark.parametrize('method', ['q_learning', 'sarsa'])
@pytest.mark.parametrize('kind', ['walled_in', 'all_open'])
@pytest.mark.parametrize('case', ['default4x4', 'maze11'])
def test_td_run_twins_on_engines_without_doors(case, kind, method):
    N, q0 = 130, 0.25
    if kind == 'walled_in':
        g, plane, twin_g = O.walled_in_case(GRIDS[case]())
        mask, T, scatter = 0, 150, True
    else:
        # td_run always resets lazily, and a reset shuts the doors: a run so short that no env that leaves the start ends its episode
        g, plane = O.keys_only_case(GRIDS[case]())
        twin_g, mask, T, scatter = g, 3, 5 if case == 'default4x4' else 20, False
    vec, twin = _twin_pair(g, plane, twin_g, N, 5, mask, scatter)
    try:
        S = g['W'] * g['H']
        for v in (vec, twin):
            v._ensure_q(q0)
        kw = dict(alpha=0.25, discount_factor=0.9, epsilon=0.3, trajectory=True, stats=True)
        got = vec.td_run(T, method, **kw)
        _same(got, twin.td_run(T, method, **kw))
        assert kind == 'walled_in' or not got['done'].any()
        q, want = vec.q_table(), twin.q_table()
        assert q.shape == (N, S << 2, 4) and want.shape == (N, S, 4)
        assert q[:, mask * S:(mask + 1) * S].tobytes() == want.tobytes() and (want != q0).any()
        rest = np.delete(q, np.s_[mask * S:(mask + 1) * S], axis=1)
        assert (rest == q0).all()  # every other row still holds q0
        assert (vec.doors_open() == mask).all()
    finally:
        vec.close()
        twin.close()


# ---- 5: the L2 path ----
def test_three_planes_that_do_not_fit_lds_rollout_and_td_run():
    N, T = 64, 30
    vec, o = _pair('open150', N, 3, q0=0.0, scatter=False)
    try:
        got = vec.rollout(T, 'uniform', auto_reset=True, stats=True)
        form = vec.engine.rollout_last_form()
        assert form['family'] == 'doors' and form['lds_bytes'] == 0
        _same(got, o.rollout(T, 'uniform', True))
        assert o.saw_everything(), o.log
        _same_state(vec, o)
        o.log = dict.fromkeys(O.EVENTS, 0)
        for method in ('q_learning', 'sarsa'):
            got = vec.td_run(T, method, alpha=0.25, discount_factor=0.9, epsilon=0.3, trajectory=True, stats=True)
            _same(got, o.td_run(T, METHODS[method], 0.25, 0.9, _eps(0.3)))
        assert o.saw_everything(), o.log
        assert vec.q_table().shape == (N, 22500 << 4, 4) and vec.q_table().tobytes() == o.q.tobytes()
        _same_state(vec, o)
    finally:
        vec.close()


# ---- 6: slot 7 ----
def test_eight_slots_reach_slot_7():
    N, T = 64, 300
    vec, o = _pair('full8', N, 5, scatter=False)
    try:
        got = vec.rollout(T, 'uniform', auto_reset=False, stats=True)
        _same(got, o.rollout(T, 'uniform', False))
        _same_state(vec, o)
        obs = np.concatenate([np.zeros((1, N), np.int32), got['obs']])
        pulls = ((obs[1:] == 15) & (obs[:-1] != 15)).sum(axis=0)  # entries of cell 15, the lever of slot 7
        assert (pulls >= 2).any()  # set and cleared again
        assert ((obs[1:] == 31) & (obs[:-1] != 31)).any()  # ... and its door at 31 let an env in
        assert o.saw_everything(), o.log
        top = np.full(N, 0x81, np.uint32)
        vec.set_doors_open(top)
        assert np.array_equal(vec.doors_open(), top)
        with pytest.raises(gua.GuError) as err:  # bit 8 is no slot
            vec.engine.set_doors_state(np.array([0x100], np.uint32))
        assert err.value.code == -1
        vec._ensure_q(0.0)
        assert vec.q_table(0, 1).shape == (1, 64 << 8, 4)
    finally:
        vec.close()


# ---- 7: td_run ----
# one learner: the seeds at which the restatement's env 0 meets all five events within 300 steps (the first one tried does)
TD_SEED_N1 = {('default4x4', 'q_learning'): 0, ('default4x4', 'sarsa'): 0, ('maze11', 'q_learning'): 0, ('maze11', 'sarsa'): 0}


@pytest.mark.parametrize('N', [1, 130])
@pytest.mark.parametrize('method', ['q_learning', 'sarsa'])
@pytest.mark.parametrize('case', ['default4x4', 'maze11'])
def test_td_run_tables_rows_and_stats_equal_the_oracle(case, method, N):
    T = 300
    seed = TD_SEED_N1[(case, method)] if N == 1 else 3
    vec, o = _pair(case, N, seed, q0=0.0 if N == 1 else 0.5)
    try:
        S, D = o.grid.S, o.D
        if N == 130:  # tables of [n, S << D, 4] through set_q_table / q_table
            q = np.random.RandomState(7).uniform(-1, 1, (N, S << D, 4))
            vec.set_q_table(q)
            o.q[:] = q
            assert vec.q_table(3, 2).tobytes() == q[3:5].tobytes()
        want = o.td_run(T, METHODS[method], 0.25, 0.9, _eps(0.3))
        assert o.saw_everything(), o.log
        got = vec.td_run(T, method, alpha=0.25, discount_factor=0.9, epsilon=0.3, trajectory=True, stats=True)
        _same(got, want)
        assert vec.q_table().shape == (N, S << D, 4) and vec.q_table().tobytes() == o.q.tobytes()
        _same_state(vec, o)
    finally:
        vec.close()


# ---- 8: the SARSA carry ----
def test_sarsa_split_in_two_carries_its_action_and_set_doors_and_set_doors_open_drop_it():
    vec, o = _pair('maze11', 130, 8, q0=0.0)
    twin, o1 = _pair('maze11', 130, 8, q0=0.0)
    try:
        kw = dict(alpha=0.5, discount_factor=0.95, epsilon=0.3, trajectory=True, stats=True)
        for T in (100, 100):  # the second launch starts with the first one's a'
            _same(vec.td_run(T, 'sarsa', **kw), o.td_run(T, O.SARSA, 0.5, 0.95, _eps(0.3)))
        assert o.carry_valid and (o.carry >= 0).any() and o.saw_everything()
        _same(twin.td_run(200, 'sarsa', **kw), o1.td_run(200, O.SARSA, 0.5, 0.95, _eps(0.3)))  # ... and equals one launch
        assert vec.q_table().tobytes() == twin.q_table().tobytes() == o.q.tobytes()
        masks = o.open.copy()
        vec.set_doors_open(masks)  # the same masks again: the carry goes
        o.set_open(masks)
        _same(vec.td_run(50, 'sarsa', **kw), o.td_run(50, O.SARSA, 0.5, 0.95, _eps(0.3)))
        assert o.carry_valid
        vec.engine.set_doors(o.door)  # the same doors again: tables, positions and counts stay, the masks and the carry go
        q = o.q.copy()
        o.set_doors(o.door)
        assert o.q.tobytes() == q.tobytes()
        _same(vec.td_run(50, 'sarsa', **kw), o.td_run(50, O.SARSA, 0.5, 0.95, _eps(0.3)))
        assert vec.q_table().tobytes() == o.q.tobytes()
        _same_state(vec, o)
    finally:
        vec.close()
        twin.close()


# ---- 9: reset paths ----
def test_every_reset_path_clears_the_masks_of_the_envs_it_resets():
    N = 130
    vec, o = _pair('default4x4', N, 2)
    try:
        _same(vec.rollout(40, 'uniform', auto_reset=False, stats=True), o.rollout(40, 'uniform', False))
        assert o.saw_everything(), o.log
        assert (o.open != 0).sum() > N // 4 and (o.state.done != 0).any() and (o.state.done == 0).any()
        assert (o.open[o.state.done != 0] != 0).any() and (o.open[o.state.done == 0] != 0).any()
        _same_state(vec, o)
        before = o.open.copy()
        vec.set_state(pos=o.state.pos)  # set_state and seed leave the masks alone
        vec.seed(2)
        o.state.episode[:] = 0
        o.state.tcount[:] = 0
        assert np.array_equal(vec.doors_open(), before)
        vec.engine.reset_done()  # the done envs only
        d = o.reset_done()
        assert d.any() and not o.open[d].any() and np.array_equal(o.open[~d], before[~d])
        _same_state(vec, o)
        mask = (np.arange(N) % 3 == 0).astype(np.uint8)
        assert np.array_equal(vec.reset(mask), o.reset(mask))  # the masked envs only
        assert (o.open[mask == 0] != 0).any()
        _same_state(vec, o)
        _same(vec.rollout(60, 'uniform', auto_reset=True, stats=True), o.rollout(60, 'uniform', True))  # the lazy reset
        _same_state(vec, o)
        vec.set_doors_open(np.full(N, 3, np.uint32))
        done = np.zeros(N, np.int32)
        done[::2] = 1
        vec.set_state(done=done)
        o.set_open(np.full(N, 3, np.uint32))
        o.state.done[:] = done
        acts = np.zeros(N, np.int32)
        vec.auto_reset = True
        obs, _, _, _ = vec.step(acts)  # the step kernel's lazy reset
        assert np.array_equal(obs, o.step(acts, True)[0])
        assert not o.open[::2].any() and (o.open[1::2] != 0).all()  # (an env that was not done keeps its mask, but for a lever it may enter)
        _same_state(vec, o)
        assert np.array_equal(vec.reset(), o.reset()) and not vec.doors_open().any()
    finally:
        vec.close()


# ---- 11: clearing the doors ----
def test_an_engine_without_its_doors_again_is_the_engine_that_never_had_any():
    g, plane, _, _ = _case('maze11')
    N, seed = 200, 9
    vec = gua.VecGridUniverse(N, template=_spec(g), seed=seed)
    ref = gua.VecGridUniverse(N, template=_spec(g), seed=seed)
    try:
        vec.set_doors(**_mappings(plane))
        vec.reset()
        vec.td_run(20, 'q_learning')
        vec.rollout(20, 'uniform', auto_reset=True)
        assert vec.engine.rollout_last_form()['family'] == 'doors'
        vec.set_doors(None)
        with pytest.raises(gua.GuError) as err:  # the tables of S << 3 rows went with the doors
            vec.engine.td_run(5)
        assert err.value.code == -4
        with pytest.raises(gua.GuError) as err:  # ... for the other learners too
            vec.engine.nstep_run(5)
        assert err.value.code == -4
        vec.seed(seed)
        assert np.array_equal(vec.reset(), ref.reset())
        for auto in (True, False):
            _same(vec.rollout(100, 'uniform', auto_reset=auto, stats=True), ref.rollout(100, 'uniform', auto_reset=auto, stats=True))
            a, b = vec.engine.rollout_last_form(), ref.engine.rollout_last_form()
            assert a['family'] == b['family'] != 'doors' and a['words'] == b['words']
        acts = np.random.RandomState(3).randint(0, 4, (8, N)).astype(np.int32)
        for i in range(8):
            a, b = vec.step(acts[i]), ref.step(acts[i])
            assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3]))
        for method in ('q_learning', 'sarsa'):
            kw = dict(alpha=0.3, discount_factor=0.9, epsilon=0.2, trajectory=True, stats=True)
            _same(vec.td_run(120, method, **kw), ref.td_run(120, method, **kw))
            assert vec.q_table().shape == (N, 121, 4) and vec.q_table().tobytes() == ref.q_table().tobytes()
        a, b = vec.get_state(), ref.get_state()
        assert all(np.array_equal(a[k], b[k]) for k in ('pos', 'done', 'episode', 'tcount'))
    finally:
        vec.close()
        ref.close()


# ---- 12: the learning claim ----
def test_q_learning_end_to_end_walks_a_shortest_walk_through_the_door():
    """64 learners, O.CLAIM_STEPS = 1400 steps, alpha 0.5, gamma 0.95, epsilon 0.1 on the 7 x 3 grid of tests/test_doors_host.py: the
    tables equal the restatement's byte for byte, and every greedy walk over (cell, mask) rows has the length and the return of the
    breadth-first search's shortest walk, 8 moves and 3.  (The claim's grid has a key and no lever, so the restatement's log is asked
    for bumps, passages and pick-ups here.)"""
    L, seed = O.CLAIM_LEARNERS, 1
    env = gua.GridUniverseEnv(grid_shape=(O.CLAIM_W, O.CLAIM_H), initial_state=O.CLAIM['starts'][0], goal_states=O.CLAIM['goals'], walls=O.CLAIM['walls'])
    q = q_learning(env, O.CLAIM_STEPS, alpha=O.CLAIM_ALPHA, discount_factor=O.CLAIM_GAMMA, epsilon=0.1, num_learners=L, seed=seed, doors=O.CLAIM_DOORS)
    grid, plane = _grid(O.CLAIM), door_plane(O.CLAIM_W, O.CLAIM_H, **O.CLAIM_DOORS)
    o = O.DoorsOracle(grid, seed, L, plane, q0=0.0)
    o.reset()
    o.td_run(O.CLAIM_STEPS, O.Q_LEARNING, O.CLAIM_ALPHA, O.CLAIM_GAMMA, O.CLAIM_EPS_Q16)
    assert all(o.log[k] > 0 for k in ('bump', 'passage', 'key'))
    assert q.shape == (L, 21 << 1, 4) and q.tobytes() == o.q.tobytes()
    want = O.shortest_walk(grid, plane, O.CLAIM['starts'][0])
    assert want == O.CLAIM_WALK
    walks = [O.greedy_walk(grid, plane, q[e]) for e in range(L)]
    assert walks == [want] * L, walks
