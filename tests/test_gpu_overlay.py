"""The overlay slot of an engine (csrc/gu_overlay.hip; DESIGN.md "Overlays"): wind, fruit and doors share one third plane, one array
of masks and one install path.  What each feature computes is checked against its CPU restatement in tests/test_gpu_wind.py,
test_gpu_fruit.py and test_gpu_doors.py; here the SLOT is checked, with engines that only ever had one overlay (or none) as the
reference: one engine cycled through all three, refused installs that must leave everything as it was, a new grid that drops the
overlay, and the masks' reset.

Shapes: an 8 x 8 grid (three planes in LDS) and, for one case, 150 x 150 (two planes fit 64 KiB and three, 67 536 bytes, do not: the
L2 kernels -- the grid tests/test_gpu_doors.py uses for them); N = 130 envs (three waves, the last one partial: the windy kernels run
its dead lanes); T = 33 steps (one full action word, a word boundary and a tail)."""
import functools

import numpy as np
import pytest

import griduniverse_amd as gua
from griduniverse_amd.grid import door_plane, fruit_plane, wind_plane

from ._tabular_cases import _spec

pytestmark = pytest.mark.gpu

N, T, SEED = 130, 33, 11
KINDS = ('wind', 'fruit', 'doors')
GUST_Q16 = 43691
FRUIT_VALUES = (1, 5, -5)


@functools.lru_cache(maxsize=None)
def _case(name):
    """(grid dict, {kind: plane uint8[S]}).  The planes sit near the start cell 0, where 33 uniform steps of 130 envs meet them."""
    if name == 'open8':
        W = H = 8
        g = dict(W=W, H=H, starts=[0], goals=[63], lava=[36], walls=[21, 45])
    else:
        W = H = 150
        S = W * H
        g = dict(W=W, H=H, starts=[0], goals=[S - 1, 3 * W + 3], lava=[2 * W + 5], walls=[])
        assert 2 * ((S + 15) & ~15) <= 65536 < 3 * ((S + 15) & ~15)
    strength = np.zeros(W, int)
    strength[:8] = [0, 1, 2, 1, 0, 3, 1, 0]
    planes = dict(wind=wind_plane(W, H, strength, 'down'),
                  fruit=fruit_plane(W, H, [2, W + 1, 3 * W + 3 + 1, 2 * W], ['apple', 'lemon', 'melon', 'apple']),
                  doors=door_plane(W, H, {0: [2 * W + 1, 2 * W + 2], 1: W + 2}, keys={0: 1}, levers={1: W}))
    return g, planes


def _install(eng, kind, plane):
    if kind == 'wind':
        eng.set_wind(plane, GUST_Q16 if plane is not None else 0)
    elif kind == 'fruit':
        eng.set_fruit(plane, FRUIT_VALUES)
    else:
        eng.set_doors(plane)


def _plane(eng, kind):
    got = {'wind': eng.get_wind, 'fruit': eng.get_fruit, 'doors': eng.get_doors}[kind]()
    return None if got is None else got[0] if kind != 'doors' else got


def _masks(eng, kind):
    return {'wind': lambda: None, 'fruit': eng.get_fruit_state, 'doors': eng.get_doors_state}[kind]()


def _set_masks(eng, kind, masks):
    {'fruit': eng.set_fruit_state, 'doors': eng.set_doors_state}[kind](masks)


def _bits(kind):
    return {'wind': 0, 'fruit': 4, 'doors': 2}[kind]


def _pattern(kind):
    """Masks that are not zero for most envs and differ between neighbours."""
    return ((np.arange(N) * 7 + 1) % (1 << _bits(kind))).astype(np.uint32)


def _run(vec, kind):
    """A T-step uniform rollout with rows and statistics, a T-step rollout on a caller's stream, one step: everything they leave
    behind, as bytes."""
    eng = vec.engine
    out = {}
    got = vec.rollout(T, 'uniform', auto_reset=True, stats=True)
    out['family'] = eng.rollout_last_form()['family']
    for k in ('obs', 'reward', 'done', 'ret', 'episodes'):
        out['uniform ' + k] = np.asarray(got[k]).tobytes()
    got = vec.rollout(T, actions=np.random.RandomState(5).randint(0, 4, (T, N)).astype(np.int32), auto_reset=True)
    for k in ('obs', 'reward', 'done'):
        out['stream ' + k] = np.asarray(got[k]).tobytes()
    obs, reward, done = eng.step(np.arange(N, dtype=np.int32) % 4, True)
    out['step'] = obs.tobytes() + reward.tobytes() + done.tobytes()
    st = vec.get_state()
    for k in ('pos', 'done', 'episode', 'tcount'):
        out['state ' + k] = np.asarray(st[k]).tobytes()
    if kind in ('fruit', 'doors'):
        masks = _masks(eng, kind)
        assert masks.any()  # (the run ate fruit / opened doors: the masks compared are not all zero)
        out['masks'] = masks.tobytes()
    return out


@functools.lru_cache(maxsize=None)
def _reference(grid, kind):
    """What _run leaves on a fresh engine that only ever had the overlay `kind` (None: never any)."""
    g, planes = _case(grid)
    vec = gua.VecGridUniverse(N, template=_spec(g), seed=SEED)
    try:
        if kind:
            _install(vec.engine, kind, planes[kind])
        vec.reset()
        return _run(vec, kind)
    finally:
        vec.close()


# ---- 1: one slot, cycled ----
@pytest.mark.parametrize('grid', ['open8', 'open150'])
def test_one_engine_cycled_through_the_overlays_equals_engines_that_only_had_one(grid):
    g, planes = _case(grid)
    vec = gua.VecGridUniverse(N, template=_spec(g), seed=SEED)
    try:
        had = None
        for kind in (None, 'wind', None, 'fruit', None, 'doors', None):
            if kind:
                _install(vec.engine, kind, planes[kind])
            elif had:
                _install(vec.engine, had, None)
            for k in KINDS:
                assert (_plane(vec.engine, k) is not None) == (k == kind), (kind, k)
            vec.seed(SEED)
            vec.reset()
            got, want = _run(vec, kind), _reference(grid, kind)
            assert got['family'] == want['family'] and (got['family'] == kind if kind else got['family'] not in KINDS)
            for k in want:
                assert got[k] == want[k], (kind, had, k)
            had = kind
        # (each overlay changed what the envs did or were paid)
        assert len({_reference(grid, k)['uniform obs'] + _reference(grid, k)['uniform reward'] for k in (None,) + KINDS}) == 4
    finally:
        vec.close()


# ---- 2: refusals leave the engine alone ----
def _invalid(kind, g, planes):
    plane = planes[kind].copy()
    if kind == 'wind':
        plane[5] = 0x80  # a wind byte with a high bit
    elif kind == 'fruit':
        plane[g['walls'][0]] = (1 << 5) | 4  # fruit on a wall
    else:
        plane[:] = 0
        plane[20] = 1 << 4  # a door of slot 0 and no key or lever for it
    return plane


@pytest.mark.parametrize('have', KINDS)
def test_a_refused_install_leaves_plane_masks_and_q_tables_as_they_were(have):
    g, planes = _case('open8')
    vec = gua.VecGridUniverse(N, template=_spec(g), seed=SEED)
    try:
        eng = vec.engine
        _install(eng, have, planes[have])
        vec.reset()
        eng.td_init(0.25)
        eng.td_run(T)  # (tables that are not all q0)
        if _bits(have):
            _set_masks(eng, have, _pattern(have))

        def snapshot():
            masks = _masks(eng, have)
            return (_plane(eng, have).tobytes(), eng.get_wind()[1] if have == 'wind' else None, None if masks is None else masks.tobytes(),
                    eng.td_get_q().tobytes(), eng.td_rows)

        before = snapshot()
        assert before[4] == 64 << _bits(have) and (before[2] is None or np.frombuffer(before[2], np.uint32).any())
        for other in KINDS:
            if other == have:
                continue
            with pytest.raises(gua.GuError) as err:  # another overlay: unsupported, and the message names the one that is set
                _install(eng, other, planes[other])
            assert err.value.code == -6 and have in str(err.value)
            with pytest.raises(gua.GuError) as err:  # ... and so is taking that other one away
                _install(eng, other, None)
            assert err.value.code == -6
            assert _plane(eng, other) is None and snapshot() == before
        with pytest.raises(gua.GuError) as err:  # an invalid plane of the same feature: its own error
            _install(eng, have, _invalid(have, g, planes))
        assert err.value.code == -1
        assert snapshot() == before
        eng.td_run(T)  # (the tables are still the engine's)
    finally:
        vec.close()


# ---- 3: a new grid drops the overlay ----
@pytest.mark.parametrize('kind', KINDS)
def test_a_new_grid_drops_the_overlay_and_its_q_rows(kind):
    g, planes = _case('open8')
    vec = gua.VecGridUniverse(N, template=_spec(g), seed=SEED)
    try:
        eng = vec.engine
        _install(eng, kind, planes[kind])
        eng.td_init(0.0)
        assert eng.td_rows == 64 << _bits(kind) and eng.td_get_q(0, 2).shape == (2, 64 << _bits(kind), 4)
        eng.set_grid(_spec(g))
        assert all(_plane(eng, k) is None for k in KINDS) and eng.td_rows == 64
        if _bits(kind):
            with pytest.raises(gua.GuError) as err:  # (tables of S << bits rows went with the masks)
                eng.td_get_q(0, 2)
            assert err.value.code == -4
        eng.td_init(0.0)
        assert eng.td_get_q(0, 2).shape == (2, 64, 4)
        eng.look_step_ahead([0], [1])  # (refused while an overlay is set)
        vec.reset()
        vec.rollout(T, 'uniform', auto_reset=True)
        assert eng.rollout_last_form()['family'] not in KINDS
    finally:
        vec.close()


# ---- 4: reset ----
@pytest.mark.parametrize('kind', ['fruit', 'doors'])
def test_reset_clears_the_masks_of_exactly_the_envs_it_takes(kind):
    g, planes = _case('open8')
    vec = gua.VecGridUniverse(N, template=_spec(g), seed=SEED)
    try:
        eng = vec.engine
        _install(eng, kind, planes[kind])
        vec.reset()
        pattern = _pattern(kind)
        assert (pattern != 0).sum() > N // 2
        take = np.arange(N) % 3 == 0
        _set_masks(eng, kind, pattern)
        vec.reset(take.astype(np.uint8))  # gu_reset under a mask of envs
        assert np.array_equal(_masks(eng, kind), np.where(take, 0, pattern))
        _set_masks(eng, kind, pattern)
        done = (np.arange(N) % 5 < 2).astype(np.int32)
        vec.set_state(done=done)
        eng.reset_done()  # gu_reset_done: the done envs only
        assert np.array_equal(_masks(eng, kind), np.where(done != 0, 0, pattern))
        assert not vec.get_state()['done'].any()
        _set_masks(eng, kind, pattern)
        vec.reset()  # every env
        assert not _masks(eng, kind).any()
    finally:
        vec.close()
