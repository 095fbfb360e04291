"""The overlay slot with boxes as its fourth kind (csrc/gu_overlay.hip; DESIGN.md "Overlays"): the slot tests of
tests/test_gpu_overlay.py restated over wind, fruit, doors AND boxes, on that module's grids, planes and runs.  What the box kernels
compute is checked against the CPU restatement in tests/test_gpu_boxes.py; here the SLOT is checked, with engines that only ever had
one overlay (or none) as the reference: one engine cycled through all four -- so that a reset value, a parameter word or a mask buffer
left by an earlier tenant would show --, refused installs that must leave everything as it was, a new grid that drops the overlay,
and the masks' reset to the slot's reset value.

Shapes as there: 8 x 8 (three planes in LDS) and 150 x 150 (the L2 kernels), N = 130, T = 33.  One box: b = 6 bits on the small grid, so
gu_td_init takes it (64 << 6 rows), and 15 on the large one."""
import functools

import numpy as np
import pytest

import griduniverse_amd as gua
from griduniverse_amd.grid import box_plane

from . import test_gpu_overlay as V
from ._tabular_cases import _spec

pytestmark = pytest.mark.gpu

N, T, SEED = V.N, V.T, V.SEED
KINDS = V.KINDS + ('boxes',)
ON_TARGET = 5
BOX, TARGETS = 1, (3, 10)  # right of the start cell 0: a push right, and again, and a third against what lies behind


@functools.lru_cache(maxsize=None)
def _case(name):
    g, planes = V._case(name)
    return g, dict(planes, boxes=box_plane(g['W'], g['H'], [BOX], list(TARGETS)))


def _install(eng, kind, plane):
    if kind == 'boxes':
        eng.set_boxes(plane, ON_TARGET)
    else:
        V._install(eng, kind, plane)


def _plane(eng, kind):
    if kind == 'boxes':
        got = eng.get_boxes()
        return None if got is None else got[0]
    return V._plane(eng, kind)


def _masks(eng, kind):
    return eng.get_boxes_state() if kind == 'boxes' else V._masks(eng, kind)


def _set_masks(eng, kind, masks):
    eng.set_boxes_state(masks) if kind == 'boxes' else V._set_masks(eng, kind, masks)


def _bits(kind):
    return 6 if kind == 'boxes' else V._bits(kind)


def _reset_value(kind):
    return BOX if kind == 'boxes' else 0


def _pattern(kind, g):
    """Masks that differ from the reset value for most envs and differ between neighbours; under boxes: free cells."""
    if kind != 'boxes':
        return V._pattern(kind)
    free = np.array([s for s in range(g['W'] * g['H']) if s not in g['walls'] + g['goals'] + g['lava']], np.uint32)
    return free[(np.arange(N) * 7 + 1) % len(free)]


def _run(vec, kind):
    out = V._run(vec, kind)
    if kind == 'boxes':
        words = _masks(vec.engine, kind)
        assert (words != BOX).any()  # (the run pushed boxes: the words compared are not all the reset value)
        out['masks'] = words.tobytes()
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


# ---- 1: one slot, cycled: boxes behind every other tenant, and every other tenant behind boxes ----
@pytest.mark.parametrize('grid', ['open8', 'open150'])
def test_one_engine_cycled_through_the_four_overlays_equals_engines_that_only_had_one(grid):
    g, planes = _case(grid)
    vec = gua.VecGridUniverse(N, template=_spec(g), seed=SEED)
    try:
        had = None
        for kind in (None, 'boxes', None, 'wind', None, 'boxes', None, 'fruit', None, 'boxes', None, 'doors', None, 'boxes', None):
            if kind:
                _install(vec.engine, kind, planes[kind])
            elif had:
                _install(vec.engine, had, None)
            for k in KINDS:
                assert (_plane(vec.engine, k) is not None) == (k == kind), (kind, k)
            st = vec.engine.stores()
            assert st['overlay'] == (KINDS.index(kind) + 1 if kind else 0)
            vec.seed(SEED)
            vec.reset()
            got, want = _run(vec, kind), _reference(grid, kind)
            assert got['family'] == want['family'] and (got['family'] == kind if kind else got['family'] not in KINDS)
            for k in want:
                assert got[k] == want[k], (kind, had, k)
            had = kind
        # (each overlay changed what the envs did or were paid)
        assert len({_reference(grid, k)['uniform obs'] + _reference(grid, k)['uniform reward'] for k in (None,) + KINDS}) == 5
    finally:
        vec.close()


# ---- 2: refusals leave the engine alone ----
def _invalid(kind, g, planes):
    if kind != 'boxes':
        return V._invalid(kind, g, planes)
    plane = planes[kind].copy()
    plane[g['walls'][0]] = 1  # a target on a wall
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
            _set_masks(eng, have, _pattern(have, g))

        def snapshot():
            masks = _masks(eng, have)
            extra = eng.get_wind()[1] if have == 'wind' else eng.get_boxes()[1:] if have == 'boxes' else None
            return (_plane(eng, have).tobytes(), extra, None if masks is None else masks.tobytes(), eng.td_get_q().tobytes(), eng.td_rows)

        before = snapshot()
        assert before[4] == 64 << _bits(have) and (before[2] is None or (np.frombuffer(before[2], np.uint32) != _reset_value(have)).any())
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
        st = eng.stores()
        assert st['overlay'] == 0 and st['overlay_bits'] == 0
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
@pytest.mark.parametrize('kind', ['fruit', 'doors', 'boxes'])
def test_reset_sets_the_masks_of_exactly_the_envs_it_takes_to_the_slots_reset_value(kind):
    g, planes = _case('open8')
    vec = gua.VecGridUniverse(N, template=_spec(g), seed=SEED)
    try:
        eng = vec.engine
        _install(eng, kind, planes[kind])
        init = _reset_value(kind)
        assert (_masks(eng, kind) == init).all()  # the install itself
        vec.reset()
        pattern = _pattern(kind, g)
        assert (pattern != init).sum() > N // 2
        take = np.arange(N) % 3 == 0
        _set_masks(eng, kind, pattern)
        vec.reset(take.astype(np.uint8))  # gu_reset under a mask of envs
        assert np.array_equal(_masks(eng, kind), np.where(take, init, pattern))
        _set_masks(eng, kind, pattern)
        done = (np.arange(N) % 5 < 2).astype(np.int32)
        vec.set_state(done=done)
        eng.reset_done()  # gu_reset_done: the done envs only
        assert np.array_equal(_masks(eng, kind), np.where(done != 0, init, pattern))
        assert not vec.get_state()['done'].any()
        _set_masks(eng, kind, pattern)
        vec.reset()  # every env
        assert (_masks(eng, kind) == init).all()
    finally:
        vec.close()
