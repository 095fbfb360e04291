"""The overlay slot of an engine (csrc/gu_overlay.hip; DESIGN.md "Overlays"): wind, fruit, doors, boxes and errands share one third
plane, one array of masks and one install path.  What each feature computes is checked against its CPU restatement in
tests/test_gpu_wind.py, test_gpu_fruit.py, test_gpu_doors.py, test_gpu_boxes.py and test_gpu_errands.py; here the SLOT is checked, for every kind of tests/_overlays.py alike, with
engines that only ever had one overlay (or none) as the reference: one engine cycled through the kinds -- so that a reset value, a
parameter word or a mask buffer left by an earlier tenant would show --, refused installs that must leave everything as it was, a new
grid that drops the overlay, the masks' reset to the slot's reset value, and every call that has no overlay form refused while a
kind is set.

Shapes: an 8 x 8 grid (three planes in LDS) and, for the cycle, 150 x 150 (two planes fit 64 KiB and three, 67 536 bytes, do not: the
L2 kernels); N = 130 envs (three waves, the last one partial: the windy kernels run its dead lanes); T = 33 steps (one full action
word, a word boundary and a tail).  One box: b = 6 bits on the small grid, so gu_td_init takes it (64 << 6 rows), and 15 on the large
one.  The errands lie on the fruit plane's cells (four fruit and the registry's two instructions: seven bits).  The refusals: the
11 x 11 maze, N = 64."""
import functools

import numpy as np
import pytest

import griduniverse_amd as gua
from griduniverse_amd.algorithms.exploration import ucb_tables
from griduniverse_amd.grid import box_plane, door_plane, fruit_plane, wind_plane

from ._overlays import NO_OVERLAY_CALLS, OVERLAYS, no_overlay_context
from ._tabular_cases import GRIDS, _spec, code

pytestmark = pytest.mark.gpu

N, T, SEED = 130, 33, 11
KINDS = tuple(OVERLAYS)
BOX, TARGETS = 1, (3, 10)  # right of the start cell 0: a push right, and again, and a third against what lies behind


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
                  doors=door_plane(W, H, {0: [2 * W + 1, 2 * W + 2], 1: W + 2}, keys={0: 1}, levers={1: W}),
                  boxes=box_plane(W, H, [BOX], list(TARGETS)))
    planes['errands'] = planes['fruit']  # (two apples and a lemon: the registry's two instructions; fruit and errands read one plane two ways)
    return g, planes


def _pattern(kind, g, planes):
    """Masks that differ from the reset value for most envs and differ between neighbours; under boxes: free cells; under errands:
    words that gu_set_errands_state takes (progress 0 or 1, which both of the registry's instructions reach, behind pb = 2 bits)."""
    if kind == 'errands':
        F, i = int(np.count_nonzero(planes[kind])), np.arange(N)
        return (((i * 7 + 1) % (1 << F)) | ((i % 2) << F) | ((i // 2 % 2) << (F + 2))).astype(np.uint32)
    if kind != 'boxes':
        return ((np.arange(N) * 7 + 1) % (1 << OVERLAYS[kind].bits(planes[kind]))).astype(np.uint32)
    free = np.array([s for s in range(g['W'] * g['H']) if s not in g['walls'] + g['goals'] + g['lava']], np.uint32)
    return free[(np.arange(N) * 7 + 1) % len(free)]


def _run(vec, kind, plane):
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
    masks = OVERLAYS[kind].masks(eng) if kind else None
    if masks is not None:
        assert (masks != OVERLAYS[kind].reset_value(plane)).any()  # (the run ate fruit / opened doors / pushed boxes: not all the reset value)
        out['masks'] = masks.tobytes()
    return out


@functools.lru_cache(maxsize=None)
def _reference(grid, kind):
    """What _run leaves on a fresh engine that only ever had the overlay `kind` (None: never any)."""
    g, planes = _case(grid)
    vec = gua.VecGridUniverse(N, template=_spec(g), seed=SEED)
    try:
        if kind:
            OVERLAYS[kind].install(vec.engine, planes[kind])
        vec.reset()
        return _run(vec, kind, planes.get(kind))
    finally:
        vec.close()


# ---- 1: one slot, cycled: each kind behind the one before it, and boxes and errands behind and before every other tenant ----
ORDERS = {'three': (None, 'wind', None, 'fruit', None, 'doors', None),
          'four': (None, 'boxes', None, 'wind', None, 'boxes', None, 'fruit', None, 'boxes', None, 'doors', None, 'boxes', None),
          'five': (None, 'errands', None, 'fruit', None, 'errands', None, 'boxes', None, 'errands', None, 'doors', None, 'wind', None, 'errands', None)}


@pytest.mark.parametrize('grid', ['open8', 'open150'])
@pytest.mark.parametrize('order', sorted(ORDERS))
def test_one_engine_cycled_through_the_overlays_equals_engines_that_only_had_one(order, grid):
    g, planes = _case(grid)
    vec = gua.VecGridUniverse(N, template=_spec(g), seed=SEED)
    try:
        had = None
        for kind in ORDERS[order]:
            if kind:
                OVERLAYS[kind].install(vec.engine, planes[kind])
            elif had:
                OVERLAYS[had].take_away(vec.engine)
            for k in KINDS:
                assert (OVERLAYS[k].plane(vec.engine) is not None) == (k == kind), (kind, k)
            st = vec.engine.stores()
            assert st['overlay'] == (KINDS.index(kind) + 1 if kind else 0)
            vec.seed(SEED)
            vec.reset()
            got, want = _run(vec, kind, planes.get(kind)), _reference(grid, kind)
            assert got['family'] == want['family'] and (got['family'] == kind if kind else got['family'] not in KINDS)
            for k in want:
                assert got[k] == want[k], (kind, had, k)
            had = kind
        # (each overlay changed what the envs did or were paid)
        assert len({_reference(grid, k)['uniform obs'] + _reference(grid, k)['uniform reward'] for k in (None,) + KINDS}) == len(KINDS) + 1
    finally:
        vec.close()


# ---- 2: refusals leave the engine alone ----
def _snapshot(eng, kind):
    """The plane, its parameters, the masks, the Q tables and their row count, as values that compare with ==."""
    K = OVERLAYS[kind]
    masks = K.masks(eng)
    return K.plane(eng).tobytes(), K.params(eng), None if masks is None else masks.tobytes(), eng.td_get_q().tobytes(), eng.td_rows


@pytest.mark.parametrize('have', KINDS)
def test_a_refused_install_leaves_plane_masks_and_q_tables_as_they_were(have):
    g, planes = _case('open8')
    H = OVERLAYS[have]
    vec = gua.VecGridUniverse(N, template=_spec(g), seed=SEED)
    try:
        eng = vec.engine
        H.install(eng, planes[have])
        vec.reset()
        eng.td_init(0.25)
        eng.td_run(T)  # (tables that are not all q0)
        if H.state:
            H.set_masks(eng, _pattern(have, g, planes))
        before = _snapshot(eng, have)
        assert before[4] == 64 << H.bits(planes[have])
        assert before[2] is None or (np.frombuffer(before[2], np.uint32) != H.reset_value(planes[have])).any()
        for other in KINDS:
            if other == have:
                continue
            with pytest.raises(gua.GuError) as err:  # another overlay: unsupported, and the message names the one that is set
                OVERLAYS[other].install(eng, planes[other])
            assert err.value.code == -6 and have in str(err.value)
            assert code(lambda: OVERLAYS[other].take_away(eng)) == -6  # ... and so is taking that other one away
            assert OVERLAYS[other].plane(eng) is None and _snapshot(eng, have) == before
        assert code(lambda: H.install(eng, H.invalid(planes[have], g))) == -1  # an invalid plane of the same feature: its own error
        assert _snapshot(eng, have) == before
        eng.td_run(T)  # (the tables are still the engine's)
    finally:
        vec.close()


# ---- 3: a new grid drops the overlay ----
@pytest.mark.parametrize('kind', KINDS)
def test_a_new_grid_drops_the_overlay_and_its_q_rows(kind):
    g, planes = _case('open8')
    bits = OVERLAYS[kind].bits(planes[kind])
    vec = gua.VecGridUniverse(N, template=_spec(g), seed=SEED)
    try:
        eng = vec.engine
        OVERLAYS[kind].install(eng, planes[kind])
        eng.td_init(0.0)
        assert eng.td_rows == 64 << bits and eng.td_get_q(0, 2).shape == (2, 64 << bits, 4)
        eng.set_grid(_spec(g))
        assert all(OVERLAYS[k].plane(eng) is None for k in KINDS) and eng.td_rows == 64
        st = eng.stores()
        assert st['overlay'] == 0 and st['overlay_bits'] == 0
        if bits:
            assert code(lambda: eng.td_get_q(0, 2)) == -4  # (tables of S << bits rows went with the masks)
        eng.td_init(0.0)
        assert eng.td_get_q(0, 2).shape == (2, 64, 4)
        eng.look_step_ahead([0], [1])  # (refused while an overlay is set)
        vec.reset()
        vec.rollout(T, 'uniform', auto_reset=True)
        assert eng.rollout_last_form()['family'] not in KINDS
    finally:
        vec.close()


# ---- 4: reset ----
@pytest.mark.parametrize('kind', [k for k in KINDS if OVERLAYS[k].state])
def test_reset_sets_the_masks_of_exactly_the_envs_it_takes_to_the_slots_reset_value(kind):
    g, planes = _case('open8')
    K = OVERLAYS[kind]
    vec = gua.VecGridUniverse(N, template=_spec(g), seed=SEED)
    try:
        eng = vec.engine
        K.install(eng, planes[kind])
        init = K.reset_value(planes[kind])
        assert (K.masks(eng) == init).all()  # the install itself
        vec.reset()
        pattern = _pattern(kind, g, planes)
        assert (pattern != init).sum() > N // 2
        take = np.arange(N) % 3 == 0
        K.set_masks(eng, pattern)
        rb = K.reset_bits(planes[kind])  # (every bit; under errands a reset draws the instruction's index above them)

        def after(took):
            """The masks, of the envs the reset took the bits it sets alone."""
            masks = K.masks(eng)
            assert rb == 0xFFFFFFFF or len(set((masks[took] & ~np.uint32(rb)).tolist())) == 2  # (both instructions were drawn)
            return np.where(took, masks & np.uint32(rb), masks)

        vec.reset(take.astype(np.uint8))  # gu_reset under a mask of envs
        assert np.array_equal(after(take), np.where(take, init, pattern))
        K.set_masks(eng, pattern)
        done = (np.arange(N) % 5 < 2).astype(np.int32)
        vec.set_state(done=done)
        eng.reset_done()  # gu_reset_done: the done envs only
        assert np.array_equal(after(done != 0), np.where(done != 0, init, pattern))
        assert not vec.get_state()['done'].any()
        K.set_masks(eng, pattern)
        vec.reset()  # every env
        assert (after(np.ones(N, bool)) == init).all()
    finally:
        vec.close()


# ---- 5: the calls without an overlay form ----
@functools.lru_cache(maxsize=None)
def _maze11():
    """(grid dict, {kind: plane uint8[121]}): the 11 x 11 maze under the planes of the kinds' own device files; one box (7 bits) on the
    corridor that leaves the start cell 14."""
    g = GRIDS['maze11']()
    free = [s for s in range(121) if s not in set(g['walls']) | set(g['goals']) | set(g['lava'])]
    rs = np.random.RandomState(5)
    planes = dict(wind=wind_plane(11, 11, rs.randint(0, 4, (11, 11)), rs.randint(0, 4, (11, 11))),
                  fruit=fruit_plane(11, 11, [free[3], free[len(free) // 2], free[-4]], ['apple', 'lemon', 'melon']),
                  doors=door_plane(11, 11, {0: 45, 1: 23, 2: [67, 102]}, keys={0: 13, 2: 100}, levers={1: 12, 2: 34}),
                  boxes=box_plane(11, 11, [13], [12]),
                  errands=fruit_plane(11, 11, [free[3], free[len(free) // 2], free[-4]], ['apple', 'lemon', 'apple']))
    return g, planes


def _refused(call, name):
    """`call` is refused as unsupported and the message names `name`."""
    with pytest.raises(gua.GuError) as err:
        call()
    assert err.value.code == -6 and name in str(err.value), (name, str(err.value))


@pytest.mark.parametrize('kind', KINDS)
def test_calls_without_an_overlay_form_are_refused_and_a_refused_call_changes_nothing(kind):
    g, planes = _maze11()
    K, plane, others = OVERLAYS[kind], planes[kind], [k for k in KINDS if k != kind]
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
        c = no_overlay_context(g, N)
        # the tables the learners need exist before the overlay is set (the inits are not refused either way)
        vec._ensure_q()
        vec._ensure_model()
        vec._ensure_queue()
        vec._ensure_counts()
        vec._ensure_tree()
        vec._ensure_ac()
        vec._ensure_is()
        vec._ensure_pairs()
        K.install(eng, plane)
        vec._ensure_q()  # (tables of S << bits rows, and not all zero)
        vec.td_run(50, 'q_learning')
        before = _snapshot(eng, kind)
        assert before[4] == S << K.bits(plane) and np.frombuffer(before[3], np.float64).any()
        for name, call in NO_OVERLAY_CALLS.items():
            _refused(lambda: call(vec, c), kind)
        _refused(lambda: eng.rollout(8, 'uniform', True, 'packed'), kind)  # packed rows
        _refused(lambda: eng.trail_enable(16), kind)  # the trail refuses while an overlay is set
        for other in others:  # ... and so does every other kind; nothing of it stays behind
            _refused(lambda: OVERLAYS[other].install(eng, planes[other]), kind)
            assert OVERLAYS[other].plane(eng) is None
        assert _snapshot(eng, kind) == before and eng.stores()['overlay'] == KINDS.index(kind) + 1
        # what reads rows or state only is unaffected
        vec.rollout(8, 'uniform', auto_reset=True)
        eng.mc_evaluate(8, np.full(N, c.start, np.int32), 0.9 ** np.arange(8), np.ones(8, bool))
        eng.vi_get()
        vec.sense(radius=1)
        vec.get_state()
        K.take_away(eng)
        vec._ensure_tree()
        for name, call in NO_OVERLAY_CALLS.items():  # the same calls succeed once the overlay is gone
            call(vec, c)
        for other in others:  # every other kind, then this one: refused, and the tenant is named
            OVERLAYS[other].install(eng, planes[other])
            _refused(lambda: K.install(eng, plane), other)
            OVERLAYS[other].take_away(eng)
        eng.trail_enable(16)  # the trail, then this one
        _refused(lambda: K.install(eng, plane), 'trail')
        eng.trail_enable(0)
        assert all(OVERLAYS[k].plane(eng) is None for k in KINDS)  # (each refused call left the engine as it was)
        K.install(eng, plane)
        assert K.plane(eng) is not None
        eng.set_grid(_spec(g))  # a new grid drops the overlay
        assert K.plane(eng) is None and eng.stores()['overlay'] == 0
        eng.look_step_ahead([c.start], [1])
    finally:
        vec.close()
    grids = [_spec(g), _spec(g)]
    multi = gua.VecGridUniverse(N, templates=grids, seed=1)
    try:
        eng = multi.engine
        _refused(lambda: K.install(eng, plane), kind)  # an overlay is a property of a single-grid engine
        eng.set_grid(_spec(g))
        K.install(eng, plane)
        eng.set_grids(grids)  # ... and several grids drop it
        assert K.plane(eng) is None
        eng.set_grid(_spec(g))
        K.install(eng, plane)
        eng.generate_mazes(2, 11, 11, 5)  # ... as device mazes do
        assert K.plane(eng) is None
    finally:
        multi.close()
