"""The overlay tests' own scaffold (tests/_overlays.py), checked without a device: the list of calls without an overlay form is the
library's, the shared state comparison fails when one element differs, and what each registry entry says about a plane is what the
kind's CPU restatement computes from it."""
import glob
import os
import re

import numpy as np
import pytest

from . import _overlay_starts as S
from ._overlays import NO_OVERLAY_CALLS, OVERLAYS, errand_bits, masks_of, same_state

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'griduniverse_amd', 'csrc')


def test_the_refused_calls_are_the_librarys_guarded_entry_points():
    """An entry point that gains GU_NO_OVERLAY and is not added to NO_OVERLAY_CALLS (or one that loses it) fails here."""
    guarded = []
    for path in glob.glob(os.path.join(CSRC, '*.hip')):
        with open(path) as f:
            guarded += re.findall(r'GU_NO_OVERLAY\(h, "(\w+)"\)', f.read())
    assert len(guarded) == len(set(guarded)) >= 24
    assert sorted(NO_OVERLAY_CALLS) == sorted(guarded)


# ---- same_state bites ----
class _Vec(object):
    """Stands in for a batch: get_state() and the engine's get_<kind>_state() answer what the restatement holds, as copies that a test
    may spoil."""

    def __init__(self, o, kind):
        self.state = dict((k, getattr(o.state, k).copy()) for k in ('pos', 'done', 'episode', 'tcount'))
        self.masks = None if masks_of(o, kind) is None else masks_of(o, kind).copy()
        self.engine = self
        setattr(self, 'get_%s_state' % kind, lambda: self.masks)

    def get_state(self):
        return self.state


def _ran(kind):
    grid = 'one_box8' if kind == 'boxes' else 'starts8'
    o = S.oracle(kind, grid, 0)
    o.reset()
    S.rollout_of(o, grid, 'uniform', auto=False)
    assert (o.state.done != 0).any() and not (o.state.done != 0).all()
    return o


@pytest.mark.parametrize('kind', list(OVERLAYS))
def test_same_state_fails_on_one_bit_of_one_mask_and_on_one_done_flag(kind):
    o = _ran(kind)
    same_state(_Vec(o, kind), o, kind)
    for key in ('pos', 'episode', 'tcount'):
        vec = _Vec(o, kind)
        vec.state[key][-1] += 1
        with pytest.raises(AssertionError):
            same_state(vec, o, kind)
    vec = _Vec(o, kind)
    vec.state['done'][-1] = not vec.state['done'][-1]
    with pytest.raises(AssertionError):
        same_state(vec, o, kind)
    vec = _Vec(o, kind)
    vec.state['done'] = vec.state['done'] * 7  # (by truth value: the device keeps other flags than the C oracle's int32 ones)
    same_state(vec, o, kind)
    if OVERLAYS[kind].state:
        assert masks_of(o, kind).any()
        vec = _Vec(o, kind)
        vec.masks[-1] ^= 1
        with pytest.raises(AssertionError):
            same_state(vec, o, kind)


# ---- the entries against the restatements ----
def test_the_registry_names_are_the_kinds_of_the_start_cases():
    assert list(OVERLAYS) == [k for k in S.KINDS if k != 'gusts'] == [k.name for k in OVERLAYS.values()]


@pytest.mark.parametrize('grid', ['starts8', 'one_box8', 'open150'])
@pytest.mark.parametrize('kind', list(OVERLAYS))
def test_bits_reset_value_and_invalid_plane_agree_with_the_restatement(kind, grid):
    K, plane = OVERLAYS[kind], S.plane(kind, grid)
    o = K.oracle(S.c_grid(grid), 0, 3, plane, q0=None)
    assert K.bits(plane) == o._bits()
    if kind == 'errands':  # (the registry's two instructions under five fruit; the case's own three: ten bits)
        assert K.bits(plane) == 5 + 2 + 1 and S.oracle(kind, grid, 0, n=3)._bits() == errand_bits(plane, S.extra(kind, grid)[0]) == 5 + 3 + 2
    if K.state:
        assert (masks_of(o, kind) == K.reset_value(plane)).all()
        o.reset()
        assert (masks_of(o, kind) & K.reset_bits(plane) == K.reset_value(plane)).all()
        assert K.reset_bits(plane) == 0xFFFFFFFF or (kind == 'errands' and K.reset_bits(plane) == (1 << 7) - 1 and (masks_of(o, kind) >> 7).any())
    else:
        assert masks_of(o, kind) is None and K.reset_value(plane) == 0
    g = dict(S.grid_dict(grid), walls=[21, 45])
    bad = K.invalid(plane, g)
    assert bad.dtype == plane.dtype and bad.shape == plane.shape and not np.array_equal(bad, plane)
    assert np.array_equal(plane, S.plane(kind, grid))  # (the valid plane is left as it was)
