"""The overlay kinds of an engine (csrc/gu_overlay.hip; DESIGN.md "Overlays"), one entry each, for the tests that treat them alike: the
slot and refusal tests of tests/test_gpu_overlay.py, the cases of tests/_overlay_starts.py, and the kinds' own device files.  An entry
knows how to install its plane on an engine and take it away, how to read the plane, its parameters and the per-env masks back, what
a plane means for the slot (mask bits, reset value, the bits a reset sets), a plane that the kind's own validation refuses, and the
kind's CPU restatement.
Beside the table: the calls that have no overlay form, and the helpers that every kind's device file used to copy.  Nothing here needs
a device."""
import collections
import types

import numpy as np

from griduniverse_amd.grid import errand_bytes

from . import _boxes_oracle as BO
from . import _doors_oracle as DO
from . import _errands_oracle as EO
from . import _fruit_oracle as FO
from . import _wind_oracle as WO
from ._td_oracle import Q_LEARNING, SARSA

METHODS = {'q_learning': Q_LEARNING, 'sarsa': SARSA}


class Overlay(object):
    """`name` as in error messages, Engine.ROLLOUT_FAMILIES and Engine.set_<name> / get_<name> / get_<name>_state / set_<name>_state;
    `extra`: the setter's arguments behind the plane where the caller names none; `state`: the restatement's attribute that holds
    the per-env masks (None: the kind keeps none); bits(plane), reset_value(plane) and invalid(plane, grid dict) as below."""

    def __init__(self, name, extra, oracle_cls, state, bits, reset_value, invalid):
        self.name, self.extra, self.oracle_cls, self.state = name, extra, oracle_cls, state
        self.bits, self.reset_value, self.invalid = bits, reset_value, invalid

    def install(self, eng, plane, *extra):
        getattr(eng, 'set_' + self.name)(plane, *(extra or self.extra))

    def take_away(self, eng):
        getattr(eng, 'set_' + self.name)(None)

    def _got(self, eng):
        got = getattr(eng, 'get_' + self.name)()
        return got if got is None or isinstance(got, tuple) else (got,)

    def plane(self, eng):
        """uint8[S], or None while the engine has no overlay of this kind."""
        got = self._got(eng)
        return None if got is None else got[0]

    def params(self, eng):
        """What get_<name> answers beside the plane (the gust probability, the fruit values, the boxes' pay, count and width)."""
        return tuple(np.asarray(x).tolist() for x in self._got(eng)[1:])

    def masks(self, eng):
        return getattr(eng, 'get_%s_state' % self.name)() if self.state else None

    def set_masks(self, eng, masks):
        getattr(eng, 'set_%s_state' % self.name)(masks)

    def oracle(self, grid, seed, n, plane, *extra, **kw):
        return self.oracle_cls(grid, seed, n, plane, *(extra or self.extra), **kw)

    def masks_of(self, o):
        return getattr(o, self.state) if self.state else None

    def reset_bits(self, plane):
        """The bits of a mask that a reset sets to reset_value(plane): all of them."""
        return 0xFFFFFFFF


class Errands(Overlay):
    """`extra` is (instructions, pay) as the restatement takes them; the engine takes the instruction bytes, their count and the pay.
    A reset clears the eaten bits and the progress and DRAWS the instruction's index above them (stream 11: tests/test_gpu_errands.py
    holds the draw against the restatement); the install leaves index 0 in every word."""

    def install(self, eng, plane, *extra):
        instructions, pay = extra or self.extra
        eng.set_errands(plane, errand_bytes([list(i) for i in instructions]), len(instructions), np.array(pay, np.int32))

    def reset_bits(self, plane):
        return (1 << (self.bits(plane) - (len(self.extra[0]) - 1).bit_length())) - 1


def errand_bits(plane, instructions):
    """F + pb + ib: a bit per fruit, the progress 0 .. the longest list, the instruction's index."""
    return int(np.count_nonzero(plane)) + max(len(i) for i in instructions).bit_length() + (len(instructions) - 1).bit_length()


def _with(plane, cell, byte, clear=False):
    p = np.zeros_like(plane) if clear else plane.copy()
    p[cell] = byte
    return p


def _box_bits(plane):
    return max(1, int(plane.size - 1).bit_length())


def _box_word(plane):
    return sum(int(s) << (k * _box_bits(plane)) for k, s in enumerate(np.flatnonzero(plane & BO.INITIAL)))


OVERLAYS = collections.OrderedDict((k.name, k) for k in (  # in the order of stores()['overlay']: 1 wind, 2 fruit, 3 doors, 4 boxes, 5 errands
    Overlay('wind', (WO.GUST_THIRDS,), WO.WindOracle, None, bits=lambda p: 0, reset_value=lambda p: 0,
            invalid=lambda p, g: _with(p, 5, 0x80)),  # a wind byte with a high bit
    Overlay('fruit', ((1, 5, -5),), FO.FruitOracle, 'eaten', bits=lambda p: int(np.count_nonzero(p)), reset_value=lambda p: 0,
            invalid=lambda p, g: _with(p, g['walls'][0], (1 << 5) | 4)),  # fruit on a wall
    Overlay('doors', (), DO.DoorsOracle, 'open', bits=lambda p: len(set((p[p != 0] & 7).tolist())), reset_value=lambda p: 0,
            invalid=lambda p, g: _with(p, 20, DO.DOOR << 4, clear=True)),  # a door of slot 0 and no key or lever for it
    Overlay('boxes', (5,), BO.BoxesOracle, 'words', bits=lambda p: _box_bits(p) * int(np.count_nonzero(p & BO.INITIAL)), reset_value=_box_word,
            invalid=lambda p, g: _with(p, g['walls'][0], BO.TARGET)),  # a target on a wall
    # (two instructions that every plane with two apples and a lemon can carry out; bits = F + pb + ib under them)
    Errands('errands', (EO.TD_INSTRUCTIONS, EO.CASE_PAY), EO.ErrandsOracle, 'words', bits=lambda p: errand_bits(p, EO.TD_INSTRUCTIONS),
            reset_value=lambda p: 0, invalid=lambda p, g: _with(p, g['walls'][0], (1 << 5) | int(np.count_nonzero(p)))),  # a fruit (the next slot) on a wall
))


def overlay(kind):
    """The entry of `kind`; 'gusts' (tests/_overlay_starts.py) is wind with a gust probability: the same entry."""
    return OVERLAYS['wind' if kind == 'gusts' else kind]


def masks_of(o, kind):
    """The per-env overlay state of a restatement: eaten masks, open masks, box words, errand words; None under wind."""
    return overlay(kind).masks_of(o)


# ---- the entry points without an overlay form: one per GU_NO_OVERLAY(h, "...") of csrc/*.hip (tests/test_overlay_registry_host.py
# reads them out of the sources), each as a call of a batch `vec` that is refused with GU_ERR_UNSUPPORTED while an overlay is set and
# succeeds without one.  `c`: no_overlay_context ----
NO_OVERLAY_CALLS = {
    'gu_step_graph': lambda vec, c: vec.engine.step_graph(0, 4),
    'gu_dyna_run': lambda vec, c: vec.dyna_run(5, planning_steps=2),
    'gu_sweep_run': lambda vec, c: vec.sweep_run(5),
    'gu_search_run': lambda vec, c: vec.search_run(3, simulations=1, depth=2),
    'gu_explore_run': lambda vec, c: vec.explore_run(5),
    'gu_mcts_run': lambda vec, c: vec.tree_search_run(3, simulations=1, tree_depth=2, depth=2),  # (one simulation: the pool _ensure_tree made)
    'gu_nstep_run': lambda vec, c: vec.nstep_run(5),
    'gu_lambda_run': lambda vec, c: vec.lambda_run(5),
    'gu_esarsa_run': lambda vec, c: vec.expected_sarsa_run(5),
    'gu_double_run': lambda vec, c: vec.double_q_run(5),
    'gu_ac_run': lambda vec, c: vec.actor_critic_run(5),
    'gu_reinforce_run': lambda vec, c: vec.reinforce_run(5),
    'gu_is_run': lambda vec, c: vec.off_policy_mc_run(5),
    'gu_fa_run': lambda vec, c: vec.fa_run(5),
    'gu_look_step_ahead': lambda vec, c: vec.engine.look_step_ahead([c.start], [1]),
    'gu_vi_sweep': lambda vec, c: vec.engine.vi_sweep(0.9, 1),
    'gu_vi_run': lambda vec, c: vec.engine.vi_run(0.9, 1e-3, 3),
    'gu_vi_eval_run': lambda vec, c: vec.engine.vi_eval_run(0.9, 1e-3, 3),
    'gu_vi_greedy': lambda vec, c: vec.engine.vi_greedy(0.9),
    'gu_vi_sweep_step': lambda vec, c: vec.engine.vi_sweep_step(0.9),
    'gu_vi_sweep_step_run': lambda vec, c: vec.engine.vi_sweep_step_run(0.9, 2),
    'gu_mc_walk_lengths': lambda vec, c: vec.engine.mc_walk_lengths(c.u, 8, [c.start], 16, c.cdf),
    'gu_mc_walk_episodes': lambda vec, c: vec.engine.mc_walk_episodes(c.u, c.cdf, np.zeros(c.N, np.int64), np.full(c.N, c.start, np.int32), 16, 8),
    'gu_shortest_paths': lambda vec, c: vec.engine.shortest_paths(),
}


def no_overlay_context(g, N):
    """What NO_OVERLAY_CALLS take beside the batch of N envs on grid dict g: uniform draws, a uniform policy's CDF, the start cell."""
    S = g['W'] * g['H']
    cdf = np.tile(np.array([0.25, 0.5, 0.75, 1.0]), (S, 1))
    return types.SimpleNamespace(N=N, start=g['starts'][0], u=np.random.RandomState(0).rand(256), cdf=cdf)


# ---- what the kinds' device files share ----
def scatter(g, N):
    """N cells of the grid that are neither wall nor terminal: where the tests put the envs, so that a batch with one start cell
    (and a deterministic policy) still walks the whole grid."""
    taken = set(g['walls']) | set(g['goals']) | set(g['lava'])
    free = np.array([s for s in range(g['W'] * g['H']) if s not in taken], np.int32)
    return free[np.random.RandomState(N).randint(0, len(free), N)]


def same_state(vec, o, kind):
    """The batch's env state and per-env masks against the restatement's (`done` by truth value: the restatement keeps the C
    oracle's int32 flags)."""
    st = vec.get_state()
    assert np.array_equal(st['pos'], o.state.pos) and np.array_equal(st['done'] != 0, o.state.done != 0)
    assert np.array_equal(st['episode'], o.state.episode) and np.array_equal(st['tcount'], o.state.tcount)
    masks = overlay(kind).masks(vec.engine)
    assert masks is None or np.array_equal(masks, masks_of(o, kind))


def policy_table(S):
    pi = np.random.RandomState(1).dirichlet(np.ones(4), S)
    pi[::7] = np.eye(4)[np.arange(len(pi[::7])) % 4]  # one-hot rows: thresholds that no word reaches
    return pi
