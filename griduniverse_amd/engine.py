"""Engine: numpy-facing wrapper of one libgu handle (one device, one HIP stream).

Thin by design -- every method is one C-ABI call (include/gu.h) plus array
marshalling; all grid / argument semantics of the reference live in
`griduniverse_amd.envs` (host Python) and in the kernels (device).
"""
import ctypes

import numpy as np

from . import _lib
from ._lib import check, ptr
from .grid import GridSpec, check_sense_args

_POLICIES = {'uniform': _lib.POLICY_UNIFORM, 'stream': _lib.POLICY_STREAM, 'greedy': _lib.POLICY_GREEDY,
             'sample': _lib.POLICY_SAMPLE}
_EXPLORE_RULES = {'ucb': _lib.EXPLORE_UCB, 'thompson': _lib.EXPLORE_THOMPSON, 0: _lib.EXPLORE_UCB, 1: _lib.EXPLORE_THOMPSON}
_TD_METHODS = {'q_learning': _lib.TD_Q_LEARNING, 'sarsa': _lib.TD_SARSA, 0: _lib.TD_Q_LEARNING, 1: _lib.TD_SARSA}


def _learner_flags(trajectory, stats):
    """The flags of a tabular learner launch (gu_td_run, gu_dyna_run, gu_nstep_run, gu_ac_run): rows and statistics only."""
    return (_lib.F_TRAJECTORY if trajectory else 0) | (_lib.F_STATS if stats else 0)


def _tables(x, row, name, dtype=np.float64):
    """`x` as a contiguous `dtype` array [n, *row]; an array of shape `row` is the table of one env."""
    x = np.asarray(x, dtype)
    x = _lib.as_array(x.reshape((-1,) + row) if x.ndim == len(row) else x, dtype, None, name)
    if x.ndim != len(row) + 1 or x.shape[1:] != row:
        raise ValueError('{} must have shape (n, {}), got {}'.format(name, ', '.join(str(k) for k in row), x.shape))
    return x


class Engine(object):
    def __init__(self, num_envs, spec, device=0, env_id0=0, seed=0):
        if not isinstance(spec, GridSpec):
            raise TypeError('spec must be a GridSpec')
        self._h = ctypes.c_void_p()
        self.lib = _lib.load()
        self.N = int(num_envs)
        self.env_id0 = int(env_id0)
        self.device = int(device)
        check(self.lib.gu_create(self.device, self.N, self.env_id0, ctypes.byref(self._h)))
        self.spec = None
        self._pinned = {}
        self._pinned_io = None
        try:
            self.set_grid(spec)
            self.seed(seed)
        except Exception:
            self.close()
            raise

    # ------------------------------------------------------------------ lifetime
    def close(self):
        for p in getattr(self, '_pinned', {}).values():
            p.free()
        self._pinned = {}
        self._pinned_io = None
        if getattr(self, '_h', None) is not None and self._h.value:
            self.lib.gu_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001  (interpreter shutdown)
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @staticmethod
    def device_info(device=0):
        """dict: name, arch, pci, cus, lds_per_cu, sclk_khz, mclk_khz, bus_bits, l2_bytes, hbm_bytes, hbm_free (gu_device_info)."""
        return _lib.device_info(device)

    # ------------------------------------------------------------------ options
    def set_option(self, name, value):
        """Launch-shape / search option of THIS engine (include/gu.h "options"; `_lib.OPTIONS` names them); None returns
        it to the process default.  Results never depend on options."""
        check(self.lib.gu_set_option(self._h, _lib.OPTIONS[name], _lib.OPT_UNSET if value is None else int(value)))

    def get_option(self, name):
        v = ctypes.c_int64(0)
        check(self.lib.gu_get_option(self._h, _lib.OPTIONS[name], ctypes.byref(v)))
        return v.value

    # ------------------------------------------------------------------ configuration
    def set_grid(self, spec):
        p = spec.planes()
        starts = np.asarray(spec.starts, dtype=np.int32)
        check(self.lib.gu_set_grid(self._h, spec.W, spec.H, spec.words_per_row, ptr(p['wall']), ptr(p['goal']),
                                   ptr(p['lava']), ptr(p['rplus']), ptr(p['rminus']), ptr(starts), len(starts)))
        self.spec = spec

    def set_grids(self, specs):
        """Several distinct grids of one shape: env e uses specs[e // (N // len(specs))]."""
        G = len(specs)
        W, H = specs[0].W, specs[0].H
        if any((sp.W, sp.H) != (W, H) for sp in specs):
            raise ValueError('all grids of one engine must have the same shape')
        planes = [sp.planes() for sp in specs]
        stack = {k: np.ascontiguousarray(np.stack([p[k] for p in planes])) for k in planes[0]}
        max_starts = max(len(sp.starts) for sp in specs)
        starts = np.zeros((G, max_starts), np.int32)
        n_starts = np.zeros(G, np.int32)
        for g, sp in enumerate(specs):
            starts[g, :len(sp.starts)] = sp.starts
            n_starts[g] = len(sp.starts)
        check(self.lib.gu_set_grids(self._h, G, W, H, specs[0].words_per_row, ptr(stack['wall']), ptr(stack['goal']),
                                    ptr(stack['lava']), ptr(stack['rplus']), ptr(stack['rminus']), ptr(starts),
                                    ptr(n_starts), max_starts))
        self.spec = specs[0]
        self.specs = list(specs)

    def generate_mazes(self, n_grids, W, H, maze_seed):
        """n_grids random mazes carved on the device (one per env group of N // n_grids envs)."""
        check(self.lib.gu_generate_mazes(self._h, int(n_grids), int(W), int(H), int(maze_seed) & 0xFFFFFFFFFFFFFFFF))
        self.spec = GridSpec(W, H, [0], [W * H - 1], [], [])  # shape holder; the real grids live on the device
        self.specs = None

    def get_cells(self, grid_index=0):
        """(flags uint8[S], reward int8[S], starts int32[n]) of one grid as compiled on the device."""
        S = self.spec.S
        flags, reward = np.empty(S, np.uint8), np.empty(S, np.int8)
        n = ctypes.c_int32(0)
        check(self.lib.gu_get_cells(self._h, int(grid_index), None, None, None, ctypes.byref(n)))
        starts = np.empty(max(n.value, 1), np.int32)  # a start list may repeat cells and be longer than the grid
        check(self.lib.gu_get_cells(self._h, int(grid_index), ptr(flags), ptr(reward), ptr(starts), ctypes.byref(n)))
        return flags, reward, starts[:n.value].copy()

    def set_wind(self, wind, gust_q16=0):
        """Install the wind plane uint8[S] (grid.wind_plane) and the gust probability in 1/65536; None calms the engine again
        (gu_set_wind)."""
        w = None if wind is None else _lib.as_array(wind, np.uint8, (self.spec.S,), 'wind')
        check(self.lib.gu_set_wind(self._h, ptr(w), int(gust_q16)))

    def get_wind(self):
        """(wind uint8[S], gust_q16), or None while the engine is calm (gu_get_wind)."""
        wind = np.empty(self.spec.S, np.uint8)
        gust, present = ctypes.c_uint32(0), ctypes.c_int32(0)
        check(self.lib.gu_get_wind(self._h, ptr(wind), ctypes.byref(gust), ctypes.byref(present)))
        return (wind, gust.value) if present.value else None

    def set_fruit(self, fruit, values=(0, 0, 0)):
        """Install the fruit plane uint8[S] (grid.fruit_plane) and the three kinds' values (each -16 .. 16); None takes the fruit
        away again (gu_set_fruit).  Clears every env's mask of eaten fruit."""
        f = None if fruit is None else _lib.as_array(fruit, np.uint8, (self.spec.S,), 'fruit')
        v = _lib.as_array(values, np.int32, (3,), 'values')
        check(self.lib.gu_set_fruit(self._h, ptr(f), ptr(v)))

    def get_fruit(self):
        """(fruit uint8[S], values int32[3]), or None while no fruit is set (gu_get_fruit)."""
        fruit, values = np.empty(self.spec.S, np.uint8), np.empty(3, np.int32)
        n = ctypes.c_int32(0)
        check(self.lib.gu_get_fruit(self._h, ptr(fruit), ptr(values), ctypes.byref(n)))
        return (fruit, values) if n.value else None

    def _get_masks(self, getter, env0, n):
        env0, n, n0 = self._env_range(env0, n)
        masks = np.empty(n0, np.uint32)
        check(getter(self._h, env0, n, ptr(masks)))
        return masks

    def _set_masks(self, setter, masks, env0, name):
        m = _lib.as_array(masks, np.uint32, None, name)
        check(setter(self._h, int(env0), m.size, ptr(m)))

    def get_fruit_state(self, env0=0, n=None):
        """uint32[n]: the masks of eaten fruit (bit = slot) of envs env0 .. env0+n-1 (gu_get_fruit_state)."""
        return self._get_masks(self.lib.gu_get_fruit_state, env0, n)

    def set_fruit_state(self, eaten, env0=0):
        """Install the masks uint32[n] of envs env0 .. env0+n-1 (gu_set_fruit_state)."""
        self._set_masks(self.lib.gu_set_fruit_state, eaten, env0, 'eaten')

    def set_doors(self, door):
        """Install the door plane uint8[S] (grid.door_plane); None takes the doors away again (gu_set_doors).  Clears every env's
        mask of open slots."""
        d = None if door is None else _lib.as_array(door, np.uint8, (self.spec.S,), 'door')
        check(self.lib.gu_set_doors(self._h, ptr(d)))

    def get_doors(self):
        """door uint8[S], or None while no doors are set (gu_get_doors)."""
        door = np.empty(self.spec.S, np.uint8)
        n = ctypes.c_int32(0)
        check(self.lib.gu_get_doors(self._h, ptr(door), ctypes.byref(n)))
        return door if n.value else None

    def get_doors_state(self, env0=0, n=None):
        """uint32[n]: the masks of open slots (bit = slot) of envs env0 .. env0+n-1 (gu_get_doors_state)."""
        return self._get_masks(self.lib.gu_get_doors_state, env0, n)

    def set_doors_state(self, mask, env0=0):
        """Install the masks uint32[n] of envs env0 .. env0+n-1 (gu_set_doors_state)."""
        self._set_masks(self.lib.gu_set_doors_state, mask, env0, 'mask')

    def set_boxes(self, box, on_target=0):
        """Install the box plane uint8[S] (grid.box_plane) and what a box pushed onto a target pays (0 .. 16); None takes the boxes
        away again (gu_set_boxes).  Sets every env's word to the initial boxes' cells."""
        b = None if box is None else _lib.as_array(box, np.uint8, (self.spec.S,), 'box')
        check(self.lib.gu_set_boxes(self._h, ptr(b), int(on_target)))

    def get_boxes(self):
        """(box uint8[S], on_target, B, b): the plane, the pay, the number of boxes and the bits of one box's cell in an env's word,
        or None while no boxes are set (gu_get_boxes)."""
        box = np.empty(self.spec.S, np.uint8)
        v, n, b = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0)
        check(self.lib.gu_get_boxes(self._h, ptr(box), ctypes.byref(v), ctypes.byref(n), ctypes.byref(b)))
        return (box, v.value, n.value, b.value) if n.value else None

    def get_boxes_state(self, env0=0, n=None):
        """uint32[n]: the words of envs env0 .. env0+n-1, box k's cell in bits [k * b, (k + 1) * b) (gu_get_boxes_state)."""
        return self._get_masks(self.lib.gu_get_boxes_state, env0, n)

    def set_boxes_state(self, words, env0=0):
        """Install the words uint32[n] of envs env0 .. env0+n-1 (gu_set_boxes_state)."""
        self._set_masks(self.lib.gu_set_boxes_state, words, env0, 'words')

    def set_errands(self, errand, instr=(0, 0, 0, 0), n_instr=0, pay=(0, 0, 0)):
        """Install the errand plane uint8[S] (grid.fruit_plane), the instruction bytes uint8[4] (grid.errand_bytes) of which the first
        `n_instr` count, and the pay (right 0 .. 16, wrong -16 .. 0, finish 0 .. 16); None takes the errands away again
        (gu_set_errands).  Sets every env's word to 0: instruction 0, nothing eaten."""
        p = None if errand is None else _lib.as_array(errand, np.uint8, (self.spec.S,), 'errand')
        i = _lib.as_array(instr, np.uint8, (4,), 'instr')
        v = _lib.as_array(pay, np.int32, (3,), 'pay')
        check(self.lib.gu_set_errands(self._h, ptr(p), int(n_instr), ptr(i), ptr(v)))

    def get_errands(self):
        """(errand uint8[S], instr uint8[4], n_instr, pay int32[3], F), or None while no errands are set (gu_get_errands)."""
        errand, instr, pay = np.empty(self.spec.S, np.uint8), np.empty(4, np.uint8), np.empty(3, np.int32)
        n, F = ctypes.c_int32(0), ctypes.c_int32(0)
        check(self.lib.gu_get_errands(self._h, ptr(errand), ctypes.byref(n), ptr(instr), ptr(pay), ctypes.byref(F)))
        return (errand, instr, n.value, pay, F.value) if n.value else None

    def get_errands_state(self, env0=0, n=None):
        """uint32[n]: the words of envs env0 .. env0+n-1, eaten | progress << F | instruction << (F + pb) (gu_get_errands_state)."""
        return self._get_masks(self.lib.gu_get_errands_state, env0, n)

    def set_errands_state(self, words, env0=0):
        """Install the words uint32[n] of envs env0 .. env0+n-1 (gu_set_errands_state)."""
        self._set_masks(self.lib.gu_set_errands_state, words, env0, 'words')

    @property
    def td_rows(self):
        """Rows of one env's Q table: S, or S << F while F fruits are set (include/gu.h: gu_set_fruit), or S << D while doors with
        D slots are set (gu_set_doors), or S << (b * B) while B boxes of b bits each are set (gu_set_boxes), or
        S << (F + pb + ib) while errands are set (gu_set_errands)."""
        return self.spec.S << self.stores()['overlay_bits']

    def seed(self, seed):
        self.seed_value = int(seed) & 0xFFFFFFFFFFFFFFFF
        check(self.lib.gu_seed(self._h, self.seed_value))

    # ------------------------------------------------------------------ reset / step
    def reset(self, mask=None, start_choice=None):
        m = None if mask is None else _lib.as_array(np.asarray(mask).astype(bool), np.uint8, (self.N,), 'mask')
        c = None if start_choice is None else _lib.as_array(start_choice, np.int32, (self.N,), 'start_choice')
        obs = np.empty(self.N, np.int32)
        check(self.lib.gu_reset(self._h, ptr(m), ptr(c), ptr(obs)))
        return obs

    def reset_done(self):
        check(self.lib.gu_reset_done(self._h))

    def step(self, actions, auto_reset=False):
        a = _lib.as_array(actions, np.int32, (self.N,), 'actions')
        obs, rew, don = (np.empty(self.N, np.int32) for _ in range(3))
        check(self.lib.gu_step(self._h, ptr(a), _lib.F_AUTO_RESET if auto_reset else 0, ptr(obs), ptr(rew), ptr(don)))
        return obs, rew, don

    def _pin(self, key, shape, dtype=np.int32):
        p = self._pinned.get(key)
        if p is None or p.array.shape != tuple(shape):
            self._pinned_io = None
            if p is not None:
                p.free()
            p = self._pinned[key] = _lib.PinnedArray(tuple(shape), dtype)
        return p.array

    @property
    def pinned_actions(self):
        """int32[N] page-locked action buffer: fill it in place, then call step_pinned()."""
        return self._pin('act', (self.N,))

    def step_pinned(self, auto_reset=False):
        """gu_step on the engine's page-locked buffers (no bounce copies).  Returns views that stay
        valid -- and are overwritten -- until the next step_pinned()."""
        io = self._pinned_io
        if io is None:  # views and their C pointers are built once: per call they would cost more than the launch
            a, out = self.pinned_actions, self._pin('out', (3, self.N))
            io = self._pinned_io = ((ptr(a), ptr(out[0]), ptr(out[1]), ptr(out[2])), (out[0], out[1], out[2]))
        flags = (_lib.F_AUTO_RESET if auto_reset else 0) | _lib.F_PINNED_IO
        p = io[0]
        rc = self.lib.gu_step(self._h, p[0], flags, p[1], p[2], p[3])
        if rc:
            check(rc)
        return io[1]

    def upload_actions(self, actions):
        a = np.ascontiguousarray(actions, dtype=np.int32)
        if a.ndim != 2 or a.shape[1] != self.N:
            raise ValueError('actions must have shape (T, {}), got {}'.format(self.N, a.shape))
        check(self.lib.gu_upload_actions(self._h, ptr(a), a.shape[0]))

    def step_device(self, t, auto_reset=False):
        check(self.lib.gu_step_device(self._h, int(t), _lib.F_AUTO_RESET if auto_reset else 0))

    def step_graph(self, t0, T, auto_reset=False):
        check(self.lib.gu_step_graph(self._h, int(t0), int(T), _lib.F_AUTO_RESET if auto_reset else 0))

    def read_outputs(self):
        obs, rew, don = (np.empty(self.N, np.int32) for _ in range(3))
        check(self.lib.gu_read_outputs(self._h, ptr(obs), ptr(rew), ptr(don)))
        return obs, rew, don

    # ------------------------------------------------------------------ rollout
    def reserve_trajectory(self, T):
        check(self.lib.gu_reserve_trajectory(self._h, int(T)))

    def trajectory_placement(self):
        """(candidate allocations tried, probe ms of the kept one, probe ms of the slowest) of the trajectory buffer."""
        n, best, worst = ctypes.c_int32(0), ctypes.c_float(0.0), ctypes.c_float(0.0)
        check(self.lib.gu_trajectory_placement(self._h, ctypes.byref(n), ctypes.byref(best), ctypes.byref(worst)))
        return n.value, best.value, worst.value

    def trajectory_placement_detail(self):
        """Everything the placement search of the trajectory buffer tried: dict(probe_ms=[...], address=[...], kept=index,
        search_ms=wall time of the search, peak_bytes=most device memory it held at once)."""
        n, kept = ctypes.c_int32(0), ctypes.c_int32(-1)
        search, peak = ctypes.c_float(0.0), ctypes.c_uint64(0)
        check(self.lib.gu_trajectory_placement_detail(self._h, 0, None, None, ctypes.byref(n), ctypes.byref(kept),
                                                      ctypes.byref(search), ctypes.byref(peak)))
        ms, addr = np.zeros(max(n.value, 1), np.float32), np.zeros(max(n.value, 1), np.uint64)
        check(self.lib.gu_trajectory_placement_detail(self._h, ms.size, ptr(ms), ptr(addr), ctypes.byref(n), None, None, None))
        return dict(probe_ms=[float(x) for x in ms[:n.value]], address=['0x%x' % int(a) for a in addr[:n.value]],
                    kept=kept.value, search_ms=float(search.value), peak_bytes=int(peak.value))

    def probe_trajectory(self):
        """ms of one full write of the trajectory buffer the engine holds, in the rollout's store shape (overwrites it)."""
        ms = ctypes.c_float(0.0)
        check(self.lib.gu_probe_trajectory(self._h, ctypes.byref(ms)))
        return ms.value

    def rollout(self, T, policy='uniform', auto_reset=True, trajectory=True, stats=False):
        """trajectory: False / True (three int32 rows per step) / 'packed' (one uint32 per env-step)."""
        tflag = _lib.F_PACKED if trajectory == 'packed' else (_lib.F_TRAJECTORY if trajectory else 0)
        flags = (_lib.F_AUTO_RESET if auto_reset else 0) | tflag | (_lib.F_STATS if stats else 0)
        check(self.lib.gu_rollout(self._h, int(T), _POLICIES[policy], flags))

    ROLLOUT_FORM = ('family', 'layout', 'map', 'block', 'workgroups', 'lds_bytes', 'flags', 'K', 'row_shift', 'stream_words', 'pace_slot', 'pace_mode')
    ROLLOUT_FAMILIES = {0: None, 1: 'general', 2: 'rows', 3: 'kstep', 4: 'wind', 5: 'fruit', 6: 'doors', 7: 'boxes', 8: 'errands'}
    ROLLOUT_FLAG_BITS = ('pair', 'half', 'per_wave', 'pi_lds', 'straddle', 'entry_table', 'xcd_remap')

    def rollout_last_form(self):
        """What the last rollout of this engine ran on (gu_diag_rollout_form): dict with the twelve form words under the names of
        ROLLOUT_FORM ('family' as a name: 'general', 'rows', 'kstep', 'wind', 'fruit', 'doors', 'boxes', 'errands'; None before the first rollout), each flag bit as a
        bool under its name in ROLLOUT_FLAG_BITS, and the raw words as 'words'."""
        words = np.zeros(len(self.ROLLOUT_FORM), np.int32)
        n = ctypes.c_int32(0)
        check(self.lib.gu_diag_rollout_form(self._h, ptr(words), words.size, ctypes.byref(n)))
        out = dict(zip(self.ROLLOUT_FORM, (int(w) for w in words)))
        out.update((name, bool(out['flags'] >> bit & 1)) for bit, name in enumerate(self.ROLLOUT_FLAG_BITS))
        out['family'] = self.ROLLOUT_FAMILIES[out['family']]
        out['words'] = [int(w) for w in words]
        return out

    def calibrate_rollout(self, T, policy='uniform', auto_reset=True, trajectory=True, stats=False):
        """= rollout(...).  Rounds 3 and 4 searched the store-pacing period here; the launches choose it themselves now
        (include/gu.h: gu_rollout_calibrate), so nothing is left to ask for."""
        flags = (_lib.F_AUTO_RESET if auto_reset else 0) | (_lib.F_STATS if stats else 0)
        flags |= _lib.F_PACKED if trajectory == 'packed' else (_lib.F_TRAJECTORY if trajectory else 0)
        check(self.lib.gu_rollout_calibrate(self._h, int(T), _POLICIES[policy], flags))

    def rollout_pacing_totals(self):
        """Over all launch kinds of this engine: dict(calibration_ms, launches_spent, kinds_paced, kinds_from_cache, kinds_waiting) --
        calibration_ms and launches_spent are 0: no launch is ever spent on a search."""
        ms = ctypes.c_float(0.0)
        n = [ctypes.c_int32(0) for _ in range(4)]
        check(self.lib.gu_rollout_pacing_totals(self._h, ctypes.byref(ms), *[ctypes.byref(x) for x in n]))
        return dict(calibration_ms=ms.value, launches_spent=n[0].value, kinds_paced=n[1].value, kinds_from_cache=n[2].value, kinds_waiting=n[3].value)

    def rollout_pacing(self, policy='uniform', auto_reset=True, packed=False):
        """The schedule of this launch kind on the current trajectory buffer (include/gu.h: gu_rollout_pacing): dict(period = 10 ns
        ticks per 16 steps of its last launch, ms_paced = that launch on the device's clock, evaluated = launches of the kind so
        far; ms_unpaced and calibration_ms are 0), or None when the kind keeps no schedule (not launched yet, or too small)."""
        period, n = ctypes.c_int32(0), ctypes.c_int32(0)
        a, b, c = ctypes.c_float(0.0), ctypes.c_float(0.0), ctypes.c_float(0.0)
        rc = self.lib.gu_rollout_pacing(self._h, _POLICIES[policy], (_lib.F_AUTO_RESET if auto_reset else 0) | (_lib.F_PACKED if packed else 0), ctypes.byref(period),
                                        ctypes.byref(a), ctypes.byref(b), ctypes.byref(n), ctypes.byref(c))
        if rc == -4:
            return None
        check(rc)
        return dict(period=period.value, ms_unpaced=a.value, ms_paced=b.value, evaluated=n.value, calibration_ms=c.value)

    def rollout_pace_log(self, policy='uniform', auto_reset=True, packed=False):
        """The records of the last (at most 61) launches of this kind, oldest first, as a dict of arrays: seq, period (ticks, float;
        0 = the launch ran without the limiter), verdict (of the launch behind it: 0 none yet, 1 on schedule, 2 behind), phase (0
        limiter on, 1 probing without it, 2 limiter off, 3 probing with it), waves, elapsed (ticks from start to report, slowest
        wave), ended_late (waves), max_behind (ticks), interval (ticks to the next launch's start; 0 for the last); plus 'launches'
        (of the kind on the current shape).  None when the kind keeps no schedule."""
        buf = np.zeros((61, 8), dtype=np.uint64)
        n, launches = ctypes.c_int32(0), ctypes.c_uint32(0)
        rc = self.lib.gu_rollout_pace_log(self._h, _POLICIES[policy], (_lib.F_AUTO_RESET if auto_reset else 0) | (_lib.F_PACKED if packed else 0), 61,
                                          buf.ctypes.data, ctypes.byref(n), ctypes.byref(launches))
        if rc == -4:
            return None
        check(rc)
        e = buf[:n.value].astype(np.int64)
        return dict(seq=e[:, 0], period=e[:, 1] / 64.0, verdict=e[:, 2] & 0xFF, phase=(e[:, 2] >> 8) & 0xFF, dec_q=e[:, 2] >> 16, waves=e[:, 3], elapsed=e[:, 4],
                    ended_late=e[:, 5], max_behind=e[:, 6], interval=e[:, 7], launches=launches.value)

    def rollout_pace_waves(self, policy='uniform', auto_reset=True, packed=False):
        """MEASUREMENT AID: what every wave of this kind's last launch reported: int64[waves] ticks (10 ns) from the wave's start to
        its report a few groups before the end of the launch (0 = did not report).  None when the kind keeps no schedule."""
        cap = (self.N + 31) // 32  # (the most a launch can have: the transition-row kernel's half waves)
        buf = np.zeros(cap, dtype=np.uint32)
        n = ctypes.c_int32(0)
        rc = self.lib.gu_rollout_pace_waves(self._h, _POLICIES[policy], (_lib.F_AUTO_RESET if auto_reset else 0) | (_lib.F_PACKED if packed else 0), cap,
                                            buf.ctypes.data, ctypes.byref(n))
        if rc == -4:
            return None
        check(rc)
        return buf[:n.value].astype(np.int64)

    def read_trajectory(self, t0, T, pinned=False):
        """Rows t0..t0+T-1 of the trajectory as obs/reward/done int32[T, N].  pinned=True returns views of
        page-locked buffers owned by the engine (full PCIe rate; overwritten by the next pinned read)."""
        if pinned:
            buf = self._pin('traj', (3, T, self.N))
            obs, rew, don = buf[0], buf[1], buf[2]
        else:
            obs, rew, don = (np.empty((T, self.N), np.int32) for _ in range(3))
        check(self.lib.gu_read_trajectory(self._h, int(t0), int(T), ptr(obs), ptr(rew), ptr(don)))
        return dict(obs=obs, reward=rew, done=don)

    def read_trajectory_packed(self, t0, T, unpack=True, pinned=False):
        """After rollout(trajectory='packed'): uint32[T, N] words obs | (reward & 0xFF) << 16 | done << 24, or --
        unpack=True -- the same dict of int32 arrays read_trajectory returns."""
        words = self._pin('trajp', (T, self.N), np.uint32) if pinned else np.empty((T, self.N), np.uint32)
        check(self.lib.gu_read_trajectory_packed(self._h, int(t0), int(T), ptr(words)))
        if not unpack:
            return words
        return dict(obs=(words & 0xFFFF).astype(np.int32), reward=((words >> 16) & 0xFF).astype(np.int8).astype(np.int32),
                    done=((words >> 24) & 1).astype(np.int32))

    def read_stats(self):
        ret = np.empty(self.N, np.int64)
        eps = np.empty(self.N, np.int32)
        check(self.lib.gu_read_stats(self._h, ptr(ret), ptr(eps)))
        return ret, eps

    def _env_range(self, env0, n):
        """env0 and n as the library takes them (n None: all from env0), and the rows of the result."""
        env0 = int(env0)
        n = self.N - env0 if n is None else int(n)
        return env0, n, max(n, 0)

    # ------------------------------------------------------------------ tabular TD control (include/gu.h: gu_td_*)
    def td_init(self, q0=0.0):
        """One float64 Q table [S][4] per env, every entry q0."""
        check(self.lib.gu_td_init(self._h, float(q0)))

    def td_run(self, T, method='q_learning', alpha=0.1, gamma=0.99, eps_q16=6554, trajectory=False, stats=False):
        """T epsilon-greedy Q-learning / SARSA iterations per env in one launch (auto-reset always on).  eps_q16: explore
        probability in 1/65536 (65536 = always).  Rows and statistics as rollout(): read_trajectory / read_stats."""
        check(self.lib.gu_td_run(self._h, int(T), _TD_METHODS[method], float(alpha), float(gamma), int(eps_q16),
                                 _learner_flags(trajectory, stats)))

    def td_get_q(self, env0=0, n=None):
        """float64[n, S, 4]: the tables of envs env0 .. env0+n-1 (all from env0 when n is None); S << F rows under fruit, S << D under doors."""
        env0, n, n0 = self._env_range(env0, n)
        q = np.empty((n0, self.td_rows, 4), np.float64)
        check(self.lib.gu_td_get_q(self._h, env0, n, ptr(q)))
        return q

    def td_set_q(self, q, env0=0):
        """Install tables float64[n, S, 4] (or [S, 4] for one env) for envs env0 .. env0+n-1."""
        q = _tables(q, (self.td_rows, 4), 'q')
        check(self.lib.gu_td_set_q(self._h, int(env0), q.shape[0], ptr(q)))

    def td_evaluate(self, K, L, gamma=1.0, first_state=None):
        """K greedy test episodes of at most L steps per env on its td_init table (include/gu.h: gu_td_evaluate): nothing learns and
        nothing of the engine moves.  first_state: int32[K, N] start cells in the place of the drawn ones.  Returns a dict of [K, N]
        arrays: ret, len, outcome (0 ran to L, 1 goal, 2 other terminal cell, 3 ended by the overlay), end, word (uint32) and disc
        (float64, the return discounted by gamma)."""
        K = int(K)
        if first_state is not None:
            first_state = _lib.as_array(np.asarray(first_state, np.int32), np.int32, (max(K, 0), self.N), 'first_state')
        out = {k: np.empty((max(K, 0), self.N), np.int32) for k in ('ret', 'len', 'outcome', 'end')}
        out['word'] = np.empty((max(K, 0), self.N), np.uint32)
        out['disc'] = np.empty((max(K, 0), self.N), np.float64)
        check(self.lib.gu_td_evaluate(self._h, K, int(L), float(gamma), ptr(first_state), *(ptr(out[k]) for k in ('ret', 'len', 'outcome', 'end', 'word', 'disc'))))
        return out

    # ------------------------------------------------------------------ Expected SARSA and Double Q-learning (include/gu.h: gu_esarsa_run, gu_double_*)
    def esarsa_run(self, T, alpha=0.1, gamma=0.99, eps_q16=6554, trajectory=False, stats=False):
        """T Expected SARSA iterations per env in one launch on the td_init tables: acts as Q-learning does, bootstraps on the mean of
        Q[s'] under the epsilon-greedy policy."""
        check(self.lib.gu_esarsa_run(self._h, int(T), float(alpha), float(gamma), int(eps_q16), _learner_flags(trajectory, stats)))

    def double_init(self, q0=0.0):
        """A pair of float64 tables [S][2][4] per env (storage of its own, not the td_init tables), every entry q0."""
        check(self.lib.gu_double_init(self._h, float(q0)))

    def double_run(self, T, alpha=0.1, gamma=0.99, eps_q16=6554, trajectory=False, stats=False):
        """T Double Q-learning iterations per env in one launch: epsilon-greedy on A + B, a coin per step picks the table that learns."""
        check(self.lib.gu_double_run(self._h, int(T), float(alpha), float(gamma), int(eps_q16), _learner_flags(trajectory, stats)))

    def double_get_q(self, env0=0, n=None):
        """float64[n, S, 2, 4]: the pairs of envs env0 .. env0+n-1 (all from env0 when n is None); [:, :, 0] is A, [:, :, 1] is B."""
        env0, n, n0 = self._env_range(env0, n)
        q = np.empty((n0, self.spec.S, 2, 4), np.float64)
        check(self.lib.gu_double_get_q(self._h, env0, n, ptr(q)))
        return q

    def double_set_q(self, q, env0=0):
        """Install pairs float64[n, S, 2, 4] (or [S, 2, 4] for one env) for envs env0 .. env0+n-1."""
        q = _tables(q, (self.spec.S, 2, 4), 'q')
        check(self.lib.gu_double_set_q(self._h, int(env0), q.shape[0], ptr(q)))

    # ------------------------------------------------------------------ tabular Dyna-Q (include/gu.h: gu_dyna_*)
    def dyna_init(self):
        """A cleared Dyna-Q model per env (count 0, every (s, a) unobserved); the Q tables come from td_init."""
        check(self.lib.gu_dyna_init(self._h))

    def dyna_run(self, T, planning_steps=10, alpha=0.1, gamma=0.99, eps_q16=6554, trajectory=False, stats=False):
        """T real Q-learning steps per env in one launch, each followed by `planning_steps` updates replayed from the env's
        learned model.  Rows and statistics (real steps only) as td_run()."""
        check(self.lib.gu_dyna_run(self._h, int(T), int(planning_steps), float(alpha), float(gamma), int(eps_q16),
                                   _learner_flags(trajectory, stats)))

    def dyna_get_model(self, env0=0, n=None):
        """The models of envs env0 .. env0+n-1: dict next / reward / done int32[n, S, 4] (unobserved: -1 / 0 / 0),
        list int32[n, 4S] (observed pairs s*4+a in first-observation order, -1 beyond count) and count int32[n]."""
        env0, n, n0 = self._env_range(env0, n)
        S = self.spec.S
        out = dict(next=np.empty((n0, S, 4), np.int32), reward=np.empty((n0, S, 4), np.int32), done=np.empty((n0, S, 4), np.int32),
                   list=np.empty((n0, 4 * S), np.int32), count=np.empty(n0, np.int32))
        check(self.lib.gu_dyna_get_model(self._h, env0, n, ptr(out['next']), ptr(out['reward']), ptr(out['done']),
                                         ptr(out['list']), ptr(out['count'])))
        return out

    # ------------------------------------------------------------------ prioritized sweeping (include/gu.h: gu_sweep_*)
    def sweep_init(self):
        """dyna_init plus an empty priority queue per env (a grid of more than 16 384 states: GU_ERR_INVALID)."""
        check(self.lib.gu_sweep_init(self._h))

    def sweep_run(self, T, planning_steps=10, theta=1e-4, alpha=0.1, gamma=0.99, eps_q16=6554, trajectory=False, stats=False):
        """T real steps per env in one launch; each records its outcome in the env's model, queues its pair under |TD error| (above
        `theta`) and is followed by up to `planning_steps` updates of the pair with the largest priority, whose predecessors are
        queued in turn.  Rows and statistics (real steps only) as td_run()."""
        check(self.lib.gu_sweep_run(self._h, int(T), int(planning_steps), float(theta), float(alpha), float(gamma), int(eps_q16),
                                    _learner_flags(trajectory, stats)))

    def sweep_get_queue(self, env0=0, n=None):
        """The queues of envs env0 .. env0+n-1: dict key uint64[n, S, 4] (0 = not queued) and size int32[n]."""
        env0, n, n0 = self._env_range(env0, n)
        out = dict(key=np.empty((n0, self.spec.S, 4), np.uint64), size=np.empty(n0, np.int32))
        check(self.lib.gu_sweep_get_queue(self._h, env0, n, ptr(out['key']), ptr(out['size'])))
        return out

    def diag_sweep_heap(self, env0=0, n=None):
        """The device's raw form of those queues: dict heap uint64[n, 4S+2] (a 1-based binary max-heap in slots 1 .. size; slot 0:
        pops | inserts << 32 since sweep_init) and pos int32[n, 4S] (the slot of each queued pair, -1 elsewhere)."""
        env0, n, n0 = self._env_range(env0, n)
        S = self.spec.S
        out = dict(heap=np.empty((n0, 4 * S + 2), np.uint64), pos=np.empty((n0, 4 * S), np.int32))
        check(self.lib.gu_diag_sweep_heap(self._h, env0, n, ptr(out['heap']), ptr(out['pos'])))
        return out

    # ------------------------------------------------------------------ rollout search at decision time (include/gu.h: gu_search_*)
    def search_run(self, T, simulations=4, depth=16, alpha=0.1, gamma=0.99, eps_q16=6554, eps_sim_q16=65536, trajectory=False,
                   stats=False):
        """T real steps per env in one launch, each non-exploring one chosen by `simulations` (0 .. SEARCH_MAX_M) simulated rollouts
        per action of `depth` (0 .. SEARCH_MAX_D) moves with the true model, under an epsilon-greedy rollout policy (eps_sim_q16;
        65536 = uniform) on the td_init tables, which then learn from the real transition by Q-learning.  simulations = 0 is
        td_run('q_learning').  Rows and statistics (real steps only) as td_run()."""
        check(self.lib.gu_search_run(self._h, int(T), int(simulations), int(depth), float(alpha), float(gamma), int(eps_q16),
                                     int(eps_sim_q16), _learner_flags(trajectory, stats)))

    def search_get(self, env0=0, n=None):
        """Of envs env0 .. env0+n-1: dict score float64[n, 4] (the summed returns per action of the env's most recent searched
        step; zeros until there is one) and sim_steps int64[n] (simulated moves of the last launch)."""
        env0, n, n0 = self._env_range(env0, n)
        out = dict(score=np.empty((n0, 4), np.float64), sim_steps=np.empty(n0, np.int64))
        check(self.lib.gu_search_get(self._h, env0, n, ptr(out['score']), ptr(out['sim_steps'])))
        return out

    # ------------------------------------------------------------------ count-based exploration (include/gu.h: gu_explore_*)
    def explore_init(self):
        """Zeroed visit counts uint32 [S][4] per env; the Q tables come from td_init."""
        check(self.lib.gu_explore_init(self._h))

    def set_exploration(self, U, B):
        """The exploration schedule: float64 U[C] and B[C], 2 <= C <= EXPLORE_MAX_C, every entry finite and >= 0.  The bonus of
        action b in a state visited n_s times is U[min(n_s, C-1)] * B[min(n_b, C-1)] (algorithms.exploration builds both)."""
        U, B = _lib.as_array(U, np.float64, None, 'U'), _lib.as_array(B, np.float64, None, 'B')
        if U.ndim != 1 or U.shape != B.shape:
            raise ValueError('U and B must be vectors of one length, got {} and {}'.format(U.shape, B.shape))
        check(self.lib.gu_explore_set_tables(self._h, U.shape[0], ptr(U), ptr(B)))

    def explore_run(self, T, rule='ucb', alpha=0.1, gamma=0.99, eps_q16=0, trajectory=False, stats=False):
        """T Q-learning iterations per env in one launch whose non-exploring actions are greedy on Q + bonus ('ucb') or on
        Q + bonus * noise ('thompson'), the bonus from the env's visit counts and the set_exploration tables.  With tables of
        zeros it is td_run('q_learning').  Rows and statistics as td_run()."""
        check(self.lib.gu_explore_run(self._h, int(T), _EXPLORE_RULES[rule], float(alpha), float(gamma), int(eps_q16),
                                      _learner_flags(trajectory, stats)))

    def explore_get_counts(self, env0=0, n=None):
        """uint32[n, S, 4]: the visit counts of envs env0 .. env0+n-1 (all from env0 when n is None)."""
        env0, n, n0 = self._env_range(env0, n)
        c = np.empty((n0, self.spec.S, 4), np.uint32)
        check(self.lib.gu_explore_get_counts(self._h, env0, n, ptr(c)))
        return c

    def explore_set_counts(self, counts, env0=0):
        """Install counts uint32[n, S, 4] (or [S, 4] for one env) for envs env0 .. env0+n-1; none above EXPLORE_COUNT_MAX."""
        c = np.asarray(counts)
        if c.size and (c.min() < 0 or c.max() > 0xFFFFFFFF):
            raise ValueError('counts must fit uint32')
        c = _tables(c.astype(np.uint32), (self.spec.S, 4), 'counts', np.uint32)
        check(self.lib.gu_explore_set_counts(self._h, int(env0), c.shape[0], ptr(c)))

    # ------------------------------------------------------------------ Monte-Carlo tree search at decision time (include/gu.h: gu_mcts_*)
    def mcts_init(self, max_sims=64):
        """An empty pool of max_sims + 1 tree nodes per env (1 <= max_sims <= MCTS_MAX_SIMS); the Q tables come from td_init."""
        check(self.lib.gu_mcts_init(self._h, int(max_sims)))

    def set_tree_tables(self, U, B, I):
        """The schedule of the tree search: float64 U[C], B[C] and I[C], 2 <= C <= EXPLORE_MAX_C, every entry finite and >= 0.  An
        action tried n_b times at a node visited n_s times scores w_b * I[min(n_b, C-1)] + U[min(n_s, C-1)] * B[min(n_b, C-1)]
        (algorithms.search.uct_tables builds UCB1's)."""
        U, B, I = (_lib.as_array(t, np.float64, None, k) for t, k in ((U, 'U'), (B, 'B'), (I, 'I')))
        if U.ndim != 1 or U.shape != B.shape or U.shape != I.shape:
            raise ValueError('U, B and I must be vectors of one length, got {}, {} and {}'.format(U.shape, B.shape, I.shape))
        check(self.lib.gu_mcts_set_tables(self._h, U.shape[0], ptr(U), ptr(B), ptr(I)))

    def mcts_run(self, T, simulations=64, tree_depth=8, depth=4, alpha=0.1, gamma=0.99, eps_q16=6554, eps_sim_q16=65536, trajectory=False,
                 stats=False):
        """T real steps per env in one launch, each non-exploring one chosen by a UCT tree of `simulations` (0 .. mcts_init's
        max_sims) simulations with the true model: selection down to `tree_depth` (1 .. MCTS_MAX_DEPTH) levels, one new node, a
        rollout of `depth` (0 .. SEARCH_MAX_D) moves under an epsilon-greedy policy (eps_sim_q16; 65536 = uniform) on the td_init
        tables, which then learn from the real transition by Q-learning.  simulations = 0 is td_run('q_learning').  Rows and
        statistics (real steps only) as td_run()."""
        check(self.lib.gu_mcts_run(self._h, int(T), int(simulations), int(tree_depth), int(depth), float(alpha), float(gamma), int(eps_q16),
                                   int(eps_sim_q16), _learner_flags(trajectory, stats)))

    def mcts_get(self, env0=0, n=None):
        """Of envs env0 .. env0+n-1, from each env's most recent searched step: dict w float64[n, 4] and visits uint32[n, 4] (the
        root's return sums and visit counts; zeros until there is one), nodes int32[n] (the nodes of that tree) and sim_steps
        int64[n] (simulated moves of the last launch)."""
        env0, n, n0 = self._env_range(env0, n)
        out = dict(w=np.empty((n0, 4), np.float64), visits=np.empty((n0, 4), np.uint32), nodes=np.empty(n0, np.int32),
                   sim_steps=np.empty(n0, np.int64))
        check(self.lib.gu_mcts_get(self._h, env0, n, ptr(out['w']), ptr(out['visits']), ptr(out['nodes']), ptr(out['sim_steps'])))
        return out

    def mcts_tree(self, env0=0, n=None):
        """The whole tree of each env's most recent searched step, P = max_sims + 1 node slots per env in order of creation: dict
        state int32[n, P], parent int32[n, P] (parent * 4 + action; -1 for the root), child int32[n, P, 4] (-1 = none), visits
        uint32[n, P, 4], w float64[n, P, 4] and count int32[n]; slots beyond count hold -1 / -1 / -1 / 0 / 0.0."""
        env0, n, n0 = self._env_range(env0, n)
        P = self.stores()['mcts_nodes']
        out = dict(state=np.empty((n0, P), np.int32), parent=np.empty((n0, P), np.int32), child=np.empty((n0, P, 4), np.int32),
                   visits=np.empty((n0, P, 4), np.uint32), w=np.empty((n0, P, 4), np.float64), count=np.empty(n0, np.int32))
        check(self.lib.gu_mcts_get_tree(self._h, env0, n, ptr(out['state']), ptr(out['parent']), ptr(out['child']), ptr(out['visits']),
                                        ptr(out['w']), ptr(out['count'])))
        return out

    # ------------------------------------------------------------------ tabular n-step Q-learning / SARSA (include/gu.h: gu_nstep_*)
    def nstep_run(self, T, method='sarsa', n=4, alpha=0.1, gamma=0.99, eps_q16=6554, trajectory=False, stats=False):
        """T iterations of n-step Q-learning / SARSA per env in one launch, into the td_init tables.  The window of pending
        transitions carries into the next nstep_run of the same method and n; any other call in between drops it.  Rows and
        statistics as td_run()."""
        check(self.lib.gu_nstep_run(self._h, int(T), _TD_METHODS[method], int(n), float(alpha), float(gamma), int(eps_q16),
                                    _learner_flags(trajectory, stats)))

    def nstep_get_window(self, env0=0, n=None):
        """The windows of envs env0 .. env0+n-1: dict sa / reward int32[n, NSTEP_MAX] (pending s*4+a and r, oldest first;
        -1 / 0 beyond count) and count int32[n] (0 once dropped)."""
        env0, n, n0 = self._env_range(env0, n)
        out = dict(sa=np.empty((n0, _lib.NSTEP_MAX), np.int32), reward=np.empty((n0, _lib.NSTEP_MAX), np.int32),
                   count=np.empty(n0, np.int32))
        check(self.lib.gu_nstep_get_window(self._h, env0, n, ptr(out['sa']), ptr(out['reward']), ptr(out['count'])))
        return out

    # ------------------------------------------------------------------ tabular SARSA(lambda) / Watkins's Q(lambda) (include/gu.h: gu_lambda_*)
    def lambda_run(self, T, method='sarsa', K=32, lam=0.9, alpha=0.1, gamma=0.99, eps_q16=6554, trajectory=False, stats=False):
        """T iterations of SARSA(lambda) ('sarsa') / Watkins's Q(lambda) ('q_learning') per env in one launch, into the td_init
        tables: replacing traces, truncated after K (1 .. LAMBDA_MAX) steps.  The trace window carries into the next lambda_run of
        the same method and K; any other call in between drops it.  Rows and statistics as td_run()."""
        check(self.lib.gu_lambda_run(self._h, int(T), _TD_METHODS[method], int(K), float(alpha), float(gamma), float(lam),
                                     int(eps_q16), _learner_flags(trajectory, stats)))

    def lambda_get_window(self, env0=0, n=None):
        """int32[n, LAMBDA_MAX]: the trace windows of envs env0 .. env0+n-1, index = age (the pair s*4+a, -1 for none; all -1
        once dropped)."""
        env0, n, n0 = self._env_range(env0, n)
        sa = np.empty((n0, _lib.LAMBDA_MAX), np.int32)
        check(self.lib.gu_lambda_get_window(self._h, env0, n, ptr(sa)))
        return sa

    # ------------------------------------------------------------------ tabular softmax actor-critic (include/gu.h: gu_ac_*)
    def ac_init(self, h0=0.0, v0=0.0):
        """One float64 preference table [S][4] (every entry h0) and one value table [S] (every entry v0) per env."""
        check(self.lib.gu_ac_init(self._h, float(h0), float(v0)))

    def ac_run(self, T, alpha_actor=0.1, alpha_critic=0.1, gamma=0.99, trajectory=False, stats=False):
        """T one-step actor-critic iterations per env in one launch (softmax policy, auto-reset always on).  Rows and
        statistics as td_run()."""
        check(self.lib.gu_ac_run(self._h, int(T), float(alpha_actor), float(alpha_critic), float(gamma),
                                 _learner_flags(trajectory, stats)))

    def ac_get(self, env0=0, n=None):
        """(preferences float64[n, S, 4], values float64[n, S]) of envs env0 .. env0+n-1 (all from env0 when n is None)."""
        env0, n, n0 = self._env_range(env0, n)
        S = self.spec.S
        h, v = np.empty((n0, S, 4), np.float64), np.empty((n0, S), np.float64)
        check(self.lib.gu_ac_get(self._h, env0, n, ptr(h), ptr(v)))
        return h, v

    def ac_set(self, h=None, v=None, env0=0):
        """Install preferences float64[n, S, 4] (or [S, 4]) and / or values float64[n, S] (or [S]) for envs env0 ..; when both
        are given they must cover the same envs."""
        S, n = self.spec.S, None
        if h is not None:
            h = _tables(h, (S, 4), 'h')
            n = h.shape[0]
        if v is not None:
            v = _tables(v, (S,), 'v')
            if n is not None and v.shape[0] != n:
                raise ValueError('h and v cover {} and {} envs'.format(n, v.shape[0]))
            n = v.shape[0]
        if n is None:
            raise ValueError('give h, v or both')
        check(self.lib.gu_ac_set(self._h, int(env0), n, ptr(h) if h is not None else None, ptr(v) if v is not None else None))

    # ------------------------------------------------------------------ tabular REINFORCE with baseline (include/gu.h: gu_reinforce_*)
    def reinforce_run(self, T, L=256, alpha_actor=0.003, alpha_baseline=0.1, gamma=0.99, trajectory=False, stats=False):
        """T iterations of REINFORCE with baseline per env in one launch, into the ac_init tables: the backward pass over a
        segment runs when its episode ends or after L (1 .. REINFORCE_MAX) steps.  The episode buffer carries into the next
        reinforce_run with the same L; any other call in between drops it.  Rows and statistics as td_run()."""
        check(self.lib.gu_reinforce_run(self._h, int(T), int(L), float(alpha_actor), float(alpha_baseline), float(gamma),
                                        _learner_flags(trajectory, stats)))

    def reinforce_get_episode(self, env0=0, n=None):
        """The episode buffers of envs env0 .. env0+n-1: dict sa / reward int32[n, REINFORCE_MAX] (pending s*4+a and r, oldest
        first; -1 / 0 beyond count) and count int32[n] (0 once dropped)."""
        env0, n, n0 = self._env_range(env0, n)
        out = dict(sa=np.empty((n0, _lib.REINFORCE_MAX), np.int32), reward=np.empty((n0, _lib.REINFORCE_MAX), np.int32),
                   count=np.empty(n0, np.int32))
        check(self.lib.gu_reinforce_get_episode(self._h, env0, n, ptr(out['sa']), ptr(out['reward']), ptr(out['count'])))
        return out

    # ------------------------------------------------------------------ off-policy Monte-Carlo control, weighted importance sampling (include/gu.h: gu_is_*)
    def is_init(self):
        """One float64 table [S][4] of cumulative weights per env, all zero; the Q tables come from td_init."""
        check(self.lib.gu_is_init(self._h))

    def is_run(self, T, L=64, gamma=0.99, eps_q16=6554, w_cap=2.0 ** 64, trajectory=False, stats=False):
        """T iterations of off-policy every-visit Monte-Carlo control with weighted importance sampling per env in one launch,
        into the td_init tables and the is_init weights: epsilon-greedy behaviour, greedy target; the backward pass over a
        segment runs when its episode ends or after L (1 .. IS_MAX) steps and stops at the first action that is no longer
        greedy, or where the weight leaves [2^-256, w_cap).  The episode buffer carries into the next is_run with the same L;
        any other call in between drops it.  Rows and statistics as td_run()."""
        check(self.lib.gu_is_run(self._h, int(T), int(L), float(gamma), int(eps_q16), float(w_cap), _learner_flags(trajectory, stats)))

    def is_get(self, env0=0, n=None):
        """float64[n, S, 4]: the cumulative weights of envs env0 .. env0+n-1 (all from env0 when n is None)."""
        env0, n, n0 = self._env_range(env0, n)
        c = np.empty((n0, self.spec.S, 4), np.float64)
        check(self.lib.gu_is_get(self._h, env0, n, ptr(c)))
        return c

    def is_set(self, c, env0=0):
        """Install cumulative weights float64[n, S, 4] (or [S, 4] for one env) for envs env0 .. env0+n-1: finite, not negative."""
        c = _tables(c, (self.spec.S, 4), 'c')
        check(self.lib.gu_is_set(self._h, int(env0), c.shape[0], ptr(c)))

    def is_get_episode(self, env0=0, n=None):
        """The episode buffers of envs env0 .. env0+n-1: dict sa / reward / cls int32[n, IS_MAX] (pending s*4+a, r and the class
        of the action, oldest first; -1 / 0 / 0 beyond count) and count int32[n] (0 once dropped)."""
        env0, n, n0 = self._env_range(env0, n)
        out = dict(sa=np.empty((n0, _lib.IS_MAX), np.int32), reward=np.empty((n0, _lib.IS_MAX), np.int32),
                   cls=np.empty((n0, _lib.IS_MAX), np.int32), count=np.empty(n0, np.int32))
        check(self.lib.gu_is_get_episode(self._h, env0, n, ptr(out['sa']), ptr(out['reward']), ptr(out['cls']), ptr(out['count'])))
        return out

    # ------------------------------------------------------------------ the learners' float64 building blocks (include/gu_diag.h: gu_probe_numeric*)
    def _probe_numeric(self, op, x):
        x = np.ascontiguousarray(x, np.float64).reshape(-1)
        y = np.empty_like(x)
        if x.size:
            check(self.lib.gu_probe_numeric(self._h, op, x.size, ptr(x), ptr(y)))
        return y

    def probe_exp(self, x):
        """float64[n]: the device's gu_exp of x[n] (x <= 0, -inf included)."""
        return self._probe_numeric(_lib.PROBE_EXP, x)

    def probe_recip14(self, z):
        """float64[n]: the device's gu_recip14 of z[n], the correctly rounded 1 / z of z in [1, 4]."""
        return self._probe_numeric(_lib.PROBE_RECIP14, z)

    def probe_is_recip(self, x):
        """float64[n]: the device's RECIP of gu_is_run on x[n], positive normal numbers whose reciprocals are normal."""
        return self._probe_numeric(_lib.PROBE_IS_RECIP, x)

    def probe_softmax(self, h, w):
        """Rules 2 and 3 of gu_ac_run on the device for preference rows h float64[n, 4] and words w uint32[n]: dict e float64[n, 4],
        Z and iz float64[n], action int32[n]."""
        h = np.ascontiguousarray(h, np.float64)
        w = np.ascontiguousarray(w, np.uint32).reshape(-1)
        if h.ndim != 2 or h.shape[1] != 4 or h.shape[0] != w.size:
            raise ValueError('h must be [n, 4] and w [n], got {} and {}'.format(h.shape, w.shape))
        n = w.size
        out = dict(e=np.empty((n, 4), np.float64), Z=np.empty(n, np.float64), iz=np.empty(n, np.float64), action=np.empty(n, np.int32))
        if n:
            check(self.lib.gu_probe_numeric_softmax(self._h, n, ptr(h), ptr(w), ptr(out['e']), ptr(out['Z']), ptr(out['iz']), ptr(out['action'])))
        return out

    # ------------------------------------------------------------------ semi-gradient SARSA / Q-learning on features (include/gu.h: gu_fa_*)
    def fa_init(self, phi, n_features=None, w0=0.0):
        """Install the feature table phi int32[S, K] (K active binary features per state, 1 <= K <= FA_MAX_K, column k a slot of
        its own) shared by all envs, and one float64 weight table [F][4] per env, every entry w0.  F = n_features, or
        phi.max() + 1."""
        phi = np.asarray(phi)
        if phi.ndim == 1:
            phi = phi[:, None]
        if phi.ndim != 2 or phi.shape[0] != self.spec.S:
            raise ValueError('phi must have shape ({}, K), got {}'.format(self.spec.S, phi.shape))
        phi = _lib.as_array(phi, np.int32, None, 'phi')
        F = (int(phi.max()) + 1 if phi.size else 0) if n_features is None else int(n_features)
        check(self.lib.gu_fa_init(self._h, phi.shape[1], F, ptr(phi), float(w0)))

    def _fa_features(self):
        F = self.stores()['fa_f']
        if not F:  # (never made, or dropped by a grid of another size)
            raise RuntimeError('no features: call fa_init first')
        return F

    def fa_run(self, T, method='sarsa', alpha=0.1, gamma=0.99, eps_q16=6554, trajectory=False, stats=False):
        """T iterations of episodic semi-gradient SARSA / Q-learning per env in one launch, on the fa_init features.  alpha is
        applied as given (divide by K yourself).  Rows and statistics as td_run()."""
        check(self.lib.gu_fa_run(self._h, int(T), _TD_METHODS[method], float(alpha), float(gamma), int(eps_q16),
                                 _learner_flags(trajectory, stats)))

    def fa_get_w(self, env0=0, n=None):
        """float64[n, F, 4]: the weights of envs env0 .. env0+n-1 (all from env0 when n is None)."""
        env0, n, n0 = self._env_range(env0, n)
        w = np.empty((n0, self._fa_features(), 4), np.float64)
        check(self.lib.gu_fa_get_w(self._h, env0, n, ptr(w)))
        return w

    def fa_set_w(self, w, env0=0):
        """Install weights float64[n, F, 4] (or [F, 4] for one env) for envs env0 .. env0+n-1."""
        w = _tables(w, (self._fa_features(), 4), 'w')
        check(self.lib.gu_fa_set_w(self._h, int(env0), w.shape[0], ptr(w)))

    def fa_get_q(self, env0=0, n=None):
        """float64[n, S, 4]: the action values of envs env0 .. env0+n-1, folded from the weights on the device."""
        env0, n, n0 = self._env_range(env0, n)
        q = np.empty((n0, self.spec.S, 4), np.float64)
        check(self.lib.gu_fa_get_q(self._h, env0, n, ptr(q)))
        return q

    # ------------------------------------------------------------------ state
    def get_state(self):
        pos, don = np.empty(self.N, np.int32), np.empty(self.N, np.int32)
        ep, tc = np.empty(self.N, np.uint32), np.empty(self.N, np.uint64)  # (step counts have 64 bits: include/gu.h, state)
        check(self.lib.gu_get_state(self._h, ptr(pos), ptr(don), ptr(ep), ptr(tc)))
        return dict(pos=pos, done=don, episode=ep, tcount=tc)

    def set_state(self, pos=None, done=None, episode=None, tcount=None):
        pos = None if pos is None else _lib.as_array(pos, np.int32, (self.N,), 'pos')
        done = None if done is None else _lib.as_array(done, np.int32, (self.N,), 'done')
        episode = None if episode is None else _lib.as_array(episode, np.uint32, (self.N,), 'episode')
        tcount = None if tcount is None else _lib.as_array(tcount, np.uint64, (self.N,), 'tcount')
        check(self.lib.gu_set_state(self._h, ptr(pos), ptr(done), ptr(episode), ptr(tcount)))

    STORES = ('s', 'n_grids', 'overlay', 'overlay_bits', 'td_rows', 'double', 'dyna', 'sweep', 'explore', 'explore_c', 'mcts_nodes', 'mcts_c', 'ac', 'is', 'fa_f',
              'fa_k', 'trail_cap')

    def stores(self):
        """What the engine holds right now (gu_get_stores): dict of the GU_STORE_* words under the names of STORES.  A store's word is
        non-zero exactly when the calls that need the store would find it; 'td_rows' counts only tables of the rows td_run learns on
        now, s << overlay_bits.  A few host loads in the library: no synchronisation, nothing a learner carries is dropped.  Nothing in
        Python keeps such a fact: whoever needs one asks here."""
        words = (ctypes.c_int64 * len(self.STORES))()
        check(self.lib.gu_get_stores(self._h, len(self.STORES), words, None))
        return dict(zip(self.STORES, words))

    def done_indices(self):
        idx = np.empty(self.N, np.int32)
        count = ctypes.c_int32(0)
        check(self.lib.gu_done_indices(self._h, ptr(idx), ctypes.byref(count)))
        return idx[:count.value].copy()

    def look_step_ahead(self, states, actions, care_about_terminal=True):
        s = np.ascontiguousarray(states, dtype=np.int32).ravel()
        a = np.ascontiguousarray(actions, dtype=np.int32).ravel()
        if s.size != a.size:
            raise ValueError('states and actions must have the same number of elements')
        nxt, rew, don = (np.empty(s.size, np.int32) for _ in range(3))
        check(self.lib.gu_look_step_ahead(self._h, s.size, ptr(s), ptr(a), 1 if care_about_terminal else 0,
                                          ptr(nxt), ptr(rew), ptr(don)))
        return nxt, rew, don

    # ------------------------------------------------------------------ tabular DP
    def vi_set(self, v, pi):
        S = self.spec.S
        v = _lib.as_array(v, np.float64, (S,), 'value_function')
        pi = _lib.as_array(pi, np.float64, (S, 4), 'policy')
        check(self.lib.gu_vi_set(self._h, ptr(v), ptr(pi)))

    def vi_sweep(self, gamma=1.0, iters=1, greedy_update=True):
        deltas = np.empty(int(iters), np.float64)
        check(self.lib.gu_vi_sweep(self._h, float(gamma), int(iters), 1 if greedy_update else 0, ptr(deltas)))
        return deltas

    def vi_run(self, gamma=1.0, threshold=1e-5, max_steps=1000):
        """value_iteration's loop in one call (stopping rule on the device).  Returns (rounds done, deltas)."""
        done = ctypes.c_int32(0)
        deltas = np.full(max(int(max_steps), 1), np.nan)
        check(self.lib.gu_vi_run(self._h, float(gamma), float(threshold), int(max_steps), ctypes.byref(done), ptr(deltas)))
        return done.value, deltas[:done.value].copy()

    def vi_eval_run(self, gamma=1.0, threshold=1e-5, max_steps=1000):
        """policy_iteration's evaluation loop: V1 sweeps on the fixed policy until delta < threshold (or max_steps).
        Returns (sweeps done, deltas)."""
        done = ctypes.c_int32(0)
        deltas = np.full(max(int(max_steps), 1), np.nan)
        check(self.lib.gu_vi_eval_run(self._h, float(gamma), float(threshold), int(max_steps), ctypes.byref(done), ptr(deltas)))
        return done.value, deltas[:done.value].copy()

    def vi_greedy(self, gamma=1.0):
        check(self.lib.gu_vi_greedy(self._h, float(gamma)))

    def vi_get(self):
        S = self.spec.S
        v, pi = np.empty(S, np.float64), np.empty((S, 4), np.float64)
        check(self.lib.gu_vi_get(self._h, ptr(v), ptr(pi)))
        return v, pi

    def vi_sweep_step(self, gamma=1.0, auto_reset=False, want_delta=True):
        d = ctypes.c_double(0.0)
        check(self.lib.gu_vi_sweep_step(self._h, float(gamma), _lib.F_AUTO_RESET if auto_reset else 0,
                                        ctypes.byref(d) if want_delta else None))
        return d.value if want_delta else None

    def vi_sweep_step_run(self, gamma=1.0, iters=1, auto_reset=False):
        """`iters` rounds of {V1 + V2 sweep; every env steps greedily on the updated policy} -- one launch (synchronised per XCD, or
        chip-wide) when table and batch fit the resident workgroups, see vi_last_form().  Returns the per-round deltas."""
        deltas = np.empty(int(iters), np.float64)
        check(self.lib.gu_vi_sweep_step_run(self._h, float(gamma), int(iters), _lib.F_AUTO_RESET if auto_reset else 0, ptr(deltas)))
        return deltas

    def vi_last_form(self):
        """Which form the last vi_sweep_step_run took: 1 = one launch synchronised per XCD, 2 = one launch with a chip-wide
        barrier per round, 3 = one launch per round (0: none yet)."""
        return int(self.lib.gu_vi_last_form(self._h))

    def vi_last_dp_form(self):
        """Which form finished the last vi_sweep / vi_run / vi_eval_run: 1 = one XCD's workgroups in one launch, 2 = one workgroup,
        3 = chip-wide cluster, 4 = one launch per round (0: none yet)."""
        return int(self.lib.gu_vi_last_dp_form(self._h))

    def vi_xcd_torn_words(self):
        """A -DGU_VI_XCD_TORN build: exchange words of the per-XCD launches found with the right tag and the wrong payload, summed over
        this engine's launches; None on the product library."""
        n = ctypes.c_int64(0)
        rc = self.lib.gu_vi_xcd_torn_words(self._h, ctypes.byref(n))
        return None if rc else int(n.value)

    def vi_last_clusters(self):
        """Workgroups per XCC id in the last per-XCD launch of vi_sweep_step_run, as the hardware reported them (list of 8)."""
        m = np.zeros(8, np.int32)
        check(self.lib.gu_vi_last_clusters(self._h, ptr(m)))
        return m.tolist()

    def mc_walk_lengths(self, u, n_offsets, start_states, cap, cdf):
        """include/gu.h: gu_mc_walk_lengths.  uint16[n_starts, n_offsets]: the length of the reference's episode that begins at uniform
        i of `u` in start cell start_states[c] (0xFFFF: the uniforms ran out before it ended)."""
        u = _lib.as_array(u, np.float64, None, 'u')
        starts = _lib.as_array(start_states, np.int32, None, 'start_states')
        cdf = _lib.as_array(cdf, np.float64, (self.spec.S, 4), 'cdf')  # (the library copies S * 32 bytes from it)
        out = np.empty((starts.size, int(n_offsets)), np.uint16)
        check(self.lib.gu_mc_walk_lengths(self._h, u.size, ptr(u), int(n_offsets), starts.size, ptr(starts), int(cap), ptr(cdf), ptr(out)))
        return out

    def mc_walk_episodes(self, u, cdf, offsets, first_state, cap, T):
        """include/gu.h: gu_mc_walk_episodes: episode e from uniform offsets[e] and cell first_state[e] into rows 0 .. T-1 of the trajectory."""
        u = _lib.as_array(u, np.float64, None, 'u')
        cdf = _lib.as_array(cdf, np.float64, (self.spec.S, 4), 'cdf')
        off = _lib.as_array(offsets, np.int64, (self.N,), 'offsets')
        first = _lib.as_array(first_state, np.int32, (self.N,), 'first_state')
        check(self.lib.gu_mc_walk_episodes(self._h, u.size, ptr(u), ptr(cdf), ptr(off), ptr(first), int(cap), int(T)))

    def mc_evaluate(self, T, first_state, discount_pow, keep, every_visit=False, incremental_mean=True,
                    stationary_env=True, alpha=0.001):
        """Monte-Carlo evaluation over the trajectory rows 0..T-1 of the last rollout (env e = episode e).
        Returns (value_function[S], total_visit_counter[S])."""
        first = _lib.as_array(first_state, np.int32, (self.N,), 'first_state')
        pw = _lib.as_array(discount_pow, np.float64, (T,), 'discount_pow')
        kp = _lib.as_array(np.asarray(keep).astype(bool), np.uint8, (T,), 'keep')
        S = self.spec.S
        value, visits = np.empty(S, np.float64), np.empty(S, np.float64)
        check(self.lib.gu_mc_evaluate(self._h, int(T), ptr(first), 1 if every_visit else 0, 1 if incremental_mean else 0,
                                      1 if stationary_env else 0, float(alpha), ptr(pw), ptr(kp), ptr(value), ptr(visits)))
        return value, visits

    def shortest_paths(self, max_path=None):
        """Breadth-first shortest path from each grid's first start cell to the first terminal state the FIFO search
        dequeues (maze_solving.py semantics).  Returns a list with one int8 action array (or None) per grid, plus the
        terminal states reached."""
        G, S = self.stores()['n_grids'], self.spec.S
        max_path = int(max_path or S)
        path = np.zeros((G, max_path), np.int8)
        plen, term = np.zeros(G, np.int32), np.zeros(G, np.int32)
        check(self.lib.gu_shortest_paths(self._h, max_path, ptr(path), ptr(plen), ptr(term)))
        if (plen == -2).any():
            raise ValueError('a path is longer than max_path={}'.format(max_path))
        return [None if n < 0 else path[g, :n].copy() for g, n in enumerate(plen)], term

    def render_policy_rgb(self, cell_px=52):
        """uint8[H*cell_px, W*cell_px, 3]: the tiles of grid 0 with the current policy table drawn as arrows."""
        out = np.empty((self.spec.H * cell_px, self.spec.W * cell_px, 3), np.uint8)
        check(self.lib.gu_render_policy_rgb(self._h, int(cell_px), ptr(out)))
        return out

    def render_rgb(self, env0=0, n_envs=1, cell_px=8):
        """uint8[n_envs, H*cell_px, W*cell_px, 3] frames of envs env0 .. env0+n_envs-1 (rendered on the device)."""
        W, H = self.spec.W, self.spec.H
        out = np.empty((int(n_envs), H * cell_px, W * cell_px, 3), np.uint8)
        check(self.lib.gu_render_rgb(self._h, int(env0), int(n_envs), int(cell_px), ptr(out)))
        return out

    def _view_shape(self, mode, radius):
        return (self.spec.H, self.spec.W) if mode else (2 * radius + 1, 2 * radius + 1)

    def sense(self, env0=0, n=None, radius=1, mode='ego'):
        """uint8[n, K, K] ('ego', K = 2 * radius + 1) or uint8[n, H, W] ('grid'): what envs env0 .. env0+n-1 (to the end when n is
        None) see from where they stand (include/gu.h: gu_sense)."""
        m, r = check_sense_args(radius, mode)
        env0, n, n0 = self._env_range(env0, n)
        out = np.empty((n0,) + self._view_shape(m, r), np.uint8)
        check(self.lib.gu_sense(self._h, env0, n, m, r, ptr(out)))
        return out

    def sense_trajectory(self, t0, T, radius=1, mode='ego', chunk_bytes=256 << 20):
        """uint8[T, N, K, K] or uint8[T, N, H, W]: the views along rows t0 .. t0+T-1 of the trajectory buffer, the position
        being each row's obs (include/gu.h: gu_sense_trajectory).  One library call per run of rows of at most `chunk_bytes`."""
        m, r = check_sense_args(radius, mode)
        t0, T = int(t0), int(T)
        shape = self._view_shape(m, r)
        out = np.empty((max(T, 0), self.N) + shape, np.uint8)
        rows = max(1, int(chunk_bytes) // (self.N * shape[0] * shape[1]))
        if T <= 0:  # (the library's message)
            check(self.lib.gu_sense_trajectory(self._h, t0, T, m, r, None))
        for r0 in range(0, T, rows):
            nr = min(rows, T - r0)
            check(self.lib.gu_sense_trajectory(self._h, t0 + r0, nr, m, r, ptr(out[r0:r0 + nr])))
        return out

    def sense_device(self, T=None, t0=0, radius=1, mode='ego'):
        """The sensor kernel alone, for timing (tools/sense_rate.py): the views of the current state (T None) or of T rows stay
        in the engine's scratch memory; nothing is copied."""
        m, r = check_sense_args(radius, mode)
        if T is None:
            check(self.lib.gu_sense(self._h, 0, self.N, m, r, None))
        else:
            check(self.lib.gu_sense_trajectory(self._h, int(t0), int(T), m, r, None))

    def trail_enable(self, capacity=500):
        """Keep the reference viewer's agent trail per env (env:92-93, 182-184, 190: the cell after every step, newest `capacity`
        <= 500, emptied by reset) and blend it into render_rgb frames (rendering.py:287-311); 0 switches it off again."""
        check(self.lib.gu_trail_enable(self._h, int(capacity)))

    def trail_read(self, env0=0, n_envs=1):
        """The trails of envs env0 .. env0 + n_envs - 1 as lists of cells, oldest first (the reference's last_n_states as states)."""
        cap = self.stores()['trail_cap']
        cells, length = np.empty((int(n_envs), max(cap, 1)), np.int32), np.empty(int(n_envs), np.int32)
        check(self.lib.gu_trail_read(self._h, int(env0), int(n_envs), ptr(cells), ptr(length)))
        return [cells[k, :length[k]].tolist() for k in range(int(n_envs))]

    # ------------------------------------------------------------------ stream / timing
    def sync(self):
        check(self.lib.gu_sync(self._h))

    def timer_begin(self):
        check(self.lib.gu_timer_begin(self._h))

    def timer_end(self):
        ms = ctypes.c_float(0.0)
        check(self.lib.gu_timer_end(self._h, ctypes.byref(ms)))
        return ms.value

    def timer_mark(self):
        check(self.lib.gu_timer_mark(self._h))

    def timer_laps(self, max_laps=65536):
        """Milliseconds between consecutive timer_mark() events (waits for the last one)."""
        ms = np.empty(int(max_laps), np.float32)
        n = ctypes.c_int32(0)
        check(self.lib.gu_timer_laps(self._h, ptr(ms), int(max_laps), ctypes.byref(n)))
        return ms[:n.value].astype(np.float64)

    # ------------------------------------------------------------------ RCCL gathered view
    @staticmethod
    def comm_unique_id():
        buf = np.zeros(_lib.COMM_ID_BYTES, np.uint8)
        check(_lib.load().gu_comm_unique_id(ptr(buf)))
        return buf.tobytes()

    def comm_init(self, nranks, rank, unique_id):
        buf = np.frombuffer(bytes(unique_id), dtype=np.uint8).copy()
        if buf.size != _lib.COMM_ID_BYTES:
            raise ValueError('unique id must be {} bytes'.format(_lib.COMM_ID_BYTES))
        check(self.lib.gu_comm_init(self._h, int(nranks), int(rank), ptr(buf)))
        self.nranks, self.rank = int(nranks), int(rank)

    def comm_destroy(self):
        check(self.lib.gu_comm_destroy(self._h))

    # one process, one engine per device (ncclCommInitAll + one grouped all-gather; every engine on its own device)
    @staticmethod
    def comm_init_all(engines):
        handles = (ctypes.c_void_p * len(engines))(*[e._h for e in engines])
        check(_lib.load().gu_comm_init_all(handles, len(engines)))
        for rank, e in enumerate(engines):
            e.nranks, e.rank = len(engines), rank

    @staticmethod
    def allgather_view_all(engines):
        """(obs, reward, done) of all engines' envs, env-major: one grouped RCCL all-gather, read from the first device."""
        handles = (ctypes.c_void_p * len(engines))(*[e._h for e in engines])
        total = sum(e.N for e in engines)
        obs, rew, don = (np.empty(total, np.int32) for _ in range(3))
        check(_lib.load().gu_allgather_view_all(handles, len(engines), ptr(obs), ptr(rew), ptr(don)))
        return obs, rew, don

    def allgather_view(self):
        total = self.nranks * self.N
        obs, rew, don = (np.empty(total, np.int32) for _ in range(3))
        check(self.lib.gu_allgather_view(self._h, ptr(obs), ptr(rew), ptr(don)))
        return obs, rew, don
