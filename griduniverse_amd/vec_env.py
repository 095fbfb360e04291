"""VecGridUniverse -- N lock-stepped GridUniverse instances on one MI355X.

The batched counterpart of the reference's per-instance loop

    obs = env.reset()
    for t in range(T):
        obs, reward, done, info = env.step(action)      # core/envs/griduniverse_env.py:176-185
        if done: env.reset()                            # harness policy, e.g. monte_carlo.py:25

with the same grid construction kwargs as `GridUniverseEnv` (one shared grid), array
in / array out.  `rollout(T)` fuses the whole caller loop into one kernel launch.
Sharding across GPUs: give every rank its slice via `env_id0`; per-env RNG streams are
keyed by GLOBAL env id, so the union of the shards equals the single-device batch byte
for byte (see `parallel.py`).
"""

import numpy as np

from . import _lib, softmax
from .engine import Engine
from .envs.griduniverse_env import GridUniverseEnv
from .grid import (BOX_INITIAL, BOX_ON_TARGET_MAX, BOX_TARGET, DOOR_KINDS, ERRAND_FRUIT_MAX, FRUIT_KINDS, GridSpec, box_bits, box_plane, door_plane, errand_bytes,
                   errand_fields, errand_words, fruit_plane, pack_boxes, unpack_boxes, wind_plane)


def _q16(x):
    """A probability as the library takes it: in 1/65536, to the nearest."""
    return int(round(float(x) * 65536))


def _unit(name, x):
    """`x` lies in [0, 1] (ValueError; NaN fails too)."""
    if not 0.0 <= float(x) <= 1.0:
        raise ValueError('{} must lie in [0, 1]'.format(name))


def check_off_policy_args(max_episode_len, epsilon, w_cap):
    """The argument checks of off_policy_mc_run and algorithms.off_policy (ValueError)."""
    if not 1 <= int(max_episode_len) <= _lib.IS_MAX:
        raise ValueError('max_episode_len must lie in 1 .. {}'.format(_lib.IS_MAX))
    _unit('epsilon', epsilon)
    if not 1.0 <= float(w_cap) <= 2.0 ** 256:  # (NaN and infinity fail too)
        raise ValueError('w_cap must lie in [1, 2**256]')


def check_evaluate_args(episodes, max_steps, discount_factor, first_state, num_envs, S):
    """The argument checks of evaluate() and algorithms.evaluation (ValueError); returns first_state as int32[episodes, num_envs] or None.  S None: the
    library checks the cells' range."""
    for name, v in (('episodes', episodes), ('max_steps', max_steps)):
        if v is None and name == 'max_steps':
            continue
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
            raise ValueError('{} must be an integer of at least 1'.format(name))
    if episodes > _lib.EVAL_MAX_K or episodes * num_envs > _lib.EVAL_MAX_LANES:
        raise ValueError('episodes must be at most {} and episodes x envs at most {}'.format(_lib.EVAL_MAX_K, _lib.EVAL_MAX_LANES))
    if max_steps is not None and episodes * max_steps > _lib.EVAL_BUDGET:
        raise ValueError('episodes x max_steps must be at most {}'.format(_lib.EVAL_BUDGET))
    if not np.isfinite(float(discount_factor)):
        raise ValueError('discount_factor must be finite')
    if first_state is None:
        return None
    f = np.asarray(first_state)
    if f.dtype == bool or not np.issubdtype(f.dtype, np.integer) or f.shape != (episodes, num_envs):
        raise ValueError('first_state must be integers of shape ({}, {})'.format(episodes, num_envs))
    if S is not None and f.size and (f.min() < 0 or f.max() >= S):
        raise ValueError('first_state must hold cells in 0 .. {}'.format(S - 1))
    return np.ascontiguousarray(f, np.int32)


def _masks(masks, bits, message):
    """uint32[n] from masks (or one number) of `bits` bits each, as set_fruit_eaten and set_doors_open take them (ValueError)."""
    m = np.atleast_1d(np.asarray(masks))
    if m.ndim != 1 or m.dtype == bool or not np.issubdtype(m.dtype, np.integer) or (m.size and (m.min() < 0 or m.max() >> max(bits, 1) != 0)):
        raise ValueError(message.format(bits))
    return m.astype(np.uint32)


class VecGridUniverse(object):
    # A learner's store: its word of Engine.stores(), the Engine call that makes it, that call's arguments on first use, and the store it
    # needs first.  Nothing here remembers what the engine holds: _ensure asks.
    _STORES = {'q': ('td_rows', 'td_init', (0.0,), None), 'pairs': ('double', 'double_init', (0.0,), None),
               'model': ('dyna', 'dyna_init', (), None), 'queue': ('sweep', 'sweep_init', (), None),
               'counts': ('explore', 'explore_init', (), 'q'), 'weights': ('is', 'is_init', (), 'q'),
               'ac': ('ac', 'ac_init', (0.0, 0.0), None), 'tree': ('mcts_nodes', 'mcts_init', (1,), 'q')}

    def __init__(self, num_envs, grid_shape=(4, 4), *, initial_state=0, goal_states=None, lava_states=None,
                 walls=None, custom_world_fp=None, random_maze=False, template=None, templates=None,
                 device_mazes=None, maze_seed=0, seed=0, device=0, env_id0=0, auto_reset=False, engine_factory=Engine):
        """`template`: an existing GridUniverseEnv (or any object with the reference env's grid
        attributes) to take the grid from; otherwise the grid kwargs are validated and built
        exactly like GridUniverseEnv's (same exceptions, same RNG consumption).
        `templates=[...]`: several distinct grids of one shape, env e using grid e // (num_envs // len);
        `device_mazes=G, maze_seed=k`: G random mazes of `grid_shape` generated on the GPU."""
        self.num_envs = int(num_envs)
        if templates is not None or device_mazes is not None:
            # several distinct grids of one shape; env e uses grid e // (num_envs // n_grids)
            self.env_id0, self.auto_reset, self.info = int(env_id0), bool(auto_reset), {}
            if templates is not None:
                specs = [t if isinstance(t, GridSpec) else GridSpec.from_env(t) for t in templates]
                self.template, self.spec = templates[0], specs[0]
                self.engine = engine_factory(self.num_envs, specs[0], device=device, env_id0=env_id0, seed=seed)
                self.engine.set_grids(specs)
            else:
                # `device_mazes` random mazes carved on the GPU (csrc/gu_maze.hip) instead of one host maze
                W, H = grid_shape
                self.template = None
                self.spec = GridSpec(W, H, [0], [W * H - 1], [], [])
                self.engine = engine_factory(self.num_envs, self.spec, device=device, env_id0=env_id0, seed=seed)
                self.engine.generate_mazes(int(device_mazes), W, H, maze_seed)
            return
        if template is None:
            template = GridUniverseEnv(grid_shape, initial_state=initial_state, goal_states=goal_states,
                                       lava_states=lava_states, walls=walls, custom_world_fp=custom_world_fp,
                                       random_maze=random_maze, device=device)
        self.template = template
        self.spec = template if isinstance(template, GridSpec) else GridSpec.from_env(template)
        self.env_id0 = int(env_id0)
        self.auto_reset = bool(auto_reset)
        self.engine = engine_factory(self.num_envs, self.spec, device=device, env_id0=env_id0, seed=seed)
        self.info = {}

    # gym-like surface -----------------------------------------------------------------
    def seed(self, seed):
        self.engine.seed(seed)
        return [seed]

    def reset(self, mask=None, start_choice=None):
        """Reset all (or the masked) envs; start cell of multi-start levels from RNG stream 1
        unless `start_choice` gives an index into starting_states per env.  Returns obs int32[N]."""
        return self.engine.reset(mask, start_choice)

    def step(self, actions, zero_copy=False):
        """actions int32[N] in 0..3 -> (obs int32[N], reward int32[N], done bool[N], info).

        zero_copy=True: `actions` is copied into the engine's page-locked buffer (or pass None after filling
        `self.actions_buffer` in place) and the kernel writes the results straight into page-locked host memory;
        the returned obs / reward arrays are VIEWS that the next zero-copy step overwrites."""
        if zero_copy:
            if actions is not None:
                self.engine.pinned_actions[:] = actions
            obs, reward, done = self.engine.step_pinned(self.auto_reset)
            return obs, reward, done.astype(bool), self.info
        obs, reward, done = self.engine.step(actions, self.auto_reset)
        return obs, reward, done.astype(bool), self.info

    @property
    def actions_buffer(self):
        """int32[N] page-locked array read directly by the step kernel in zero-copy mode."""
        return self.engine.pinned_actions

    def rollout(self, T, policy='uniform', actions=None, auto_reset=None, trajectory=True, stats=False):
        """T fused steps.  policy: 'uniform' (device RNG), 'stream' (give `actions` int32[T,N]) or
        'greedy' (argmax of the policy table set through `engine.vi_set`).  Returns a dict with
        obs/reward/done int32[T,N] when `trajectory` (True, or 'packed' to move 4 instead of 12 bytes per
        env-step through HBM and PCIe), plus ret/episodes when `stats`."""
        auto = self.auto_reset if auto_reset is None else bool(auto_reset)
        if actions is not None:
            policy = 'stream'
            self.engine.upload_actions(actions)
        if trajectory:
            self.engine.reserve_trajectory(T)
        self.engine.rollout(T, policy, auto, trajectory, stats)
        if trajectory == 'packed':  # one uint32 per env-step on the device, unpacked to the same three arrays here
            return self._stats_into(self.engine.read_trajectory_packed(0, T), stats)
        return self._stats_into(self.engine.read_trajectory(0, T) if trajectory else {}, stats)

    def set_wind(self, strength, direction='up', gust=0.0):
        """Wind on the engine's grid (single-grid engines; include/gu.h: gu_set_wind): every step, the agent is pushed behind its
        action by the wind of the cell it leaves -- `strength` (0 .. 3) moves in `direction`, each by the engine's move rule, so walls
        and the border stop a push and an agent blown onto a goal or lava cell stays there.  With probability `gust` (0 .. 1) a
        strength above 0 is one more or one less for that step (2/3: one third each for k - 1, k, k + 1).  `strength` and
        `direction` as grid.wind_plane takes them; set_wind(None) calms the engine.  step, rollout and td_run follow the wind;
        the other learners, the DP and look-ahead calls, the path search and the trail are refused while it is set."""
        _unit('gust', gust)
        if strength is None:
            self.engine.set_wind(None)
            return
        self.engine.set_wind(wind_plane(self.spec.W, self.spec.H, strength, direction), _q16(gust))

    def wind(self):
        """None while the engine is calm, else dict(strength=uint8[H, W], direction=uint8[H, W], gust=float)."""
        got = self.engine.get_wind()
        if got is None:
            return None
        plane = got[0].reshape(self.spec.H, self.spec.W)
        return dict(strength=(plane >> 2) & 3, direction=plane & 3, gust=got[1] / 65536.0)

    def set_fruit(self, cells, kinds='apple', values=(1, 5, -5)):
        """Fruit on the engine's grid (single-grid engines; include/gu.h: gu_set_fruit): the first step of an episode that ends on
        a fruit cell adds the value of the fruit's kind to the step's reward; every reset grows the fruit back.  `cells` and `kinds`
        as grid.fruit_plane takes them (1 .. 32 cells, none on a wall, goal or lava cell); `values`: what an 'apple', a 'lemon' and
        a 'melon' pay, integers in -16 .. 16.  set_fruit(None) takes the fruit away.  step, rollout and td_run follow the fruit
        (td_run learns on S << F rows, one per cell and mask of eaten fruit, at most 10 fruits); the other learners, the DP and
        look-ahead calls, the path search, the trail and wind are refused while it is set.  sense and render do not show fruit."""
        if cells is None:
            self.engine.set_fruit(None)
        else:
            v = np.asarray(values)
            if v.shape != (3,) or v.dtype == bool or not np.issubdtype(v.dtype, np.integer) or v.min() < -16 or v.max() > 16:
                raise ValueError('values must be three integers in -16 .. 16 (apple, lemon, melon)')
            plane = fruit_plane(self.spec.W, self.spec.H, cells, kinds)
            blocked = (self.spec.wall | self.spec.goal | self.spec.lava) & (plane != 0)
            if blocked.any():
                raise ValueError('fruit on cell {}, which is a wall or a goal or lava cell'.format(int(np.flatnonzero(blocked)[0])))
            self.engine.set_fruit(plane, v.astype(np.int32))

    def fruit(self):
        """None while no fruit is set, else dict(cells=int64[F] ascending (index = slot), kinds=list of names, values=int32[3])."""
        got = self.engine.get_fruit()
        if got is None:
            return None
        cells = np.flatnonzero(got[0])
        names = {code: name for name, code in FRUIT_KINDS.items()}
        return dict(cells=cells, kinds=[names[int(c) >> 5] for c in got[0][cells]], values=got[1])

    def fruit_eaten(self, env0=0, n=None):
        """uint32[n]: the masks of eaten fruit of envs env0 .. env0+n-1 (to the end when n is None); bit k: the fruit of slot k
        (the k-th fruit cell in ascending order) has been eaten in the env's current episode."""
        return self.engine.get_fruit_state(env0, n)

    def set_fruit_eaten(self, eaten, env0=0):
        """Install masks uint32[n] (or one number) for envs env0 ..; no bit at or above the number of fruits."""
        self.engine.set_fruit_state(_masks(eaten, self._mask_width(2), 'eaten must hold masks of the {} fruits set'), env0)

    def set_doors(self, doors, keys=None, levers=None):
        """Doors, keys and levers on the engine's grid (single-grid engines; include/gu.h: gu_set_doors): a door of slot k refuses
        entry as a wall does while bit k of the env's mask is clear; entering a key cell of slot k sets the bit, entering a lever
        cell flips it; every reset shuts the doors again.  `doors`, `keys`, `levers` as grid.door_plane takes them (mappings slot ->
        cell or cells, slots 0 .. D-1 with D <= 8, none on a wall, goal or lava cell).  set_doors(None) takes them away.  step,
        rollout and td_run follow the doors (td_run learns on S << D rows, one per cell and mask); the other learners, the DP and
        look-ahead calls, the path search, the trail, wind and fruit are refused while they are set.  sense and render show door,
        key and lever cells as free cells."""
        if doors is None:
            if keys is not None or levers is not None:
                raise ValueError('set_doors(None) takes the doors away: keys and levers must be None too')
            self.engine.set_doors(None)
        else:
            plane = door_plane(self.spec.W, self.spec.H, doors, keys, levers)
            blocked = (self.spec.wall | self.spec.goal | self.spec.lava) & (plane != 0)
            if blocked.any():
                raise ValueError('a door, key or lever on cell {}, which is a wall or a goal or lava cell'.format(int(np.flatnonzero(blocked)[0])))
            self.engine.set_doors(plane)

    def doors(self):
        """None while no doors are set, else dict(doors=, keys=, levers=): mappings slot -> int64 array of ascending cells."""
        plane = self.engine.get_doors()
        if plane is None:
            return None
        out = {}
        for name, code in DOOR_KINDS.items():
            cells = np.flatnonzero((plane >> 4) == code)
            out[name + 's'] = {int(k): cells[(plane[cells] & 7) == k] for k in np.unique(plane[cells] & 7)}
        return out

    def doors_open(self, env0=0, n=None):
        """uint32[n]: the masks of open slots of envs env0 .. env0+n-1 (to the end when n is None); bit k: the doors of slot k are
        open for the env in its current episode."""
        return self.engine.get_doors_state(env0, n)

    def set_doors_open(self, mask, env0=0):
        """Install masks uint32[n] (or one number) for envs env0 ..; no bit at or above the number of slots in use."""
        self.engine.set_doors_state(_masks(mask, self._mask_width(3), 'mask must hold masks of the {} door slots set'), env0)

    def set_boxes(self, boxes, targets=None, on_target=5):
        """Pushable boxes on the engine's grid (single-grid engines; include/gu.h: gu_set_boxes): a box refuses entry unless the
        agent's move can push it one cell on -- not into a wall, the border, a goal or lava cell or another box --, a push onto a
        target cell adds `on_target` (0 .. 16) to the step's reward and a push off one takes it back, and the step after which every
        box stands on a target pays +10 and ends the episode.  Every reset puts the boxes back.  `boxes`, `targets` as
        grid.box_plane takes them (cells not on a wall, goal or lava cell, no box on a start cell); set_boxes(None) takes the boxes
        away.  step, rollout and td_run follow the boxes (td_run learns on S << bits rows, bits = boxes x grid.box_bits(S), at most
        10); the other learners, the DP and look-ahead calls, the path search, the trail, wind, fruit and doors are refused while
        they are set.  A box pushed into a corner ends no episode: an auto-resetting env comes back only through a goal or lava
        cell.  sense, render and the N = 1 GridUniverseEnv facade show box and target cells as free cells."""
        if boxes is None:
            if targets is not None:
                raise ValueError('set_boxes(None) takes the boxes away: targets must be None too')
            self.engine.set_boxes(None)
            return
        if isinstance(on_target, (bool, np.bool_)) or not isinstance(on_target, (int, np.integer)) or not 0 <= int(on_target) <= BOX_ON_TARGET_MAX:
            raise ValueError('on_target must be an integer in 0 .. {}'.format(BOX_ON_TARGET_MAX))
        plane = box_plane(self.spec.W, self.spec.H, boxes, targets)
        blocked = (self.spec.wall | self.spec.goal | self.spec.lava) & (plane != 0)
        if blocked.any():
            raise ValueError('a box or target on cell {}, which is a wall or a goal or lava cell'.format(int(np.flatnonzero(blocked)[0])))
        on_start = [s for s in self.spec.starts if plane[s] & BOX_INITIAL]
        if on_start:
            raise ValueError('a box on cell {}, which is a start cell'.format(on_start[0]))
        self.engine.set_boxes(plane, int(on_target))

    def boxes(self):
        """None while no boxes are set, else dict(boxes=int64[B] ascending (index = box), targets=int64 ascending, on_target=int)."""
        got = self.engine.get_boxes()
        if got is None:
            return None
        return dict(boxes=np.flatnonzero(got[0] & BOX_INITIAL), targets=np.flatnonzero(got[0] & BOX_TARGET), on_target=got[1])

    def box_cells(self, env0=0, n=None):
        """int32[n, B]: the cells of the B boxes of envs env0 .. env0+n-1 (to the end when n is None); box k is the one that began
        on the k-th initial cell in ascending order."""
        got = self.engine.get_boxes()
        if got is None:
            raise ValueError('no boxes set: call set_boxes first')
        return unpack_boxes(self.spec.S, self.engine.get_boxes_state(env0, n), got[2])

    def set_box_cells(self, cells, env0=0):
        """Install the box cells int[n, B] (or [B] for one env) of envs env0 ..: distinct cells, none on a wall, goal or lava cell."""
        c = np.asarray(cells)
        B = self._mask_width(4) // box_bits(self.spec.S)
        if not B:
            raise ValueError('no boxes set: call set_boxes first')
        if c.ndim not in (1, 2) or c.shape[-1] != B:
            raise ValueError('cells must hold the cells of the {} boxes set, shape (n, {})'.format(B, B))
        words = np.atleast_1d(pack_boxes(self.spec.S, c))
        blocked = (self.spec.wall | self.spec.goal | self.spec.lava)[c.reshape(-1)]
        if blocked.any():
            raise ValueError('a box on cell {}, which is a wall or a goal or lava cell'.format(int(c.reshape(-1)[np.flatnonzero(blocked)[0]])))
        self.engine.set_boxes_state(words, env0)

    def set_errands(self, cells, kinds='apple', instructions=None, right=5, wrong=-8, finish=10):
        """Errands on the engine's grid (single-grid engines; include/gu.h: gu_set_errands): fruit on `cells` of `kinds`, as
        grid.fruit_plane takes them (1 .. 8 cells, none on a wall, goal or lava cell), and 1 .. 4 `instructions`, each a string
        ('collect the lemon and then the apple': grid.parse_instruction) or a list of 1 .. 4 kind names.  Every reset gives the env
        one of the instructions (RNG stream 11) and grows the fruit back.  A fruit eaten in the instruction's order adds `right`
        (0 .. 16) to the step's reward, any other fruit adds `wrong` (-16 .. 0) and is gone; the step that eats the instruction's last
        entry pays `finish` (0 .. 16) and ends the episode.  An instruction may name a kind at most as often as there is fruit of it.
        set_errands(None) takes the errands away.  step, rollout and td_run follow the errands (td_run learns on S << bits rows, bits
        = F + bits of the progress + bits of the instruction index, at most 10); everything refused under fruit is refused while
        they are set.  sense and render show fruit cells as free cells."""
        if cells is None:
            self.engine.set_errands(None)
            return
        pay = (right, wrong, finish)
        if any(isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) for v in pay) or not (0 <= right <= 16 and -16 <= wrong <= 0 and 0 <= finish <= 16):
            raise ValueError('right must be an integer in 0 .. 16, wrong in -16 .. 0 and finish in 0 .. 16')
        if instructions is None:
            raise ValueError('instructions: 1 .. 4 of them, each a string or a list of kind names')
        instr = errand_bytes(instructions)
        plane = fruit_plane(self.spec.W, self.spec.H, cells, kinds)
        if np.count_nonzero(plane) > ERRAND_FRUIT_MAX:
            raise ValueError('1 .. {} fruit cells, got {}'.format(ERRAND_FRUIT_MAX, int(np.count_nonzero(plane))))
        blocked = (self.spec.wall | self.spec.goal | self.spec.lava) & (plane != 0)
        if blocked.any():
            raise ValueError('fruit on cell {}, which is a wall or a goal or lava cell'.format(int(np.flatnonzero(blocked)[0])))
        have = np.bincount((plane[plane != 0] >> 5) & 3, minlength=4)
        for j in range(len(instructions)):
            named = np.bincount([(int(instr[j]) >> (2 * p)) & 3 for p in range(4)], minlength=4)
            if (named[1:] > have[1:]).any():
                raise ValueError('instruction {} names a kind more often than there is fruit of it'.format(j))
        self.engine.set_errands(plane, instr, len(instructions), np.array(pay, np.int32))

    def errands(self):
        """None while no errands are set, else dict(cells=int64[F] ascending (index = slot), kinds=list of names, instructions=list of
        lists of kind names, right=, wrong=, finish=)."""
        got = self.engine.get_errands()
        if got is None:
            return None
        plane, instr, n, pay, _ = got
        cells = np.flatnonzero(plane)
        names = {code: name for name, code in FRUIT_KINDS.items()}
        lists = [[names[(int(instr[j]) >> (2 * p)) & 3] for p in range(4) if (int(instr[j]) >> (2 * p)) & 3] for j in range(n)]
        return dict(cells=cells, kinds=[names[int(c) >> 5] for c in plane[cells]], instructions=lists, right=int(pay[0]), wrong=int(pay[1]), finish=int(pay[2]))

    def errand_state(self, env0=0, n=None):
        """dict(eaten=uint32[n], progress=uint32[n], instruction=uint32[n]) of envs env0 .. env0+n-1 (to the end when n is None): the
        mask of eaten fruit (bit k: the k-th fruit cell in ascending order), how many entries of its instruction the env has carried
        out, and which instruction its last reset gave it."""
        got = self.errands()
        if got is None:
            raise ValueError('no errands set: call set_errands first')
        e, p, j = errand_fields(self.engine.get_errands_state(env0, n), len(got['cells']), got['instructions'])
        return dict(eaten=e, progress=p, instruction=j)

    def set_errand_state(self, eaten=0, progress=0, instruction=0, env0=0):
        """Install the three fields (arrays of one length n, or single numbers) for envs env0 ..: no bit of `eaten` at or above the
        number of fruits, `instruction` below the number of instructions, `progress` at most that instruction's length."""
        got = self.errands()
        if got is None:
            raise ValueError('no errands set: call set_errands first')
        F, lists = len(got['cells']), got['instructions']
        try:
            e, p, j = np.broadcast_arrays(*(np.atleast_1d(np.asarray(x)) for x in (eaten, progress, instruction)))
        except ValueError:
            raise ValueError('eaten, progress and instruction must be of one length')
        for x in (e, p, j):
            if x.ndim != 1 or x.dtype == bool or not np.issubdtype(x.dtype, np.integer) or (x.size and x.min() < 0):
                raise ValueError('eaten, progress and instruction must be non-negative integers, one per env')
        if e.size and (e.max() >> F or j.max() >= len(lists) or (p > np.array([len(k) for k in lists])[j]).any()):
            raise ValueError('eaten must hold masks of the {} fruits set, instruction an index below {} and progress at most its length'.format(F, len(lists)))
        self.engine.set_errands_state(errand_words(e, p, j, F, lists), env0)

    def _mask_width(self, overlay):
        """Bits of an env's mask in use while `overlay` (2 fruit, 3 doors, 4 boxes, 5 errands: include/gu.h, GU_STORE_OVERLAY) is set, else 0."""
        st = self.engine.stores()
        return st['overlay_bits'] if st['overlay'] == overlay else 0

    def _ensure(self, st, store, *values, again=False):
        """`store` (a key of _STORES) on the engine whose stores() are `st`: made with its first-use arguments when the library does
        not hold it for the current grid and rows, made again when `again` or one of `values` is given (None: the first-use one)."""
        word, init, first_use, needs = self._STORES[store]
        if needs:
            self._ensure(st, needs)
        # `st` is read once and may be older than an init made since: that is safe because no init drops another store.  Without
        # `values` the call takes its first-use arguments; a value of None stands for the first-use one at its place.
        if again or any(v is not None for v in values) or not st[word]:
            getattr(self.engine, init)(*[d if v is None else v for d, v in zip(first_use, values or first_use)])

    def _ensure_q(self, q0=None):
        """Q tables on the engine: tables of zeros on first use; every entry q0 (again) when q0 is given."""
        self._ensure(self.engine.stores(), 'q', q0)

    def _ensure_model(self, clear=False):
        """Dyna-Q models on the engine: an empty model per env on first use, or when `clear`."""
        self._ensure(self.engine.stores(), 'model', again=clear)

    def _stats_into(self, out, stats):
        """`out`, the rows of the launch just made, with its statistics beside them when `stats`."""
        if stats:
            out['ret'], out['episodes'] = self.engine.read_stats()
        return out

    def _learner_out(self, T, trajectory, stats):
        """The rows and statistics of the learner launch just made, as rollout() returns them."""
        return self._stats_into(self.engine.read_trajectory(0, T) if trajectory and T > 0 else {}, stats)

    def _learner_launch(self, run, T, trajectory, stats, *args):
        """One learner launch `run(T, *args, trajectory, stats)` of the engine, with room for its rows reserved before it and
        its rows and statistics read behind it."""
        if trajectory:
            self.engine.reserve_trajectory(T)
        run(T, *args, trajectory, stats)
        return self._learner_out(T, trajectory, stats)

    def td_run(self, T, method='q_learning', alpha=0.1, discount_factor=0.99, epsilon=0.1, trajectory=False, stats=False):
        """T iterations of batched tabular Q-learning ('q_learning') or SARSA ('sarsa'): env e learns its own Q table [S][4]
        from its own experience, epsilon-greedy, auto-reset always on (include/gu.h: gu_td_run).  The first call gives every
        env a table of zeros.  Returns a dict like rollout(): obs/reward/done int32[T, N] when `trajectory`, ret/episodes
        when `stats`."""
        self._ensure_q()
        return self._learner_launch(self.engine.td_run, T, trajectory, stats, method, alpha, discount_factor, _q16(epsilon))

    def q_table(self, env0=0, n=None):
        """float64[n, S, 4]: the Q tables of envs env0 .. env0+n-1 (to the end when n is None).  While F fruits are set
        (set_fruit) the tables have S << F rows: row eaten * S + s belongs to cell s with the mask `eaten`.  While doors with D slots
        are set (set_doors) they have S << D rows: row open * S + s belongs to cell s under the mask `open`.  While B boxes are set
        (set_boxes) they have S << (b * B) rows, b = grid.box_bits(S): row word * S + s belongs to cell s under the word
        grid.pack_boxes(S, cells)."""
        return self.engine.td_get_q(env0, n)

    def set_q_table(self, q, env0=0):
        """Install Q tables float64[n, S, 4] (or [S, 4]) for envs env0 ..; the other envs get tables of zeros if they had none.
        S << F rows while F fruits are set and S << D rows while doors with D slots are set, as q_table()."""
        self._ensure_q()
        self.engine.td_set_q(q, env0)

    def evaluate(self, episodes=1, max_steps=None, discount_factor=1.0, first_state=None):
        """`episodes` greedy test episodes of at most `max_steps` steps per env on its own Q table, with the move rule the learners
        use, the overlay's included (include/gu.h: gu_td_evaluate).  Nothing learns, and the envs, what the learners carry, rows and
        statistics stay as they are.  Test episode k starts where a reset at episode count k puts a freshly seeded env, or on
        first_state[k][e] (int [episodes, N]); every step takes the first maximum of the row (np.argmax).  max_steps None: the rows of
        a table (a greedy walk without gusts that has not ended by then is in a loop), clipped to the budget of 1e8 // episodes.
        Returns a dict of [episodes, N] arrays: ret (int32), length (int32), outcome (int32: 0 ran to max_steps, 1 reached a goal,
        2 ended on another terminal cell, 3 ended by the overlay: boxes solved, errand completed), end (int32, the last cell), word
        (uint32, the last overlay word) and discounted (float64).  The first call gives every env a table of zeros."""
        first_state = check_evaluate_args(episodes, max_steps, discount_factor, first_state, self.num_envs, self.spec.S)
        self._ensure_q()
        if max_steps is None:
            max_steps = max(1, min(self.engine.td_rows, _lib.EVAL_BUDGET // int(episodes)))
        out = self.engine.td_evaluate(episodes, max_steps, discount_factor, first_state)
        return dict(ret=out['ret'], length=out['len'], outcome=out['outcome'], end=out['end'], word=out['word'], discounted=out['disc'])

    def expected_sarsa_run(self, T, alpha=0.1, discount_factor=0.99, epsilon=0.1, trajectory=False, stats=False):
        """T iterations of batched tabular Expected SARSA (Sutton & Barto 6.6) on the tables of td_run: env e acts epsilon-greedily
        as Q-learning does and bootstraps on the mean of Q[s'] under that same policy (include/gu.h: gu_esarsa_run); epsilon = 0
        gives td_run('q_learning')'s bytes.  The first call gives every env a table of zeros.  Refused while wind, fruit or doors are
        set.  Rows and statistics as td_run()."""
        _unit('epsilon', epsilon)
        self._ensure_q()
        return self._learner_launch(self.engine.esarsa_run, T, trajectory, stats, alpha, discount_factor, _q16(epsilon))

    def _ensure_pairs(self, q0=None):
        """Pairs of Q tables on the engine: two tables of zeros per env on first use; every entry q0 (again) when q0 is given."""
        self._ensure(self.engine.stores(), 'pairs', q0)

    def double_q_run(self, T, alpha=0.1, discount_factor=0.99, epsilon=0.1, trajectory=False, stats=False):
        """T iterations of batched tabular Double Q-learning (Sutton & Barto 6.7): env e keeps two tables A and B of its own (not
        the tables of td_run), acts epsilon-greedily on A + B, and a coin per step (RNG stream 10) picks the table that learns, from
        the other's estimate of its own greedy action at s' (include/gu.h: gu_double_run).  The first call gives every env two
        tables of zeros.  Refused while wind, fruit or doors are set.  Rows and statistics as td_run()."""
        _unit('epsilon', epsilon)
        self._ensure_pairs()
        return self._learner_launch(self.engine.double_run, T, trajectory, stats, alpha, discount_factor, _q16(epsilon))

    def double_q_tables(self, env0=0, n=None):
        """float64[n, S, 2, 4]: the pairs of envs env0 .. env0+n-1 (to the end when n is None); [:, :, 0] is A, [:, :, 1] is B; zeros
        before the first double_q_run."""
        self._ensure_pairs()
        return self.engine.double_get_q(env0, n)

    def set_double_q_tables(self, q, env0=0):
        """Install pairs float64[n, S, 2, 4] (or [S, 2, 4]) for envs env0 ..; the other envs get tables of zeros if they had none."""
        self._ensure_pairs()
        self.engine.double_set_q(q, env0)

    def dyna_run(self, T, planning_steps=10, alpha=0.1, discount_factor=0.99, epsilon=0.1, trajectory=False, stats=False):
        """T real steps of batched tabular Dyna-Q: env e learns its own Q table [S][4] with Q-learning and its own model of the
        env, and replays `planning_steps` model updates after every real step (include/gu.h: gu_dyna_run).  The first call gives
        every env a table of zeros (if it had none) and an empty model.  Rows and statistics cover the real steps, as td_run()."""
        st = self.engine.stores()
        self._ensure(st, 'q')
        self._ensure(st, 'model')
        return self._learner_launch(self.engine.dyna_run, T, trajectory, stats, planning_steps, alpha, discount_factor, _q16(epsilon))

    def model(self, env0=0, n=None):
        """The Dyna-Q models of envs env0 .. env0+n-1 (Engine.dyna_get_model); an empty model is allocated on first use."""
        self._ensure_model()
        return self.engine.dyna_get_model(env0, n)

    def _ensure_queue(self):
        """Priority queues (and Dyna-Q models) on the engine: empty ones on first use."""
        self._ensure(self.engine.stores(), 'queue')

    def sweep_run(self, T, planning_steps=10, theta=1e-4, alpha=0.1, discount_factor=0.99, epsilon=0.1, trajectory=False, stats=False):
        """T real steps of batched tabular prioritized sweeping (Sutton & Barto 8.4): env e keeps its own Q table, its own model of
        the env (dyna_run's) and its own priority queue.  A real step learns nothing by itself: its pair is queued under its
        |TD error| when that exceeds `theta`, and up to `planning_steps` times the pair with the largest priority is updated from the
        model and its predecessors are queued (include/gu.h: gu_sweep_run).  The first call gives every env a table of zeros (if
        it had none), an empty model and an empty queue.  Rows and statistics cover the real steps, as td_run()."""
        st = self.engine.stores()
        self._ensure(st, 'q')
        self._ensure(st, 'queue')
        return self._learner_launch(self.engine.sweep_run, T, trajectory, stats, planning_steps, theta, alpha, discount_factor, _q16(epsilon))

    def priority_queue(self, env0=0, n=None):
        """The priority queues of envs env0 .. env0+n-1: dict key uint64[n, S, 4] (0 = not queued), priority float64[n, S, 4] (the
        key with its low 16 bits, the pair index, cleared; 0.0 where the pair is not queued) and size int32[n]."""
        self._ensure_queue()
        out = self.engine.sweep_get_queue(env0, n)
        out['priority'] = (out['key'] & ~np.uint64(0xFFFF)).view(np.float64)
        return out

    def search_run(self, T, simulations=4, depth=16, alpha=0.1, discount_factor=0.99, epsilon=0.1, rollout_epsilon=1.0, trajectory=False,
                   stats=False):
        """T real steps of batched simulation-based search (Monte-Carlo rollouts at decision time): before each non-exploring
        real move, env e simulates `simulations` (0 .. 64) rollouts of `depth` (0 .. 256) moves per action with the true model, under
        an epsilon-greedy rollout policy on its own Q table (`rollout_epsilon`; 1.0 = uniformly random), bootstraps a truncated
        rollout on max Q at its leaf, takes the action with the largest summed return and learns from the real transition by
        Q-learning (include/gu.h: gu_search_run).  An exploring step (`epsilon`) simulates nothing; simulations = 0 is
        td_run('q_learning').  The first call gives every env a table of zeros.  Rows and statistics cover the real steps, as
        td_run()."""
        _unit('epsilon', epsilon)
        _unit('rollout_epsilon', rollout_epsilon)
        self._ensure_q()
        return self._learner_launch(self.engine.search_run, T, trajectory, stats, simulations, depth, alpha, discount_factor, _q16(epsilon),
                                    _q16(rollout_epsilon))

    def search_scores(self, env0=0, n=None):
        """Engine.search_get: the score rows of the most recent searched steps and the simulated moves of the last search_run."""
        self._ensure_q()
        return self.engine.search_get(env0, n)

    def set_tree_search(self, U, B, I):
        """The schedule of tree_search_run: float64 vectors U, B and I of one length C, 2 <= C <= 4096, finite and >= 0.  At a node
        visited n_s times, an action tried n_b times with summed returns w_b scores w_b * I[min(n_b, C-1)] + U[min(n_s, C-1)] *
        B[min(n_b, C-1)]; algorithms.search.uct_tables builds UCB1's."""
        self.engine.set_tree_tables(U, B, I)

    def tree_search_run(self, T, simulations=64, tree_depth=8, depth=4, alpha=0.1, discount_factor=0.99, epsilon=0.1, rollout_epsilon=1.0,
                        trajectory=False, stats=False):
        """T real steps of batched Monte-Carlo tree search (UCT at decision time): before each non-exploring real move, env e
        builds a search tree at its state by `simulations` (0 .. 255) simulations with the true model -- UCB1 selection down to
        `tree_depth` (1 .. 64) levels, one new node, a rollout of `depth` (0 .. 256) moves under an epsilon-greedy policy on its own
        Q table (`rollout_epsilon`; 1.0 = uniformly random) that bootstraps on max Q at its leaf, and a backup --, takes the root
        action with the largest mean return and learns from the real transition by Q-learning (include/gu.h: gu_mcts_run).  An
        exploring step (`epsilon`) simulates nothing; simulations = 0 is td_run('q_learning').  The first call gives every env a
        table of zeros and a node pool, and installs uct_tables(3.0) unless set_tree_search was called.  Rows and statistics
        cover the real steps, as td_run()."""
        _unit('epsilon', epsilon)
        _unit('rollout_epsilon', rollout_epsilon)
        M = int(simulations)
        if not 0 <= M <= _lib.MCTS_MAX_SIMS:
            raise ValueError('simulations must lie in 0 .. {}'.format(_lib.MCTS_MAX_SIMS))
        st = self.engine.stores()
        self._ensure(st, 'q')
        # a pool holds one node more than its simulations (no pool: 0 nodes).  Under an overlay none is made: the launch is refused, and
        # says why, where mcts_init would only miss tables of S rows
        if M > st['mcts_nodes'] - 1 and not st['overlay']:
            self.engine.mcts_init(max(M, 1))
        if not st['mcts_c']:
            from .algorithms.search import uct_tables
            self.set_tree_search(*uct_tables())
        return self._learner_launch(self.engine.mcts_run, T, trajectory, stats, M, tree_depth, depth, alpha, discount_factor, _q16(epsilon),
                                    _q16(rollout_epsilon))

    def _ensure_tree(self):
        self._ensure(self.engine.stores(), 'tree')

    def tree_search_roots(self, env0=0, n=None):
        """Engine.mcts_get: the root rows (return sums, visits) and node counts of the most recent searched steps and the simulated
        moves of the last tree_search_run."""
        self._ensure_tree()
        return self.engine.mcts_get(env0, n)

    def tree_search_tree(self, env0=0, n=None):
        """Engine.mcts_tree: the whole trees of the most recent searched steps."""
        self._ensure_tree()
        return self.engine.mcts_tree(env0, n)

    def _ensure_counts(self):
        """Visit counts on the engine: zeroed counts on first use (and tables of zeros if the envs had no Q tables)."""
        self._ensure(self.engine.stores(), 'counts')

    def set_exploration(self, U, B):
        """The exploration schedule of explore_run: float64 vectors U and B of one length C, 2 <= C <= 4096, finite and >= 0.  The
        bonus of action b in a state visited n_s times is U[min(n_s, C-1)] * B[min(n_b, C-1)]; algorithms.exploration.ucb_tables
        and thompson_tables build the two usual schedules."""
        self.engine.set_exploration(U, B)

    def explore_run(self, T, rule='ucb', alpha=0.1, discount_factor=0.99, epsilon=0.0, trajectory=False, stats=False):
        """T steps of batched tabular Q-learning with count-based exploration: env e keeps visit counts [S][4] beside its Q table
        and takes, where it does not explore by `epsilon`, the action that maximises Q + bonus ('ucb') or Q + bonus * noise
        ('thompson': four approximate normals per step from RNG stream 7), the bonus from its counts and the set_exploration
        tables (include/gu.h: gu_explore_run).  The update is td_run('q_learning')'s: the bonus never enters the table.  The
        first call gives every env zeroed counts (and a table of zeros if it had none).  Rows and statistics as td_run()."""
        if rule not in ('ucb', 'thompson'):
            raise ValueError("rule must be 'ucb' or 'thompson'")
        _unit('epsilon', epsilon)
        st = self.engine.stores()
        if not st['explore_c']:
            raise ValueError('no exploration schedule: call set_exploration(U, B) first')
        self._ensure(st, 'counts')
        return self._learner_launch(self.engine.explore_run, T, trajectory, stats, rule, alpha, discount_factor, _q16(epsilon))

    def visit_counts(self, env0=0, n=None):
        """uint32[n, S, 4]: the visit counts of envs env0 .. env0+n-1 (to the end when n is None); zeros before the first explore_run."""
        self._ensure_counts()
        return self.engine.explore_get_counts(env0, n)

    def set_visit_counts(self, counts, env0=0):
        """Install visit counts uint32[n, S, 4] (or [S, 4]) for envs env0 ..; no value above 0x3FFFFFFF, where the counts saturate."""
        self._ensure_counts()
        self.engine.explore_set_counts(counts, env0)

    def nstep_run(self, T, n=4, method='sarsa', alpha=0.1, discount_factor=0.99, epsilon=0.1, trajectory=False, stats=False):
        """T iterations of batched tabular n-step SARSA ('sarsa') or n-step Q-learning ('q_learning'), 1 <= n <= 16: env e learns
        its own Q table [S][4] from n-step returns (include/gu.h: gu_nstep_run).  The first call gives every env a table of zeros.
        Consecutive calls with the same method and n carry the window of pending transitions; any other call in between drops
        it.  Rows and statistics as td_run()."""
        self._ensure_q()
        return self._learner_launch(self.engine.nstep_run, T, trajectory, stats, method, n, alpha, discount_factor, _q16(epsilon))

    def nstep_window(self, env0=0, n=None):
        """The n-step windows of envs env0 .. env0+n-1 (Engine.nstep_get_window)."""
        return self.engine.nstep_get_window(env0, n)

    def lambda_run(self, T, lam=0.9, trace_len=32, method='sarsa', alpha=0.1, discount_factor=0.99, epsilon=0.1, trajectory=False,
                   stats=False):
        """T iterations of batched tabular SARSA(lambda) ('sarsa') or Watkins's Q(lambda) ('q_learning'): env e learns its own Q
        table [S][4] with replacing eligibility traces, truncated after `trace_len` (1 .. 64) steps (include/gu.h: gu_lambda_run).
        The first call gives every env a table of zeros.  Consecutive calls with the same method and trace_len carry the trace
        window; any other call in between drops it.  Rows and statistics as td_run()."""
        self._ensure_q()
        return self._learner_launch(self.engine.lambda_run, T, trajectory, stats, method, trace_len, lam, alpha, discount_factor, _q16(epsilon))

    def lambda_window(self, env0=0, n=None):
        """The trace windows of envs env0 .. env0+n-1 (Engine.lambda_get_window): int32[n, 64], index = age."""
        return self.engine.lambda_get_window(env0, n)

    def set_features(self, phi, n_features=None, w0=0.0):
        """Install the feature table phi int32[S, K] (K active binary features per state, K <= 8; column k is a slot of its own,
        as a tiling of tile coding is) shared by all envs, and give every env a weight table [F][4] of w0
        (include/gu.h: gu_fa_init).  F = n_features, or phi.max() + 1.  See algorithms.function_approximation.tile_coding."""
        self.engine.fa_init(phi, n_features, w0)

    def _need_features(self):
        if not self.engine.stores()['fa_f']:
            raise RuntimeError('no features: call set_features first')

    def fa_run(self, T, method='sarsa', alpha=0.1, discount_factor=0.99, epsilon=0.1, trajectory=False, stats=False):
        """T iterations of batched episodic semi-gradient SARSA ('sarsa') or semi-gradient Q-learning ('q_learning') on the
        features of set_features: env e learns its own weights [F][4], its action values being the sum of the K weight rows
        active in a state, epsilon-greedy, auto-reset always on (include/gu.h: gu_fa_run).  `alpha` is applied as given: divide
        a step size by K yourself.  Returns a dict like td_run()."""
        self._need_features()
        return self._learner_launch(self.engine.fa_run, T, trajectory, stats, method, alpha, discount_factor, _q16(epsilon))

    def weights(self, env0=0, n=None):
        """float64[n, F, 4]: the weight tables of envs env0 .. env0+n-1 (to the end when n is None)."""
        self._need_features()
        return self.engine.fa_get_w(env0, n)

    def set_weights(self, w, env0=0):
        """Install weights float64[n, F, 4] (or [F, 4]) for envs env0 .. ."""
        self._need_features()
        self.engine.fa_set_w(w, env0)

    def fa_q_table(self, env0=0, n=None):
        """float64[n, S, 4]: the action values of envs env0 .. env0+n-1 computed from their weights on the device, in the
        format of q_table()."""
        self._need_features()
        return self.engine.fa_get_q(env0, n)

    def _ensure_ac(self, h0=None, v0=None):
        """Actor-critic tables on the engine: zeros on first use; every entry h0 / v0 (again) when either is given."""
        self._ensure(self.engine.stores(), 'ac', h0, v0)

    def actor_critic_run(self, T, actor_lr=0.1, critic_lr=0.1, discount_factor=0.99, trajectory=False, stats=False):
        """T iterations of batched tabular one-step actor-critic: env e learns its own softmax preferences [S][4] and state
        values [S] from its own experience, acting on the softmax of its preferences, auto-reset always on (include/gu.h:
        gu_ac_run).  The first call gives every env tables of zeros.  Returns a dict like td_run()."""
        self._ensure_ac()
        return self._learner_launch(self.engine.ac_run, T, trajectory, stats, actor_lr, critic_lr, discount_factor)

    def reinforce_run(self, T, max_episode_len=256, actor_lr=0.003, baseline_lr=0.1, discount_factor=0.99, trajectory=False,
                      stats=False):
        """T iterations of batched tabular REINFORCE with baseline (Monte-Carlo policy gradient): env e acts on the softmax of
        its own preferences [S][4] and learns them, and its state values [S] as the baseline, from whole-episode returns in a
        backward pass when its episode ends; an episode still running after `max_episode_len` (1 .. 1024) steps is cut there and
        its return bootstraps on the baseline (include/gu.h: gu_reinforce_run).  The tables are actor_critic_run's; the first
        call gives every env tables of zeros.  Consecutive calls with the same max_episode_len carry the episode buffer; any
        other call in between drops it.  Returns a dict like td_run()."""
        self._ensure_ac()
        return self._learner_launch(self.engine.reinforce_run, T, trajectory, stats, max_episode_len, actor_lr, baseline_lr, discount_factor)

    def episode_buffer(self, env0=0, n=None):
        """The episode buffers of envs env0 .. env0+n-1 (Engine.reinforce_get_episode)."""
        return self.engine.reinforce_get_episode(env0, n)

    def _ensure_is(self):
        """Cumulative weights on the engine: zeros on first use (and tables of zeros if the envs had no Q tables)."""
        self._ensure(self.engine.stores(), 'weights')

    def off_policy_mc_run(self, T, max_episode_len=64, discount_factor=0.99, epsilon=0.1, w_cap=2.0 ** 64, trajectory=False,
                          stats=False):
        """T iterations of batched off-policy every-visit Monte-Carlo control with weighted importance sampling (Sutton & Barto
        5.7): env e acts epsilon-greedily on its own Q table [S][4] and, when its episode ends, walks it backwards, learning
        the GREEDY policy's values from returns weighted by the importance ratio, up to the first action that is no longer
        greedy; an episode still running after `max_episode_len` (1 .. 1024) steps is cut there and its return bootstraps on
        max Q (include/gu.h: gu_is_run).  A pass also ends where its weight reaches `w_cap` (1 .. 2^256).  The Q tables are
        td_run's; the first call gives every env tables of zeros and zeroed cumulative weights.  Consecutive calls with the same
        max_episode_len carry the episode buffer; any other call in between drops it.  Returns a dict like td_run()."""
        check_off_policy_args(max_episode_len, epsilon, w_cap)
        self._ensure_is()
        return self._learner_launch(self.engine.is_run, T, trajectory, stats, max_episode_len, discount_factor, _q16(epsilon), w_cap)

    def importance_weights(self, env0=0, n=None):
        """float64[n, S, 4]: the cumulative weights C of envs env0 .. env0+n-1 (to the end when n is None); zeros before the
        first off_policy_mc_run."""
        self._ensure_is()
        return self.engine.is_get(env0, n)

    def set_importance_weights(self, c, env0=0):
        """Install cumulative weights float64[n, S, 4] (or [S, 4]) for envs env0 ..: finite and not negative."""
        self._ensure_is()
        self.engine.is_set(c, env0)

    def off_policy_episode_buffer(self, env0=0, n=None):
        """The episode buffers of off_policy_mc_run of envs env0 .. env0+n-1 (Engine.is_get_episode)."""
        return self.engine.is_get_episode(env0, n)

    def preferences(self, env0=0, n=None):
        """float64[n, S, 4]: the actor's preference tables of envs env0 .. env0+n-1 (to the end when n is None)."""
        self._ensure_ac()
        return self.engine.ac_get(env0, n)[0]

    def state_values(self, env0=0, n=None):
        """float64[n, S]: the critic's state values of envs env0 .. env0+n-1 (to the end when n is None)."""
        self._ensure_ac()
        return self.engine.ac_get(env0, n)[1]

    def set_actor_critic(self, h=None, v=None, env0=0):
        """Install preferences float64[n, S, 4] and / or values float64[n, S] for envs env0 ..; the other envs get tables of
        zeros if they had none."""
        self._ensure_ac()
        self.engine.ac_set(h, v, env0)

    def softmax_policy(self, env0=0, n=None):
        """float64[n, S, 4]: the softmax policy pi of envs env0 .. env0+n-1, computed on the host with the same bytes as the
        device's (griduniverse_amd.softmax)."""
        return softmax.softmax_policy(self.preferences(env0, n))

    def sense(self, radius=1, mode='ego', env0=0, n=None):
        """What the agents see from where they stand: uint8[n, K, K] egocentric views of radius 0 .. 7 (K = 2 * radius + 1; entry
        [dy, dx] is the class of the cell dy - radius rows and dx - radius columns from the agent: 0 ground, 1 wall, 2 lava,
        3 goal, 4 outside the grid), or -- mode='grid' -- uint8[n, H, W], the class of every cell plus 8 on the agent's, for envs
        env0 .. env0+n-1 (to the end when n is None).  Computed on the device (include/gu.h: gu_sense)."""
        return self.engine.sense(env0, n, radius, mode)

    def sense_trajectory(self, T, radius=1, mode='ego', t0=0):
        """uint8[T, N, K, K] or uint8[T, N, H, W]: the same views along rows t0 .. t0+T-1 of the last rollout(trajectory=True) or
        learner launch with trajectory=True, seen from each row's obs.  Packed rows (trajectory='packed') are refused."""
        return self.engine.sense_trajectory(t0, T, radius, mode)

    def done_indices(self):
        return self.engine.done_indices()

    def get_state(self):
        return self.engine.get_state()

    def set_state(self, **kw):
        self.engine.set_state(**kw)

    def close(self):
        self.engine.close()

    @property
    def observations(self):
        return self.engine.read_outputs()[0]
