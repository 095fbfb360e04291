"""GridSpec: the reference's per-instance grid attributes -> row bit-planes for libgu.

The reference keeps a grid as Python lists and numpy arrays on the env instance
(core/envs/griduniverse_env.py:61-90: starting_states, goal_states, lava_states,
wall_grid, reward_matrix).  The engine wants them as `uint32[H][ceil(W/32)]` row
bit-planes (include/gu.h: gu_set_grid), bit (x & 31) of word (x >> 5) of row y for
cell s = y*W + x.  Five planes: wall, goal membership, lava membership, and the two
reward planes R == +10 / R == -10 (the reward matrix and the terminal test can
disagree in the reference -- negative indices wrap only in the former, SURVEY.md
8(a) quirk 5 -- so the reward planes are taken from reward_matrix itself).
"""
import numpy as np


def _row_planes(flags, W, H):
    """bool[S] -> uint32[H, ceil(W/32)]"""
    wpr = (W + 31) // 32
    padded = np.zeros((H, wpr * 32), dtype=np.uint8)
    padded[:, :W] = np.asarray(flags, dtype=np.uint8).reshape(H, W)
    weights = (np.uint64(1) << np.arange(32, dtype=np.uint64))
    words = (padded.reshape(H, wpr, 32).astype(np.uint64) * weights).sum(axis=2)
    return np.ascontiguousarray(words.astype(np.uint32))


def _membership(indices, S):
    """`s in indices` for s in range(S) -- Python equality, so out-of-range or negative
    entries simply never match (env:170-174)."""
    flags = np.zeros(S, dtype=bool)
    for i in indices:
        if isinstance(i, (int, np.integer)) and 0 <= int(i) < S:
            flags[int(i)] = True
    return flags


class GridSpec(object):
    def __init__(self, W, H, starts, goals, lava, walls, reward=None):
        self.W, self.H = int(W), int(H)
        self.S = self.W * self.H
        if self.W <= 0 or self.H <= 0:
            raise ValueError('grid must have at least one cell, got {}x{}'.format(W, H))
        self.starts = [int(s) for s in starts]
        if not self.starts:
            raise ValueError('at least one starting state is required')
        for s in self.starts:
            if not 0 <= s < self.S:
                raise ValueError('starting state {} is outside the {}x{} grid'.format(s, W, H))
        self.wall = _membership(walls, self.S)
        self.goal = _membership(goals, self.S)
        self.lava = _membership(lava, self.S)
        if reward is None:  # env:80-90
            r = np.full(self.S, -1, dtype=np.int64)
            r[self.goal] = 10
            r[self.lava] = -10
        else:
            r = np.asarray(reward, dtype=np.int64).reshape(self.S)
            if not np.isin(r, (-1, 10, -10)).all():
                raise ValueError('reward_matrix may only hold -1, +10 and -10 (env:80-90)')
        self.reward = r

    @classmethod
    def from_env(cls, env):
        """From any object exposing the reference env's attributes."""
        return cls(env.x_max, env.y_max, env.starting_states, env.goal_states, env.lava_states,
                   np.flatnonzero(np.asarray(env.wall_grid) == 1).tolist(), np.asarray(env.reward_matrix))

    @property
    def words_per_row(self):
        return (self.W + 31) // 32

    def planes(self):
        W, H = self.W, self.H
        return dict(wall=_row_planes(self.wall, W, H), goal=_row_planes(self.goal, W, H),
                    lava=_row_planes(self.lava, W, H), rplus=_row_planes(self.reward == 10, W, H),
                    rminus=_row_planes(self.reward == -10, W, H))

    def key(self):
        return (self.W, self.H, tuple(self.starts), self.wall.tobytes(), self.goal.tobytes(),
                self.lava.tobytes(), self.reward.tobytes())


# ---- agent sensors: the host mirror of csrc/gu_sense.hip (include/gu.h: gu_sense) ----------------------------------
SENSE_MAX_R = 7   # GU_SENSE_MAX_R
SENSE_OUTSIDE = 4  # class of a cell outside the grid
SENSE_AGENT = 8    # added to the agent's cell in the whole-grid view


def check_sense_args(radius, mode):
    """The argument checks of every sense() (ValueError); returns (mode, radius) as the library takes them."""
    if mode not in ('ego', 'grid'):
        raise ValueError("mode must be 'ego' or 'grid'")
    if mode == 'grid':
        return 1, 0
    if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or not 0 <= int(radius) <= SENSE_MAX_R:
        raise ValueError('radius must be an integer in 0 .. {}'.format(SENSE_MAX_R))
    return 0, int(radius)


def cell_classes(spec):
    """uint8[S]: the class of every cell by the reference viewer's tile rule (core/envs/rendering.py:119-133): goal -> 3, else
    lava -> 2, else wall -> 1, else ground -> 0."""
    return np.where(spec.goal, 3, np.where(spec.lava, 2, np.where(spec.wall, 1, 0))).astype(np.uint8)


def view_table(spec, radius):
    """uint8[S, K, K], K = 2 * radius + 1: the egocentric view from every cell (walls included): entry [s, dy, dx] is the class
    of cell (y + dy - radius, x + dx - radius) for s = y * W + x, 4 outside the grid."""
    _, r = check_sense_args(radius, 'ego')
    K = 2 * r + 1
    padded = np.pad(cell_classes(spec).reshape(spec.H, spec.W), r, mode='constant', constant_values=SENSE_OUTSIDE)
    windows = np.lib.stride_tricks.sliding_window_view(padded, (K, K))  # [H, W, K, K]
    return np.ascontiguousarray(windows.reshape(spec.S, K, K))


def grid_view(spec, pos):
    """uint8[H, W]: the whole-grid view of an agent on cell `pos`: the class of every cell, plus 8 on the agent's."""
    pos = int(pos)
    if not 0 <= pos < spec.S:
        raise ValueError('position {} is outside the {}x{} grid'.format(pos, spec.W, spec.H))
    view = cell_classes(spec)
    view[pos] += SENSE_AGENT
    return view.reshape(spec.H, spec.W)


# ---- wind: the per-cell plane of include/gu.h, gu_set_wind ---------------------------------------------------------
WIND_DIRECTIONS = {'up': 0, 'right': 1, 'down': 2, 'left': 3}  # the action codes


def _wind_field(x, W, H, name):
    """An int array [H, W], or [W] meaning per column, as int64[H, W]; a scalar fills the grid."""
    a = np.asarray(x)
    if a.dtype == bool or not np.issubdtype(a.dtype, np.integer):
        raise ValueError('{} must hold integers'.format(name))
    if a.shape == ():
        return np.full((H, W), int(a), np.int64)
    if a.shape == (W,):
        return np.broadcast_to(a.astype(np.int64)[None, :], (H, W)).copy()
    if a.shape == (H, W):
        return a.astype(np.int64)
    raise ValueError('{} must have shape ({}, {}) or ({},), got {}'.format(name, H, W, W, a.shape))


def wind_plane(W, H, strength, direction='up'):
    """uint8[S]: the wind plane of a W x H grid as gu_set_wind takes it -- bits 0..1 of cell s = y * W + x the direction (the action
    codes UP, RIGHT, DOWN, LEFT), bits 2..3 the strength.  `strength`: an int array [H, W], or [W] meaning per column, of values
    0 .. 3.  `direction`: a name ('up', 'right', 'down', 'left'), a code 0 .. 3, or an array of codes of the same shapes."""
    W, H = int(W), int(H)
    if isinstance(strength, (bool, np.bool_)) or np.ndim(strength) == 0:
        raise ValueError('strength must be an array of shape ({}, {}) or ({},)'.format(H, W, W))
    k = _wind_field(strength, W, H, 'strength')
    if k.min() < 0 or k.max() > 3:
        raise ValueError('strength must lie in 0 .. 3')
    if isinstance(direction, str):
        if direction not in WIND_DIRECTIONS:
            raise ValueError("direction must be one of 'up', 'right', 'down', 'left', or a code 0 .. 3")
        direction = WIND_DIRECTIONS[direction]
    d = _wind_field(direction, W, H, 'direction')
    if d.min() < 0 or d.max() > 3:
        raise ValueError('direction codes must lie in 0 .. 3')
    return np.ascontiguousarray((d | (k << 2)).astype(np.uint8).reshape(W * H))


# ---- fruit: the per-cell plane of include/gu.h, gu_set_fruit -------------------------------------------------------
FRUIT_KINDS = {'apple': 1, 'lemon': 2, 'melon': 3}  # the kind codes (0: no fruit)
FRUIT_MAX = 32  # fruits per grid: one bit each in an env's uint32 mask
DOOR_KINDS = {'door': 1, 'key': 2, 'lever': 3}  # the kind codes of include/gu.h, gu_set_doors (0: nothing)
DOOR_SLOTS_MAX = 8  # slots per grid: one bit each in an env's mask of open slots
BOX_TARGET, BOX_INITIAL = 1, 2  # the bits of a box byte (include/gu.h, gu_set_boxes)
BOX_ON_TARGET_MAX = 16  # the most a box pushed onto a target may pay


def fruit_plane(W, H, cells, kinds='apple'):
    """uint8[S]: the fruit plane of a W x H grid as gu_set_fruit takes it -- bits 0..4 of a fruit cell its slot, bits 5..6 its kind,
    every other cell 0.  `cells`: 1 .. 32 distinct cell indices; the slots go by ascending cell index.  `kinds`: one name ('apple',
    'lemon', 'melon') or code 1 .. 3 for all, or one per cell, in the order of `cells`."""
    W, H = int(W), int(H)
    S = W * H
    c = np.asarray(cells)
    if c.ndim != 1 or c.dtype == bool or not np.issubdtype(c.dtype, np.integer):
        raise ValueError('cells must be a list of cell indices')
    if not 1 <= c.size <= FRUIT_MAX:
        raise ValueError('1 .. {} fruit cells, got {}'.format(FRUIT_MAX, c.size))
    if c.min() < 0 or c.max() >= S:
        raise ValueError('fruit cells must lie in 0 .. {}'.format(S - 1))
    if np.unique(c).size != c.size:
        raise ValueError('a cell holds at most one fruit')
    many = not isinstance(kinds, (str, bytes)) and np.ndim(kinds) == 1
    ks = list(kinds) if many else [kinds] * c.size
    if len(ks) != c.size:
        raise ValueError('kinds must be one kind or one per cell ({}), got {}'.format(c.size, len(ks)))
    codes = []
    for k in ks:
        if isinstance(k, str):
            if k not in FRUIT_KINDS:
                raise ValueError("a kind is one of 'apple', 'lemon', 'melon', or a code 1 .. 3")
            k = FRUIT_KINDS[k]
        if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= 3:
            raise ValueError("a kind is one of 'apple', 'lemon', 'melon', or a code 1 .. 3")
        codes.append(int(k))
    plane = np.zeros(S, np.uint8)
    order = np.argsort(c, kind='stable')
    for slot, i in enumerate(order):
        plane[int(c[i])] = slot | (codes[i] << 5)
    return plane


# ---- errands: the instructions of include/gu.h, gu_set_errands (the plane is fruit_plane's) -------------------------
ERRAND_FRUIT_MAX, ERRAND_INSTRUCTIONS_MAX, ERRAND_LENGTH_MAX = 8, 4, 4
_ERRAND_FILLERS = frozenset('collect get eat take pick up the a an and then first next finally'.split())
_KIND_NAMES = {code: name for name, code in FRUIT_KINDS.items()}


def parse_instruction(text):
    """The list of kind names an instruction in words asks for, in order: 'Collect the lemon and then the apple' gives
    ['lemon', 'apple'].  The text is lower-cased and split on everything that is not a letter; the words collect, get, eat, take,
    pick, up, the, a, an, and, then, first, next and finally are dropped, and every other word must be 'apple', 'lemon' or 'melon'
    (ValueError) -- so 'after' and 'before', which would turn the order round, raise rather than being mis-read."""
    if not isinstance(text, str):
        raise ValueError('an instruction in words must be a string')
    words = [w for w in ''.join(ch if ch.isalpha() and ch.isascii() else ' ' for ch in text.lower()).split() if w not in _ERRAND_FILLERS]
    for w in words:
        if w not in FRUIT_KINDS:
            raise ValueError("an instruction names 'apple', 'lemon' and 'melon' only: {!r}".format(w))
    return words


def _errand_kinds(instruction):
    """The kind codes 1 .. 3 of one instruction: a string (parse_instruction) or a list of kind names or codes."""
    ks = parse_instruction(instruction) if isinstance(instruction, str) else list(instruction)
    codes = []
    for k in ks:
        if isinstance(k, str) and k in FRUIT_KINDS:
            k = FRUIT_KINDS[k]
        if isinstance(k, (str, bool, np.bool_)) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= 3:
            raise ValueError("a kind is one of 'apple', 'lemon', 'melon', or a code 1 .. 3")
        codes.append(int(k))
    if not 1 <= len(codes) <= ERRAND_LENGTH_MAX:
        raise ValueError('an instruction names 1 .. {} kinds, got {}'.format(ERRAND_LENGTH_MAX, len(codes)))
    return codes


def instruction_text(kinds):
    """The inverse of parse_instruction: ['lemon', 'apple'] gives 'collect the lemon and then the apple'."""
    return 'collect ' + ' and then '.join('the ' + _KIND_NAMES[k] for k in _errand_kinds(list(kinds)))


def errand_bytes(instructions):
    """uint8[4]: one byte per instruction as gu_set_errands takes them -- position p in bits 2p .. 2p+1, kind 0 the end mark (a list
    of four has none), unused bytes zero.  `instructions`: 1 .. 4 of them, each a string or a list of kind names or codes."""
    if isinstance(instructions, str) or not 1 <= len(instructions) <= ERRAND_INSTRUCTIONS_MAX:
        raise ValueError('1 .. {} instructions, each a string or a list of kinds'.format(ERRAND_INSTRUCTIONS_MAX))
    out = np.zeros(4, np.uint8)
    for j, ins in enumerate(instructions):
        out[j] = sum(k << (2 * p) for p, k in enumerate(_errand_kinds(ins)))
    return out


def pack_errands(instructions):
    """The engine's parameter word of the instructions: byte j holds instruction j (errand_bytes)."""
    return int(errand_bytes(instructions).view('<u4')[0])


def errand_widths(F, instructions):
    """(pb, ib): the bits of the progress and of the instruction index in an env's word, behind the F bits of eaten fruit."""
    lengths = [len(_errand_kinds(ins)) for ins in instructions]
    return max(lengths).bit_length(), (len(lengths) - 1).bit_length()


def errand_fields(words, F, instructions):
    """(eaten, progress, instruction): the three fields of the envs' words uint32[n] under F fruit and `instructions`."""
    w = np.asarray(words).astype(np.uint32)
    pb, ib = errand_widths(F, instructions)
    return w & np.uint32((1 << F) - 1), (w >> np.uint32(F)) & np.uint32((1 << pb) - 1), (w >> np.uint32(F + pb)) & np.uint32((1 << ib) - 1)


def errand_words(eaten, progress, instruction, F, instructions):
    """uint32: the words of the fields, the inverse of errand_fields."""
    pb, _ = errand_widths(F, instructions)
    e, p, j = (np.asarray(x).astype(np.uint32) for x in (eaten, progress, instruction))
    return (e | (p << np.uint32(F)) | (j << np.uint32(F + pb))).astype(np.uint32)


# ---- doors, keys and levers: the per-cell plane of include/gu.h, gu_set_doors ---------------------------------------
def _slot_cells(what, mapping, S):
    """{slot: sorted list of cells} of one argument of door_plane: a mapping slot -> cell or list of cells (None: empty)."""
    out = {}
    if mapping is None:
        return out
    if not hasattr(mapping, 'items'):
        raise ValueError('{} must be a mapping slot -> cell or list of cells'.format(what))
    for slot, cells in mapping.items():
        if isinstance(slot, (bool, np.bool_)) or not isinstance(slot, (int, np.integer)) or not 0 <= int(slot) < DOOR_SLOTS_MAX:
            raise ValueError('{}: a slot is an integer in 0 .. {}, got {!r}'.format(what, DOOR_SLOTS_MAX - 1, slot))
        c = np.atleast_1d(np.asarray(cells))
        if c.ndim != 1 or c.size == 0 or c.dtype == bool or not np.issubdtype(c.dtype, np.integer):
            raise ValueError('{}: slot {} needs a cell index or a list of them'.format(what, slot))
        if c.min() < 0 or c.max() >= S:
            raise ValueError('{}: the cells of slot {} must lie in 0 .. {}'.format(what, slot, S - 1))
        out[int(slot)] = sorted(int(x) for x in c)
    return out


def door_plane(W, H, doors, keys=None, levers=None):
    """uint8[S]: the door plane of a W x H grid as gu_set_doors takes it -- bits 0..2 of a cell its slot, bits 4..5 its kind (1 door,
    2 key, 3 lever), every other cell 0.  `doors`, `keys`, `levers`: mappings slot -> cell or list of cells (None: empty).  The slots
    in use must be 0 .. D-1 without a gap, each with at least one door and at least one key or lever; no cell is named twice."""
    W, H = int(W), int(H)
    S = W * H
    parts = [(name, _slot_cells(name, m, S)) for name, m in (('doors', doors), ('keys', keys), ('levers', levers))]
    used = sorted(set().union(*[set(p) for _, p in parts]))
    if not used:
        raise ValueError('no door, key or lever given')
    if used != list(range(len(used))):
        raise ValueError('the slots in use must be 0 .. D-1 without a gap, got {}'.format(used))
    for slot in used:
        if slot not in parts[0][1]:
            raise ValueError('slot {} has no door'.format(slot))
        if slot not in parts[1][1] and slot not in parts[2][1]:
            raise ValueError('slot {} has neither a key nor a lever'.format(slot))
    plane = np.zeros(S, np.uint8)
    for name, p in parts:
        for slot, cells in p.items():
            for c in cells:
                if plane[c]:
                    raise ValueError('cell {} is named twice'.format(c))
                plane[c] = slot | (DOOR_KINDS[name[:-1]] << 4)
    return plane


# ---- boxes: the per-cell plane and the per-env word of include/gu.h, gu_set_boxes ----------------------------------
def _cell_list(what, cells, S, least):
    """Sorted distinct cell indices from a cell or a list of cells (ValueError)."""
    c = np.atleast_1d(np.asarray([] if cells is None else cells))
    if c.ndim != 1 or (c.size and (c.dtype == bool or not np.issubdtype(c.dtype, np.integer))):
        raise ValueError('{} must be a list of cell indices'.format(what))
    if c.size < least:
        raise ValueError('{} must name at least {} cell'.format(what, least))
    if c.size and (c.min() < 0 or c.max() >= S):
        raise ValueError('{} must lie in 0 .. {}'.format(what, S - 1))
    if np.unique(c).size != c.size:
        raise ValueError('{} names a cell twice'.format(what))
    return sorted(int(x) for x in c)


def box_bits(S):
    """b: the bits of one box's cell in an env's word, the smallest width with S <= 1 << b (at least 1)."""
    return max(1, int(S - 1).bit_length())


def box_plane(W, H, boxes, targets):
    """uint8[S]: the box plane of a W x H grid as gu_set_boxes takes it -- bit 0 of a cell: it is a target, bit 1: a box stands on it at
    every reset; a cell may be both.  `boxes`, `targets`: a cell or a list of distinct cells.  At least one box, at least as many
    targets as boxes, at least one box off target, and the boxes' cells must fit an env's word: box_bits(S) * len(boxes) <= 32."""
    W, H = int(W), int(H)
    S = W * H
    bx, tg = _cell_list('boxes', boxes, S, 1), _cell_list('targets', targets, S, 1)
    if len(tg) < len(bx):
        raise ValueError('{} targets for {} boxes: every box needs a target'.format(len(tg), len(bx)))
    if set(bx) <= set(tg):
        raise ValueError('every box stands on a target: nothing is left to solve')
    if box_bits(S) * len(bx) > 32:
        raise ValueError('{} boxes of {} bits each do not fit the 32 bits of an env\'s word'.format(len(bx), box_bits(S)))
    plane = np.zeros(S, np.uint8)
    plane[tg] |= BOX_TARGET
    plane[bx] |= BOX_INITIAL
    return plane


def pack_boxes(S, cells):
    """uint32[n] (or one uint32 for a 1-d `cells`): the words that hold the box cells int[n, B] -- box k in bits [k * b, (k + 1) * b),
    b = box_bits(S).  Every cell must lie in 0 .. S-1, no two boxes of a word on one cell, and b * B <= 32."""
    c = np.asarray(cells)
    if c.ndim not in (1, 2) or c.shape[-1] == 0 or c.dtype == bool or not np.issubdtype(c.dtype, np.integer):
        raise ValueError('cells must be integers of shape (B,) or (n, B)')
    b, B = box_bits(S), c.shape[-1]
    if b * B > 32:
        raise ValueError('{} boxes of {} bits each do not fit the 32 bits of an env\'s word'.format(B, b))
    if c.size and (c.min() < 0 or c.max() >= S):
        raise ValueError('box cells must lie in 0 .. {}'.format(S - 1))
    rows = c.reshape(-1, B).astype(np.uint64)
    if any(np.unique(r).size != B for r in rows):
        raise ValueError('two boxes of one env on the same cell')
    words = (rows << (np.arange(B, dtype=np.uint64) * np.uint64(b))).sum(axis=1).astype(np.uint32)  # (distinct fields: the sum is the or)
    return words[0] if c.ndim == 1 else words


def unpack_boxes(S, words, B):
    """int32[n, B] (or int32[B] for one word): the box cells held by the words, the inverse of pack_boxes."""
    w = np.asarray(words)
    b = box_bits(S)
    if not 1 <= int(B) or b * int(B) > 32:
        raise ValueError('B must be at least 1 and {} bits each must fit 32 bits'.format(b))
    flat = np.atleast_1d(w).astype(np.uint64)
    cells = ((flat[:, None] >> (np.arange(int(B), dtype=np.uint64) * np.uint64(b))) & np.uint64((1 << b) - 1)).astype(np.int32)
    return cells[0] if w.ndim == 0 else cells


def sokoban_level(text):
    """(GridSpec, boxes, targets) from a level in the standard XSB characters: '#' wall, '@' agent, '+' agent on a target, '$' box, '*'
    box on a target, '.' target, ' ' or '-' floor.  Rows are the lines of `text` (empty lines before and behind are dropped), ragged
    rows are padded with floor.  The grid has the agent's cell as its start and neither goal nor lava cells: its episodes end by
    solving the level."""
    lines = [ln.rstrip('\r') for ln in str(text).split('\n')]
    while lines and not lines[0].strip():
        lines.pop(0)
    while lines and not lines[-1].strip():
        lines.pop()
    if not lines:
        raise ValueError('the level is empty')
    W, H = max(len(ln) for ln in lines), len(lines)
    walls, boxes, targets, agents = [], [], [], []
    for y, ln in enumerate(lines):
        for x, ch in enumerate(ln):
            s = y * W + x
            if ch not in '#@+$*. -':
                raise ValueError('character {!r} in row {}: a level holds # @ + $ * . - and spaces'.format(ch, y))
            if ch == '#':
                walls.append(s)
            if ch in '@+':
                agents.append(s)
            if ch in '$*':
                boxes.append(s)
            if ch in '+*.':
                targets.append(s)
    if len(agents) != 1:
        raise ValueError('a level has one agent, got {}'.format(len(agents)))
    return GridSpec(W, H, agents, [], [], walls), boxes, targets
