"""The cases of tests/test_gpu_overlays_at_scale.py and of its host twin tests/test_overlay_scale_host.py: the grids of Part A with
their planes and placements (added to tests/_overlay_starts.py's GRIDS, so that its planes, restatements, placement and policy table
serve them), how many learners td_run gets on each, what each kind's restatement must have met for a comparison to say something,
the batch of Part B, the shapes of Part C and the overlay-aware adapter that takes them through tests/_learners.py's harness.
Nothing here needs a device.

Every grid has three start cells, a goal in the far corner and ONE lava cell, the anchor: the planes' cells lie within five columns
of it, in its row and the row below (one row on 'line40000'), the first start six columns to its left, and after the first reset the
envs are put on the free cells within six columns and one row of it (`around`), so that 33 steps meet the planes and episodes end
from the first step on; the other two starts lie far away.
    big182      182 x 182 = 33 124 cells   S > GU_MAX_LDS_CELLS = 32 767; the anchor (100, 180) is cell 32 860: every plane cell, every
                                           start and two of the three rows of `around` lie past cell 32 767
    fit156      140 x 156 = 21 840 cells   cell_bytes 21 840, 3 x 21 840 = 65 520 <= 65 536: the largest three-plane LDS image
    over32      683 x 32  = 21 856 cells   cell_bytes 21 856, 3 x 21 856 = 65 568: 32 bytes too many, the overlay kernels read L2
    line40000   40 000 x 1                 W fits no int16 delta; up and down never move; the anchor is cell 36 000"""
import numpy as np

from . import _errands_oracle as EO
from . import _overlay_starts as S
from ._learners import Learner, _eps
from ._overlays import METHODS, errand_bits, overlay

N, T, ID0 = S.N, S.T, S.IDS[1]
KINDS = S.KINDS
MAX_LDS_CELLS, LDS = 32767, 65536
TD_STEPS = (150, 151)  # (the second launch starts with the action SARSA carried out of the first)
TD_BYTES = 400 << 20   # td_run gets N learners where their tables stay below this, else six
ALPHA, GAMMA, EPS = 0.25, 0.9, 0.3


def cell_bytes(S_):
    return (S_ + 15) & ~15


def _scale_grid(W, H, anchor, far):
    """The grid dict of one Part A grid: `anchor` = (x, y) of the lava cell, `far` = the (x, y) of the second and third start."""
    ax, ay = anchor
    flat = H == 1

    def at(dx, dy=0):
        return (ay + (0 if flat else dy)) * W + ax + dx

    rows = (0,) if flat else (-1, 0, 1)
    g = dict(W=W, H=H, starts=[at(-6, 1)] + [y * W + x for x, y in far], goals=[W * H - 1], lava=[at(0)], walls=[],
             around=[at(dx, dy) for dy in rows for dx in range(-6, 7) if at(dx, dy) not in (at(0), at(-6, 1))],
             cells=dict(fruit=[at(-3), at(2, 1), at(4)], doors=(at(-2), at(-4, 1)), boxes=([at(2), at(-2, 1)], [at(3), at(-3, 1)]),
                        errands=[at(2), at(3), at(-2), at(-4, 1), at(5, 1)],  # (apple, lemon, melon, apple, lemon: EO.CASE_KINDS)
                        doors3=dict(doors={0: at(-2), 1: at(3), 2: at(-5)}, keys={0: at(-4, 1), 1: at(5, 1)}, levers={2: at(1, 1)})))
    # the errands' learners: tables of tens of MB per env -- three bits (an apple, a lemon, one instruction) where S is largest, else the
    # six bits of tests/test_gpu_errands.py (three fruit, two instructions)
    if W * H > MAX_LDS_CELLS:
        g['errands_td'] = dict(cells=[at(2), at(-2)], kinds=['apple', 'lemon'], instructions=[['apple']])
    else:
        g['errands_td'] = dict(cells=[at(2), at(-2), at(3, 1)], kinds=EO.TD_KINDS, instructions=EO.TD_INSTRUCTIONS)
    return g


GRIDS = {'big182': _scale_grid(182, 182, (100, 180), [(170, 181), (20, 180)]),
         'fit156': _scale_grid(140, 156, (70, 77), [(10, 3), (130, 150)]),
         'over32': _scale_grid(683, 32, (300, 16), [(10, 2), (670, 30)]),
         'line40000': _scale_grid(40000, 1, (36000, 0), [(100, 0), (39990, 0)])}
S.GRIDS.update(GRIDS)
# what each test of Part A asserts after a rollout: rollout_last_form()['lds_bytes']
LDS_BYTES = {'big182': 0, 'fit156': 65520, 'over32': 0, 'line40000': 0}


def arithmetic(name):
    """The arithmetic of a Part A grid's row in the docstring above: (S, cell_bytes, three planes fit LDS)."""
    g = S.grid_dict(name)
    S_ = g['W'] * g['H']
    fits = S_ <= MAX_LDS_CELLS and 3 * cell_bytes(S_) <= LDS
    assert (S_, cell_bytes(S_), fits) == {'big182': (33124, 33136, False), 'fit156': (21840, 21840, True), 'over32': (21856, 21856, False),
                                         'line40000': (40000, 40000, False)}[name]
    assert LDS_BYTES[name] == (3 * cell_bytes(S_) if fits else 0)
    if name == 'big182':  # the planes, the starts and the cells the envs are put on lie past cell 32 767
        cells = g['cells']
        assert S_ > MAX_LDS_CELLS and min(g['starts'] + cells['fruit'] + list(cells['doors']) + cells['boxes'][0] + cells['boxes'][1] + cells['errands']) > 32767
        assert sum(s > 32767 for s in g['around']) >= 2 * len(g['around']) // 3
    if name == 'fit156':
        assert 3 * cell_bytes(S_) == 65520 <= LDS
    if name == 'over32':  # 32 bytes too many for three planes, while two fit: the calm kernels still stage it
        assert 3 * cell_bytes(S_) == LDS + 32 and S_ <= MAX_LDS_CELLS and 2 * cell_bytes(S_) <= LDS
    if name == 'line40000':
        assert g['W'] > 32767 and g['H'] == 1 and min(g['around']) > 32767
    return S_, cell_bytes(S_), fits


def family(kind):
    return {'gusts': 'wind'}.get(kind, kind)


def bits(kind, name):
    """The mask bits of `kind` on grid `name`: the tables have S << bits rows."""
    if kind == 'errands':
        return errand_bits(S.plane(kind, name), S.extra(kind, name)[0])
    return overlay(kind).bits(S.plane(kind, name))


def td_case(kind, name):
    """(grid name, learners) of td_run under `kind` on `name`; learners None: gu_td_init refuses the kind there (more than 10 bits)."""
    td = S.td_grid(kind, name)
    g = S.grid_dict(td)
    b = bits(kind, td)
    if b > 10:
        return td, None
    return td, N if ((g['W'] * g['H']) << b) * 32 * N <= TD_BYTES else 6


def met(kind, o, auto=True, starts=True):
    """The restatement o of `kind` met what its case is about (its own log): fruit eaten; a door opened (its key taken) and one found
    shut; a box pushed and one push refused; a gust that changed a push; an errand completed and a wrong fruit eaten, every
    instruction drawn.  Under auto-reset every start was drawn (`starts`: by enough envs to say so); without it some env took an
    absorbed step."""
    log = getattr(o, 'log', {})
    if kind == 'gusts':
        assert log['gust_moved'] >= 1, log
    if kind == 'fruit':
        assert log['eaten'] >= 1, log
    if kind == 'doors':
        assert log['key'] >= 1 and log['bump'] >= 1, log
    if kind == 'boxes':
        assert log['push'] >= 1 and log['refused_wall'] + log['refused_box'] + log['refused_terminal'] >= 1, log
    if kind == 'errands':
        assert log['completed'] >= 1 and log['wrong'] >= 1 and log['drawn'] == set(range(len(o.instr))), log
        assert auto or log['absorbed'] >= 1, log
    if auto and starts:
        S.drew_every_start(o)


def absorbed(want):
    """Rows of a rollout without auto-reset: some env was done before the last step, and so took a step that its terminal cell (or
    its solved or completed word) absorbed."""
    assert (want['done'][:-1] != 0).any()


def fresh(kind, name, n=N, q0=None, env_id0=ID0):
    """The restatement of `kind` on `name`, reset and put in place."""
    o = S.oracle(kind, name, env_id0, n=n, q0=q0)
    o.reset()
    S.place(kind, name, o)
    return o


def steps(o):
    """The step case on the restatement o, one step at a time: yields (i, actions, refused, (obs, reward, done)).  Twice, from step 10
    on and when some env is due a lazy reset, every fifth env and every env that is due one gets an action outside -4 .. 3
    (`refused`: gu_step answers GU_ERR_INVALID): those envs do not step, reset or touch their word, the others do."""
    acts, count = S.step_actions(o.n), 0
    for i in range(T):
        a, out = acts[i].copy(), np.zeros(o.n, bool)
        if i >= 10 and count < 2 and (o.state.done != 0).any():
            out = (np.arange(o.n) % 5 == 0) | (o.state.done != 0)
            a[out] = 4 + i
            count += 1
        obs, rew, don, rejected = o.step(a, True)
        assert np.array_equal(rejected, out), i
        yield i, a, bool(out.any()), (obs, rew, don)
    assert count == 2


def learned_on_masked_rows(kind, name, o):
    """The tables left their fill, under a kind with mask bits on rows of a mask other than 0 as well (key * S + s with key > 0)."""
    assert (o.q != S.Q0).any()
    if bits(kind, name):
        assert (o.q[:, o.grid.S:] != S.Q0).any()


# ---------------------------------------------------------------------------------------------------------------- Part B
BIG_N = 65536 + 70  # 257 workgroups of 256 envs, the last one of one full wave and one wave of six lanes
BATCH_GRIDS = ('starts8', 'open150')
BATCH_POLICIES = ('uniform', 'stream')
assert BIG_N == 256 * 256 + 64 + 6


def batch_step_case(kind, name, o):
    """The step case of Part B on the restatement o (reset and in place): sixteen uniform steps without auto-reset, which leave envs
    done in the first workgroup and in the last one's two waves, then gu_step on step_actions()[0] with auto-reset (their lazy resets)
    and gu_step_device on step_actions()[2].  dict(rows=, step=, step_device=): what each returns."""
    acts = S.step_actions(o.n)
    rows = S.rollout_of(o, name, 'uniform', 16, auto=False)
    done = o.state.done != 0
    assert done[:256].any() and done[-70:-6].any() and done[-6:].any() and not done.all()
    out = dict(rows=rows)
    for key, i in (('step', 0), ('step_device', 2)):
        obs, rew, don, rejected = o.step(acts[i], True)
        assert not rejected.any()
        out[key] = (obs, rew, don)
    assert len(set(o.state.pos[done].tolist())) > 3 and (out['step_device'][2] != 0).any()  # (the resets drew their starts and the envs moved on; the compaction has something to compact)
    met(kind, o)
    return out


# ---------------------------------------------------------------------------------------------------------------- Part C
class OverlayTd(Learner):
    """td_run under a MASKED overlay kind for tests/_learners.py's _stores_past_a_boundary: the restatement is the kind's own, built
    at the group's first env id, and the stores are the group's tables [n][S << bits][4] and its per-env words."""

    def __init__(self, kind, name, method):
        self.kind, self.name, self.method = kind, name, method

    def oracle(self, grid, seed, n, env_id0):
        return S.oracle(self.kind, self.name, env_id0, n=n, seed=seed, q0=S.Q0)

    def prepare(self, vec):
        overlay(self.kind).install(vec.engine, S.plane(self.kind, self.name), *S.extra(self.kind, self.name))
        vec._ensure_q(S.Q0)

    def device(self, vec, T, **kw):
        return vec.td_run(T, self.method, alpha=ALPHA, discount_factor=GAMMA, epsilon=EPS, **kw)

    def restate(self, o, T):
        return o.td_run(T, METHODS[self.method], ALPHA, GAMMA, _eps(EPS))

    def got(self, vec, env0, n):
        return dict(q=vec.q_table(env0, n), words=getattr(vec.engine, 'get_%s_state' % self.kind)(env0, n))

    def want(self, o):
        return dict(q=o.q, words=S.masks_of(o, self.kind))

    def learned(self, o):
        return [('q', o.q, S.Q0)]


def _small(W, H, errands_td=None, boxes=None):
    """An open W x H grid of Part C: three starts, a goal in the far corner, lava in the middle."""
    S_ = W * H
    g = dict(W=W, H=H, starts=[W + 1, S_ // 2 + 2, S_ - W - 2], goals=[S_ - 1], lava=[(H // 2) * W + W // 2], walls=[])
    if errands_td:
        g['errands_td'] = errands_td
    if boxes:
        g['cells'] = dict(boxes=boxes)
    return g


# fruit: the three fruit of Part A; doors: three slots (two keys and a lever) on big182; boxes: one box on 31 x 33 = 1 023 cells, 10 bits;
# errands: five fruit, a list of four and three instructions on 8 x 9, 5 + 3 + 2 bits -- the last two at the learners' limit
S.GRIDS['doors182'] = dict(GRIDS['big182'], cells=dict(GRIDS['big182']['cells'], doors=GRIDS['big182']['cells']['doors3']))
S.GRIDS['box1023'] = _small(31, 33, boxes=([16 * 31 + 18], [16 * 31 + 20]))
S.GRIDS['errand72'] = _small(8, 9, errands_td=dict(cells=[10, 12, 20, 29, 43], kinds=EO.CASE_KINDS, instructions=EO.CASE_INSTRUCTIONS['wander']))
# id: (kind, grid, bits, N, the env in whose table byte 2^32 lies, envs in a group)
MASKED = {'fruit': ('fruit', 'big182', 3, 520, 506, 8), 'doors': ('doors', 'doors182', 3, 520, 506, 8), 'boxes': ('boxes', 'box1023', 10, 136, 128, 4),
          'errands': ('errands', 'errand72:td', 10, 1830, 1820, 16)}
ELEMENTS = ('fruit', 'big182', 3, 2040, 2025, 8)  # entry 2^31 of the tables lies in env 2 025's, 2 880 rows before its end (17.3 GB)


C_LAUNCHES = (60, 41)
C_SEED = 5  # (tests/_learners.py: _stores_past_a_boundary's)


def bytes_per_env(name, b):
    g = S.grid_dict(name)
    return ((g['W'] * g['H']) << b) * 4 * 8


def group_starts(n, crossing, width):
    """The first envs of the groups _stores_past_a_boundary compares: the first, the last and the one around the crossing."""
    return sorted({0, n - width, crossing - width // 2})


def put_in_place(kind, name, n):
    """The `before` of _stores_past_a_boundary: where `name` has a placement, the batch (at the first group) and every group's
    restatement are put there, so that the learners meet the planes within the launches."""
    pos = S.placement(kind, name, n)

    def before(vec, e0, o):
        if pos is not None:
            if vec is not None and e0 == 0:
                vec.set_state(pos=pos)
            o.state.pos[:] = pos[e0:e0 + o.n]
    return before
