"""Host-side view of the engine's per-env counter RNG (the device code is csrc/gu_rng.hpp).

The reference has no per-env RNG (it draws from process-global RNGs), so the engine defines
one, keyed by (seed, GLOBAL env id, stream, counter):

    word = MurmurHash3_x86_32 over the words [seed_lo, seed_hi, env, (stream << 28) | (counter & 0x0FFFFFFF)], hash seed
           0x9747B28C; counters of 2**28 and more append a fifth word, counter >> 28 (no stream repeats before 2**32 draws)
    stream 0  uniform actions : action(t) = (word(t >> 4) >> (2 * (t & 15))) & 3, t = steps the env has taken
    stream 1  start cell      : index = (word(episode) * n_starts) >> 32, episode = resets since gu_seed
    stream 2  sampled actions : u = word(t) / 2**32 against the cumulative policy row
    stream 3  maze generation : draw k of grid g = (word(k) * n) >> 32, keyed by (maze_seed, global grid id)
    stream 4  TD control      : one word per step of gu_td_run, counter t & 0xFFFFFFFF, epoch t >> 32 (hashed right behind the
                                seed when it is not zero, as for streams 0 and 2); explore iff (word >> 16) < eps_q16, explore action
                                word & 3, greedy tie index (((word >> 2) & 0x3FFF) * ties) >> 14
    stream 9  gusts of wind   : one word per step taken from a cell with wind while gust_q16 > 0 (gu_set_wind), counter and epoch
                                as stream 4; the strength k changes iff (word >> 16) < gust_q16, to k + 1 if word & 1 else k - 1
    stream 11 errands         : the instruction an env is given at a reset while errands are set (gu_set_errands): index =
                                (word(episode) * I) >> 32, keyed like stream 1 with the episode count before the reset
    stream 10 Double Q coin   : one word per step of gu_double_run, counter and epoch as stream 4 at the same step count; bit 0 picks
                                the table that learns (0: A from B's estimate, 1: B from A's)

These helpers let a caller reproduce on the host exactly what a `policy='uniform'` rollout did on the device -- e.g.
to replay the same (grid, seed, action) sequence through the reference's own `step()`.
"""
import numpy as np

_M32 = np.uint64(0xFFFFFFFF)


def _rotl(x, r):
    return ((x << np.uint64(r)) | (x >> np.uint64(32 - r))) & _M32


def _block(h, k):
    k = (k * np.uint64(0xCC9E2D51)) & _M32
    k = _rotl(k, 15)
    k = (k * np.uint64(0x1B873593)) & _M32
    h = _rotl(h ^ k, 13)
    return (h * np.uint64(5) + np.uint64(0xE6546B64)) & _M32


def words(seed, env_ids, stream, counters, epochs=None):
    """uint32 RNG words for broadcastable arrays of global env ids and counters (and epochs: hashed behind the seed where not 0)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    env = np.asarray(env_ids, dtype=np.uint64) & _M32
    ctr = np.asarray(counters, dtype=np.uint64) & _M32
    epoch = np.zeros((), np.uint64) if epochs is None else np.asarray(epochs, dtype=np.uint64) & _M32
    env, ctr, epoch = np.broadcast_arrays(env, ctr, epoch)
    h = np.full(env.shape, 0x9747B28C, dtype=np.uint64)
    h = _block(_block(h, np.uint64(seed & 0xFFFFFFFF)), np.uint64(seed >> 32))
    h = np.where(epoch != 0, _block(h, epoch), h)
    for k in (env, np.uint64((int(stream) & 0xF) << 28) | (ctr & np.uint64(0x0FFFFFFF))):
        h = _block(h, k)
    high = ctr >> np.uint64(28)
    h = np.where(high != 0, _block(h, high) ^ np.uint64(20), h ^ np.uint64(16))
    h = h ^ (h >> np.uint64(16))
    h = (h * np.uint64(0x85EBCA6B)) & _M32
    h = h ^ (h >> np.uint64(13))
    h = (h * np.uint64(0xC2B2AE35)) & _M32
    h = h ^ (h >> np.uint64(16))
    return h.astype(np.uint32)


def uniform_actions(seed, env_ids, t0, T):
    """int32[T, N]: the actions a `policy='uniform'` rollout takes for global env ids `env_ids`, steps t0 .. t0+T-1."""
    t = (np.arange(T, dtype=np.uint64) + np.uint64(t0))[:, None]
    w = words(seed, np.asarray(env_ids, dtype=np.uint64)[None, :], 0, t >> np.uint64(4)).astype(np.uint64)
    return ((w >> (np.uint64(2) * (t & np.uint64(15)))) & np.uint64(3)).astype(np.int32)


def start_indices(seed, env_ids, episodes, n_starts):
    """Index into starting_states chosen at reset number `episodes` (0 = first reset after gu_seed)."""
    w = words(seed, env_ids, 1, episodes).astype(np.uint64)
    return ((w * np.uint64(int(n_starts))) >> np.uint64(32)).astype(np.int32)


def epsilon_greedy_words(seed, env_ids, t0, T):
    """uint32[T, N]: the stream-4 words behind steps t0 .. t0+T-1 (64-bit step counts) of gu_td_run for global env ids `env_ids`.
    t0 is one count for all, or one per env."""
    t = np.arange(T, dtype=np.uint64)[:, None] + np.asarray(t0, dtype=np.uint64)
    env = np.asarray(env_ids, dtype=np.uint64)[None, :]
    return words(seed, env, 4, t & _M32, t >> np.uint64(32))


def wind_words(seed, env_ids, t):
    """uint32: the stream-9 words behind the gusts of the steps at 64-bit step counts `t` of global env ids `env_ids` (the two
    broadcast against each other); see gu_set_wind in include/gu.h."""
    t = np.asarray(t, dtype=np.uint64)
    return words(seed, np.asarray(env_ids, dtype=np.uint64), 9, t & _M32, t >> np.uint64(32))


def errand_words(seed, env_ids, episodes):
    """uint32: the stream-11 words behind the instructions that the resets number `episodes` (0 = first reset after gu_seed) give the
    global env ids `env_ids` (the two broadcast against each other): instruction = (word * I) >> 32; see gu_set_errands in
    include/gu.h."""
    return words(seed, np.asarray(env_ids, dtype=np.uint64), 11, episodes)
