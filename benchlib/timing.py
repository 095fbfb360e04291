"""Timing of bench.py: the host channel between ranks, one block of exactly K launches between barrier + device sync pairs."""
import contextlib
import ctypes
import os
import sys
import time

import numpy as np


class Ranks(object):
    """Host channel between the ranks: griduniverse_amd.rendezvous (one socket per rank to rank 0; torchrun-style environment,
    no PyTorch).  A no-op for one process."""

    def __init__(self, rank, world):
        from griduniverse_amd.rendezvous import Rendezvous
        self.rank, self.world = rank, world
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        self.rdzv = Rendezvous(rank, world, join_timeout=float(os.environ.get('GU_RDZV_JOIN_TIMEOUT', '600')))
        self.rdzv.barrier()

    def barrier(self):
        self.rdzv.barrier()

    def reduce(self, values, op):
        """Element-wise MAX / MIN over ranks of a list of floats."""
        return self.rdzv.reduce(values, op)

    def gather(self, values):
        """[world][len] of every rank's list of floats."""
        return self.rdzv.gather(values)

    def gather_bytes(self, payload):
        return self.rdzv.gather_bytes(payload)

    def broadcast_bytes(self, payload, src=0):
        return self.rdzv.broadcast_bytes(payload, src)

    def close(self):
        self.rdzv.close()


def timed_block(eng, ranks, T, K):
    """EXACTLY K launches between barrier + device sync pairs.  Returns (wall seconds, HIP-event ms) of this rank."""
    eng.sync()
    ranks.barrier()
    t0 = time.perf_counter()
    eng.timer_begin()
    for _ in range(K):
        eng.rollout(T, 'uniform', auto_reset=True, trajectory=True)
    kernel_ms = eng.timer_end()  # HIP events on the engine's stream; also drains it
    eng.sync()
    elapsed = time.perf_counter() - t0
    ranks.barrier()
    return elapsed, kernel_ms


def timed_region(eng, ranks, T, K):
    """The settle launches of the kind (settle_launches: a fixed number, untimed), then ONE timed block of exactly K launches, so
    that --steps is the number of timed launches and every run issues the same launches.  Returns the block's wall seconds and
    HIP-event ms (each MAX over ranks) and this rank's own wall seconds, each as a one-element list, and the number of launches
    issued."""
    settle = settle_launches(eng, T, 'uniform', trajectory=True)
    for _ in range(settle):
        eng.rollout(T, 'uniform', auto_reset=True, trajectory=True)
    e, k = timed_block(eng, ranks, T, K)
    both = ranks.reduce([e, k], 'MAX')
    return both[:1], both[1:], [e], 1 + settle + K


@contextlib.contextmanager
def native_stdout_to_stderr():
    """RCCL prints a banner (ROCm version, hostname, library path) to the C-level stdout when a communicator comes up, and C
    stdio flushes it whenever it likes -- after the JSON line, when stdout is a pipe.  The driver reads ONE JSON line from
    stdout, so everything native code prints inside this block goes to stderr instead."""
    libc = ctypes.CDLL(None)
    sys.stdout.flush()
    libc.fflush(None)
    saved = os.dup(1)
    os.dup2(2, 1)
    try:
        yield
    finally:
        libc.fflush(None)
        os.dup2(saved, 1)
        os.close(saved)


def spread(values):
    v = np.sort(np.asarray(values, dtype=np.float64))
    return float(v[0]), float(np.median(v)), float(v[-1])



def settle_launches(eng, T, policy, **kw):
    """Untimed launches in front of a timed block of a launch kind: 3, or 200 for a kind whose rows keep a store schedule
    (the closed loop of the store pacing runs inside the launches themselves; 200 launches = 20 ms at the headline size)."""
    eng.rollout(T, policy, auto_reset=True, **kw)
    return settle_count(eng, policy, packed=kw.get('trajectory') == 'packed')


def settle_count(eng, policy, packed=False):
    """settle_launches' number for an engine that has launched the kind at least once."""
    paced = hasattr(eng, 'rollout_pacing') and eng.rollout_pacing(policy, True, packed=packed) is not None
    return 200 if paced else 3


def launch_ms(eng, T, K, policy='uniform', **kw):
    """HIP-event ms per launch of one launch kind after its settle launches (beside `value`, never as it)."""
    for _ in range(settle_launches(eng, T, policy, **kw)):
        eng.rollout(T, policy, auto_reset=True, **kw)
    eng.sync()
    eng.timer_begin()
    for _ in range(K):
        eng.rollout(T, policy, auto_reset=True, **kw)
    return eng.timer_end() / K
