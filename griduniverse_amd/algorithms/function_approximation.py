"""Value approximation: episodic semi-gradient SARSA (Sutton & Barto 10.1) and semi-gradient Q-learning with linear function
approximation over K active binary features per state -- the reference's roadmap entry "Value Approximation" (README.md; it ships
no code for it, so the semantics are this build's: include/gu.h, gu_fa_run).

The action values are computed, not stored: Q(s) is the sum of the K weight rows [4] that the feature table phi[S][K] activates in
s.  `tile_coding`, `state_aggregation`, `one_hot` and `view_features` build such tables; `semi_gradient_sarsa` /
`semi_gradient_q_learning` run `num_learners` independent epsilon-greedy learners on the grid of a facade `GridUniverseEnv`, learner e in env e of a batch, each
with its own float64 weights, all advanced on the MI355X by one kernel (csrc/gu_fa.hip), and return the action values folded from
the weights in the format of `temporal_difference.q_learning`, so `greedy_policy` applies unchanged.  With `one_hot` features they
are `sarsa` / `q_learning`.
"""
import numpy as np

from .. import _lib
from ._batch import _CHUNK, learn, need_learners, unit


def tile_coding(W, H, tilings, tile):
    """K = `tilings` grids of square tiles of side B = `tile` over the W x H cells, tiling k displaced by dx = (k*B)//K cells to
    the left and dy = (3*k*B//K) % B cells up.  Returns (phi int32[S, K], F): phi[s][k] = k*TW*TH + ((y+dy)//B)*TW + (x+dx)//B
    with TW = (W+B-2)//B + 1 tiles across and TH likewise down, F = K*TW*TH.  Column k holds the indices of tiling k only."""
    W, H, K, B = int(W), int(H), int(tilings), int(tile)
    if W < 1 or H < 1 or B < 1:
        raise ValueError('W, H and tile must be at least 1')
    if not 1 <= K <= _lib.FA_MAX_K:
        raise ValueError('tilings must lie in 1 .. {}'.format(_lib.FA_MAX_K))
    TW, TH = (W + B - 2) // B + 1, (H + B - 2) // B + 1
    s = np.arange(W * H)
    x, y = s % W, s // W
    phi = np.empty((W * H, K), np.int32)
    for k in range(K):
        dx, dy = (k * B) // K, (3 * k * B // K) % B
        phi[:, k] = k * TW * TH + ((y + dy) // B) * TW + (x + dx) // B
    return phi, K * TW * TH


def state_aggregation(W, H, block):
    """One feature per block x block square of cells (K = 1).  Returns (phi int32[S, 1], F)."""
    W, H, B = int(W), int(H), int(block)
    if W < 1 or H < 1 or B < 1:
        raise ValueError('W, H and block must be at least 1')
    BW, BH = (W + B - 1) // B, (H + B - 1) // B
    s = np.arange(W * H)
    return ((s // W // B) * BW + (s % W) // B).astype(np.int32)[:, None], BW * BH


def one_hot(S):
    """One feature per state (K = 1, F = S): the tabular case.  Returns (phi int32[S, 1], S)."""
    S = int(S)
    if S < 1:
        raise ValueError('S must be at least 1')
    return np.arange(S, dtype=np.int32)[:, None], S


def view_features(env, radius):
    """What the agent SEES as its only feature: phi[s] is the id of the egocentric view of `radius` from cell s (grid.view_table:
    the classes of the (2 * radius + 1)^2 cells around it, 4 outside the grid), ids in order of first appearance over s = 0 .. S-1,
    so states that look alike share one weight row -- a perceptually aliased learner on the kernel of `semi_gradient_*`.  `env`: a
    GridUniverseEnv (or anything GridSpec.from_env reads) or a GridSpec.  Returns (phi int32[S, 1], F), F the number of distinct
    views; for radius >= max(W, H) - 1 the border places the agent and the features are one_hot's, relabelled."""
    from ..grid import GridSpec, view_table
    spec = env if isinstance(env, GridSpec) else GridSpec.from_env(env)
    views = view_table(spec, radius).reshape(spec.S, -1)
    ids, phi = {}, np.empty((spec.S, 1), np.int32)
    for s in range(spec.S):
        phi[s, 0] = ids.setdefault(views[s].tobytes(), len(ids))
    return phi, len(ids)


def _fa(method, env, num_steps, features, alpha, discount_factor, epsilon, num_learners, seed, w0):
    need_learners(num_learners)
    unit('epsilon', epsilon)
    if features is None:
        features = tile_coding(env.x_max, env.y_max, 4, 4)
    phi, F = features
    phi = np.asarray(phi)
    K = 1 if phi.ndim == 1 else phi.shape[1]
    # consecutive launches carry SARSA's next action, so chunking changes nothing
    return learn(env, num_learners, seed, num_steps, _CHUNK, lambda vec: vec.set_features(phi, F, w0),
                 lambda vec, T: vec.fa_run(T, method, float(alpha) / K, discount_factor, epsilon), lambda vec: vec.fa_q_table())


def semi_gradient_sarsa(env, num_steps, features=None, alpha=0.1, discount_factor=0.99, epsilon=0.1, num_learners=1, seed=0, w0=0.0):
    """Epsilon-greedy episodic semi-gradient SARSA, `num_steps` env steps per learner (episodes restart at a start cell when
    they end).  `features`: (phi int32[S, K], F) as `tile_coding` returns it; None means tile_coding(W, H, 4, 4).  The step size
    of a launch is alpha / K.  Returns Q float64[S][4] folded from the learned weights, or [L][S][4] for L = num_learners > 1."""
    return _fa('sarsa', env, num_steps, features, alpha, discount_factor, epsilon, num_learners, seed, w0)


def semi_gradient_q_learning(env, num_steps, features=None, alpha=0.1, discount_factor=0.99, epsilon=0.1, num_learners=1, seed=0,
                             w0=0.0):
    """Epsilon-greedy semi-gradient Q-learning; arguments and result as `semi_gradient_sarsa`."""
    return _fa('q_learning', env, num_steps, features, alpha, discount_factor, epsilon, num_learners, seed, w0)
