// gu_td.hip -- batched tabular Q-learning and SARSA for gfx950: N independent learners, learner e owns env e and its own
// float64 table Q_e[S][4], advanced T steps per launch.  The semantics are build-defined (the reference has no TD code) and are
// stated in include/gu.h (gu_td_run) and restated on the CPU by tests/_td_oracle.py.
//
// One lane per env, like the rollout.  Per step the lane
//   - draws one word of RNG stream 4, keyed by its 64-bit step count t (epsilon test, explore action, tie break),
//   - moves with the engine's rule (gu_move on the staged cell map, absorbing terminal),
//   - reads the row Q[s'] (32 bytes: two 16-byte loads) -- the only dependent gather of the step -- and
//   - writes back the one updated entry Q[s][a] (8 bytes).
// The row of the current state stays in VGPRs from one step to the next; a wall bump (s' == s) forwards the updated entry
// instead of reading the row back, and a terminal s' (target = r) reads nothing.
// Table layout: learner-major, [N][S][4] -- a lane's row is one aligned 32-byte piece, so a step's gather is one memory
// transaction per lane; the rows of one wave's lanes are S * 32 bytes apart (no coalescing across lanes is possible anyway:
// the lanes sit in different states).  The host sees the same [n][S][4] (gu_td_get_q / gu_td_set_q copy it as it is).
// All arithmetic is float64 with one rounding per operation (__dadd_rn / __dmul_rn; the library builds with
// -ffp-contract=off as well), so the tables are bit-exact against the CPU restatement.
#include "gu_rollout.hpp"  // (gu_map.hpp, gu_blocks, gu_lds_block)

#include <algorithm>

#define GU_RNG_STREAM_TD 4u

struct TdArgs {
    const uint8_t *cell;
    int32_t cell_bytes, W;
    uint64_t lut;
    int32_t *pos, *reward, *done;
    uint32_t *episode;
    const uint32_t *tcount;  // per-env step-count offsets (read only: the count advances with the host's lock-step counter)
    const int32_t *starts;
    uint32_t n_starts, seed_prefix, env_id0;
    int64_t N;
    int32_t T, S;
    uint64_t steps_taken;
    double *q;               // [N][S][4]
    int8_t *next_a;          // [N] SARSA: the action carried to the next launch (-1: none)
    int32_t carry;           // 1: this launch directly follows a SARSA launch on the same engine -- start with next_a
    double alpha, gamma;
    uint32_t eps_q16;        // explore iff (word >> 16) < eps_q16; 65536 = always
    int32_t *tr_obs, *tr_reward, *tr_done;  // GU_F_TRAJECTORY: [T][N] planes, as the rollout writes them (else nullptr)
    int32_t *ret, *episodes_fin;            // GU_F_STATS (else nullptr)
    uint64_t *done_bits;
    GridSel gs;
};

struct TdRow {
    double v0, v1, v2, v3;
};

__device__ __forceinline__ TdRow gu_td_load(const double *row)
{
    const double2 lo = reinterpret_cast<const double2 *>(row)[0], hi = reinterpret_cast<const double2 *>(row)[1];
    return TdRow{lo.x, lo.y, hi.x, hi.y};
}

// (selects, not an indexed array: the row must stay in registers)
__device__ __forceinline__ double gu_td_get(const TdRow &q, uint32_t a)
{
    return a == 0u ? q.v0 : a == 1u ? q.v1 : a == 2u ? q.v2 : q.v3;
}

__device__ __forceinline__ void gu_td_put(TdRow &q, uint32_t a, double v)
{
    q.v0 = a == 0u ? v : q.v0;
    q.v1 = a == 1u ? v : q.v1;
    q.v2 = a == 2u ? v : q.v2;
    q.v3 = a == 3u ? v : q.v3;
}

// the row maximum, folded left to right with `>` (a NaN entry other than the first never wins)
__device__ __forceinline__ double gu_td_max(const TdRow &q)
{
    double mx = q.v0;
    mx = q.v1 > mx ? q.v1 : mx;
    mx = q.v2 > mx ? q.v2 : mx;
    return q.v3 > mx ? q.v3 : mx;
}

// epsilon-greedy on one row with one RNG word: explore iff (w >> 16) < eps_q16, then action w & 3; else the k-th (ascending) of
// the m actions whose value equals the row maximum exactly, k = (((w >> 2) & 0x3FFF) * m) >> 14.  (m = 0 -- only a NaN in
// action 0 can make it -- falls back to w & 3.)
__device__ __forceinline__ uint32_t gu_td_action(const TdRow &q, uint32_t w, uint32_t eps_q16)
{
    const double mx = gu_td_max(q);
    const uint32_t e0 = q.v0 == mx, e1 = q.v1 == mx, e2 = q.v2 == mx, e3 = q.v3 == mx;
    const uint32_t m = e0 + e1 + e2 + e3;
    const uint32_t k = (((w >> 2) & 0x3FFFu) * m) >> 14;
    // position of the k-th set bit of e0 e1 e2 e3
    uint32_t a = w & 3u;
    a = (e0 && k == 0u) ? 0u : a;
    a = (e1 && k == e0) ? 1u : a;
    a = (e2 && k == e0 + e1) ? 2u : a;
    a = (e3 && k == e0 + e1 + e2) ? 3u : a;
    return (w >> 16) < eps_q16 ? (w & 3u) : a;
}

template <bool SARSA, bool LDS>
__global__ void __launch_bounds__(GU_BLOCK) gu_td_kernel(const TdArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    CellMap m = gu_stage_map<LDS>(a.cell, a.cell_bytes, smem, a.gs);
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int32_t d = 0;
    if (e < a.N) {
        const LaneGrid lg = gu_lane_grid<LDS>(a.gs, a.starts, a.n_starts, (uint32_t)e, m);
        const uint32_t env = a.env_id0 + (uint32_t)e;
        const uint32_t start_prefix = gu_rng_prefix(a.seed_prefix, env);  // stream 1: keyed by the episode count, no epoch
        uint64_t t = a.steps_taken + (uint64_t)(int64_t)(int32_t)a.tcount[e];
        // stream 4: the epoch t >> 32 hashed behind the seed, hoisted; recomputed in the step that crosses a multiple of 2^32
        uint32_t prefix = gu_rng_prefix(gu_rng_seed_prefix_epoch(a.seed_prefix, (uint32_t)(t >> 32)), env);
        double *qe = a.q + (int64_t)e * a.S * 4;
        int32_t s = a.pos[e], r = a.reward[e];
        d = a.done[e];
        uint32_t ep = a.episode[e];
        TdRow q{0.0, 0.0, 0.0, 0.0};
        if (!d) q = gu_td_load(qe + (int64_t)s * 4);
        int32_t act = (SARSA && a.carry) ? (int32_t)a.next_a[e] : -1;
        int32_t ret = 0, fin = 0;
        for (int32_t i = 0; i < a.T; ++i) {
            if (d) {  // lazy auto-reset, as gu_step_kernel does it under GU_F_AUTO_RESET
                s = lg.starts[gu_rng_start_index(start_prefix, ep, lg.n_starts)];
                ++ep;
                d = 0;
                q = gu_td_load(qe + (int64_t)s * 4);
                act = -1;
            }
            if (act < 0) act = (int32_t)gu_td_action(q, gu_rng_word(prefix, GU_RNG_STREAM_TD, (uint32_t)t), a.eps_q16);
            const uint32_t ua = (uint32_t)act;
            const int32_t s2 = gu_move(s, m.f[s], ua, gu_delta<LDS>(ua, a.lut, a.W));
            r = m.r[s2];
            d = (m.f[s2] >> GU_CELL_TERM_BIT) & 1;
            ++t;
            if ((uint32_t)t == 0u) prefix = gu_rng_prefix(gu_rng_seed_prefix_epoch(a.seed_prefix, (uint32_t)(t >> 32)), env);
            TdRow n = q;  // pre-update Q[s']: the row in registers on a wall bump; not needed behind a terminal s'
            if (!d && s2 != s) n = gu_td_load(qe + (int64_t)s2 * 4);
            int32_t a2 = -1;
            double mval = 0.0;
            if (SARSA) {
                if (!d) {
                    a2 = (int32_t)gu_td_action(n, gu_rng_word(prefix, GU_RNG_STREAM_TD, (uint32_t)t), a.eps_q16);
                    mval = gu_td_get(n, (uint32_t)a2);
                }
            } else {
                mval = gu_td_max(n);
            }
            const double target = d ? (double)r : __dadd_rn((double)r, __dmul_rn(a.gamma, mval));
            double qa = gu_td_get(q, ua);
            qa = __dadd_rn(qa, __dmul_rn(a.alpha, __dsub_rn(target, qa)));
            qe[(int64_t)s * 4 + ua] = qa;
            if (s2 == s) gu_td_put(n, ua, qa);
            q = n;
            s = s2;
            act = a2;
            if (a.tr_obs) {
                const int64_t row = (int64_t)i * a.N + e;
                a.tr_obs[row] = s2;
                a.tr_reward[row] = r;
                a.tr_done[row] = d;
            }
            ret += r;
            fin += d;
        }
        a.pos[e] = s;
        a.reward[e] = r;
        a.done[e] = d;
        a.episode[e] = ep;
        if (SARSA) a.next_a[e] = (int8_t)act;
        if (a.ret) {
            a.ret[e] = ret;
            a.episodes_fin[e] = fin;
        }
    }
    const uint64_t bits = __ballot(d != 0);
    if ((threadIdx.x & 63) == 0 && e < a.N) a.done_bits[e >> 6] = bits;
}

__global__ void __launch_bounds__(256) gu_td_fill_kernel(double *__restrict__ q, size_t n, double v)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) q[i] = v;
}

int gu_td_fill(gu_engine *h, double q0)
{
    const size_t n = (size_t)h->N * (size_t)h->td_S * 4;
    const unsigned blocks = (unsigned)std::min<size_t>((n + 255) / 256, (size_t)h->n_cu * 16);
    hipLaunchKernelGGL(gu_td_fill_kernel, dim3(blocks), dim3(256), 0, h->stream, h->d_q, n, q0);
    GU_HIP(hipGetLastError());
    return GU_OK;
}

template <bool SARSA>
static void gu_td_dispatch(gu_engine *h, const TdArgs &a)
{
    const int lds_bs = gu_lds_block(h, GU_BLOCK, 2);
    if (lds_bs)
        hipLaunchKernelGGL((gu_td_kernel<SARSA, true>), dim3(gu_blocks(h->N, lds_bs)), dim3(lds_bs), 2 * (size_t)h->cell_bytes, h->stream, a);
    else
        hipLaunchKernelGGL((gu_td_kernel<SARSA, false>), dim3(gu_blocks(h->N, GU_BLOCK)), dim3(GU_BLOCK), 0, h->stream, a);
}

int gu_launch_td(gu_engine *h, int64_t T, int32_t method, double alpha, double gamma, uint32_t eps_q16, uint32_t flags)
{
    const bool traj = flags & GU_F_TRAJECTORY, stats = flags & GU_F_STATS;
    const int64_t rows = traj ? h->traj_T * h->N : 0;
    TdArgs a{};
    a.cell = h->d_cell;
    a.cell_bytes = h->cell_bytes;
    a.W = h->W;
    a.lut = h->delta_lut;
    a.pos = h->pos();
    a.reward = h->reward();
    a.done = h->done();
    a.episode = h->d_episode;
    a.tcount = h->d_tcount;
    a.starts = h->d_starts;
    a.n_starts = (uint32_t)h->n_starts;
    a.seed_prefix = h->seed_prefix;
    a.env_id0 = (uint32_t)h->env_id0;
    a.N = h->N;
    a.T = (int32_t)T;
    a.S = h->S;
    a.steps_taken = h->steps_taken;
    a.q = h->d_q;
    a.next_a = h->d_td_next;
    a.carry = (method == 1 && h->td_carry) ? 1 : 0;
    a.alpha = alpha;
    a.gamma = gamma;
    a.eps_q16 = eps_q16;
    a.tr_obs = traj ? h->d_traj : nullptr;
    a.tr_reward = traj ? h->d_traj + rows : nullptr;
    a.tr_done = traj ? h->d_traj + 2 * rows : nullptr;
    a.ret = stats ? h->d_ret : nullptr;
    a.episodes_fin = stats ? h->d_episodes_fin : nullptr;
    a.done_bits = h->d_done_bits;
    a.gs = gu_grid_sel(h);
    if (method == 1) gu_td_dispatch<true>(h, a);
    else gu_td_dispatch<false>(h, a);
    GU_HIP(hipGetLastError());
    h->steps_taken += (uint64_t)T;
    h->entry_table_ok = false;
    h->td_carry = method == 1;
    if (traj) h->traj_written = 1;
    return gu_trail_after_rollout(h, T, traj ? 1 : 0, true);
}
