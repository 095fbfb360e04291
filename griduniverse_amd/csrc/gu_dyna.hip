// gu_dyna.hip -- batched tabular Dyna-Q for gfx950 (Sutton & Barto 8.2): N independent learners, learner e owns env e, its
// float64 table Q_e[S][4] (the gu_td_* tables) and a learned model of its deterministic env, advanced T real steps per launch,
// each followed by P planning updates replayed from the model.  The semantics are build-defined and stated in include/gu.h
// (gu_dyna_run); tests/_dyna_oracle.py restates them on the CPU.
//
// One lane per env, like gu_td.hip.  The real step is gu_td_kernel's Q-learning step unchanged, plus the model update.  The env
// is deterministic, so while the cells are the ones the model was cleared under (no grid install since gu_dyna_init), a pair's
// outcome never changes: the step loads the byte of seen bits of s (N * S bytes in all -- the 8-byte model words are 8 * 4 times
// more, and reading them every step cost the P = 0 path a third of gu_td_run's rate at 65 536 learners) and writes the model
// word, the list entry and the bit on a first observation only.  After a grid install that kept the model, the step loads the
// model word of (s, a) instead and stores it back when it differs.
// Model layout, learner-major like the tables:
//   model [N][S*4] uint64   one word per (s, a): low half the reward (int32), high half s' | done << 31; all ones = unobserved
//   list  [N][S*4] int32    the observed pairs s*4+a in the order of first observation (entries >= count stay -1)
//   count [N] int32
//   seen  [N][S] uint8      bit a of byte s: (s, a) observed
// so a planning update reads one list entry, one model word, the row Q[s'_p] (skipped when d_p) and the entry Q[s_p][a_p], and
// writes that entry back.  List and model do not change during planning, so both are software-pipelined: the list entry of
// update j+2 and the model word of update j+1 are in flight while update j gathers its Q row; what stays on the dependent
// chain per update is one Q gather and the store of the updated entry.  Q loads issued after a store to the same address see
// it (one lane's vector memory operations to one address complete in order), so a planning update reads what the updates
// before it wrote, as the semantics require.
// The current state's row stays in VGPRs across real steps as in gu_td.hip; a planning update that writes an entry of that row
// forwards the value into it, so the next real step chooses its action from the table after planning.
// All arithmetic is float64 with one rounding per operation (__dadd_rn / __dmul_rn, -ffp-contract=off).
#include "gu_rollout.hpp"  // (gu_map.hpp, gu_blocks, gu_lds_block)

#define GU_RNG_STREAM_TD 4u
#define GU_DYNA_UNSEEN (~0ull)

struct DynaArgs {
    const uint8_t *cell;
    int32_t cell_bytes, W;
    uint64_t lut;
    int32_t *pos, *reward, *done;
    uint32_t *episode;
    const uint32_t *tcount;
    const int32_t *starts;
    uint32_t n_starts, seed_prefix, env_id0;
    int64_t N;
    int32_t T, S, P;
    uint64_t steps_taken;
    double *q;           // [N][S][4]
    uint64_t *model;     // [N][S*4]
    int32_t *list;       // [N][S*4]
    int32_t *count;      // [N]
    uint8_t *seen;       // [N][S] bit a of byte s: (s, a) observed
    int32_t exact;       // 1: the model holds only outcomes of the current cells (the seen bits decide); 0: compare every word
    double alpha, gamma;
    uint32_t eps_q16;
    int32_t *tr_obs, *tr_reward, *tr_done;
    int32_t *ret, *episodes_fin;
    uint64_t *done_bits;
    GridSel gs;
};

struct DynaRow {
    double v0, v1, v2, v3;
};

__device__ __forceinline__ DynaRow gu_dyna_load(const double *row)
{
    const double2 lo = reinterpret_cast<const double2 *>(row)[0], hi = reinterpret_cast<const double2 *>(row)[1];
    return DynaRow{lo.x, lo.y, hi.x, hi.y};
}

__device__ __forceinline__ double gu_dyna_get(const DynaRow &q, uint32_t a)
{
    return a == 0u ? q.v0 : a == 1u ? q.v1 : a == 2u ? q.v2 : q.v3;
}

__device__ __forceinline__ void gu_dyna_put(DynaRow &q, uint32_t a, double v)
{
    q.v0 = a == 0u ? v : q.v0;
    q.v1 = a == 1u ? v : q.v1;
    q.v2 = a == 2u ? v : q.v2;
    q.v3 = a == 3u ? v : q.v3;
}

// as gu_td_max: folded left to right with `>`
__device__ __forceinline__ double gu_dyna_max(const DynaRow &q)
{
    double mx = q.v0;
    mx = q.v1 > mx ? q.v1 : mx;
    mx = q.v2 > mx ? q.v2 : mx;
    return q.v3 > mx ? q.v3 : mx;
}

// as gu_td_action (include/gu.h, gu_td_run rule 2)
__device__ __forceinline__ uint32_t gu_dyna_action(const DynaRow &q, uint32_t w, uint32_t eps_q16)
{
    const double mx = gu_dyna_max(q);
    const uint32_t e0 = q.v0 == mx, e1 = q.v1 == mx, e2 = q.v2 == mx, e3 = q.v3 == mx;
    const uint32_t m = e0 + e1 + e2 + e3;
    const uint32_t k = (((w >> 2) & 0x3FFFu) * m) >> 14;
    uint32_t a = w & 3u;
    a = (e0 && k == 0u) ? 0u : a;
    a = (e1 && k == e0) ? 1u : a;
    a = (e2 && k == e0 + e1) ? 2u : a;
    a = (e3 && k == e0 + e1 + e2) ? 3u : a;
    return (w >> 16) < eps_q16 ? (w & 3u) : a;
}

__device__ __forceinline__ uint64_t gu_dyna_pack(int32_t s2, int32_t r, int32_t d)
{
    return (uint64_t)(uint32_t)r | ((uint64_t)((uint32_t)s2 | ((uint32_t)d << 31)) << 32);
}

// stream-5 prefix of planning draw c (epoch c >> 32 hashed behind the seed, then the env)
__device__ __forceinline__ uint32_t gu_dyna_prefix(uint32_t seed_prefix, uint32_t env, uint64_t c)
{
    return gu_rng_prefix(gu_rng_seed_prefix_epoch(seed_prefix, (uint32_t)(c >> 32)), env);
}

// the list index drawn for planning update c: (word * count) >> 32.  The prefix of c's epoch is cached in (pre, epoch) and
// recomputed where c enters another epoch -- a wave-uniform test, the block out of line.
__device__ __forceinline__ uint32_t gu_dyna_pick(uint32_t &pre, uint32_t &epoch, uint32_t seed_prefix, uint32_t env, uint64_t c, uint32_t count)
{
    const uint32_t hi = (uint32_t)(c >> 32);
    if (__builtin_expect(__builtin_amdgcn_ballot_w64(hi != epoch) != 0ull, 0)) {
        const uint32_t p = gu_dyna_prefix(seed_prefix, env, c);
        pre = hi != epoch ? p : pre;
        epoch = hi;
    }
    return __umulhi(gu_rng_word(pre, GU_RNG_STREAM_DYNA, (uint32_t)c), count);
}

template <bool PLAN, bool LDS>
__global__ void __launch_bounds__(GU_BLOCK) gu_dyna_kernel(const DynaArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    CellMap m = gu_stage_map<LDS>(a.cell, a.cell_bytes, smem, a.gs);
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int32_t d = 0;
    if (e < a.N) {
        const LaneGrid lg = gu_lane_grid<LDS>(a.gs, a.starts, a.n_starts, (uint32_t)e, m);
        const uint32_t env = a.env_id0 + (uint32_t)e;
        const uint32_t start_prefix = gu_rng_prefix(a.seed_prefix, env);
        uint64_t t = a.steps_taken + (uint64_t)(int64_t)(int32_t)a.tcount[e];
        uint32_t prefix = gu_rng_prefix(gu_rng_seed_prefix_epoch(a.seed_prefix, (uint32_t)(t >> 32)), env);
        const int64_t SA = (int64_t)a.S * 4;
        double *__restrict__ qe = a.q + e * SA;
        uint64_t *__restrict__ me = a.model + e * SA;
        int32_t *__restrict__ le = a.list + e * SA;
        uint8_t *__restrict__ se = a.seen + e * (int64_t)a.S;
        uint32_t count = (uint32_t)a.count[e];
        // stream 5: the prefix of the epoch of the first planning draw, then cached
        const uint64_t c0 = t * (uint64_t)a.P;
        uint32_t pre5 = PLAN ? gu_dyna_prefix(a.seed_prefix, env, c0) : 0u, epoch5 = (uint32_t)(c0 >> 32);
        int32_t s = a.pos[e], r = a.reward[e];
        d = a.done[e];
        uint32_t ep = a.episode[e];
        DynaRow q{0.0, 0.0, 0.0, 0.0};
        if (!d) q = gu_dyna_load(qe + (int64_t)s * 4);
        int32_t ret = 0, fin = 0;
        for (int32_t i = 0; i < a.T; ++i) {
            if (d) {  // lazy auto-reset, as gu_td_kernel
                s = lg.starts[gu_rng_start_index(start_prefix, ep, lg.n_starts)];
                ++ep;
                d = 0;
                q = gu_dyna_load(qe + (int64_t)s * 4);
            }
            const uint32_t ua = gu_dyna_action(q, gu_rng_word(prefix, GU_RNG_STREAM_TD, (uint32_t)t), a.eps_q16);
            const int32_t sa = s * 4 + (int32_t)ua;
            const int32_t s2 = gu_move(s, m.f[s], ua, gu_delta<LDS>(ua, a.lut, a.W));
            r = m.r[s2];
            d = (m.f[s2] >> GU_CELL_TERM_BIT) & 1;
            const uint64_t t_old = t;
            ++t;
            if ((uint32_t)t == 0u) prefix = gu_rng_prefix(gu_rng_seed_prefix_epoch(a.seed_prefix, (uint32_t)(t >> 32)), env);
            DynaRow n = q;
            if (!d && s2 != s) n = gu_dyna_load(qe + (int64_t)s2 * 4);
            // the model's load goes out behind the Q[s'] gather and lands in its shadow (issued at the top of the step, the wait
            // before the action choice would take its whole latency)
            const uint32_t bits = a.exact ? (uint32_t)se[s] : 0u;
            const uint64_t seen = a.exact ? 0ull : me[sa];
            const double target = d ? (double)r : __dadd_rn((double)r, __dmul_rn(a.gamma, gu_dyna_max(n)));
            double qa = gu_dyna_get(q, ua);
            qa = __dadd_rn(qa, __dmul_rn(a.alpha, __dsub_rn(target, qa)));
            qe[sa] = qa;
            if (s2 == s) gu_dyna_put(n, ua, qa);
            // model update.  While the cells are those the model was cleared under, an observed pair's word can only be
            // written again with the same value: only a first observation writes (word, list entry, seen bit).  After a grid
            // install that kept the model, every observation is compared with the stored word.
            const uint64_t word = gu_dyna_pack(s2, r, d);
            if (a.exact) {
                if (!((bits >> ua) & 1u)) {
                    me[sa] = word;
                    le[count++] = sa;
                    se[s] = (uint8_t)(bits | (1u << ua));
                }
            } else {
                if (seen != word) me[sa] = word;
                if (seen == GU_DYNA_UNSEEN) le[count++] = sa;
            }
            q = n;
            s = s2;
            if (PLAN) {
                // planning: updates c = t_old * P + j, j = 0 .. P-1; pipeline: p0 = the list entry of update j, p1 = that of j+1,
                // w0 = the model word of update j
                const int32_t P = a.P;
                uint64_t c = t_old * (uint64_t)P;
                int32_t p0 = le[gu_dyna_pick(pre5, epoch5, a.seed_prefix, env, c, count)];
                int32_t p1 = P > 1 ? le[gu_dyna_pick(pre5, epoch5, a.seed_prefix, env, c + 1, count)] : p0;
                uint64_t w0 = me[p0];
                for (int32_t j = 0; j < P; ++j) {
                    const uint64_t w1 = j + 1 < P ? me[p1] : w0;
                    const int32_t p2 = j + 2 < P ? le[gu_dyna_pick(pre5, epoch5, a.seed_prefix, env, c + (uint64_t)(j + 2), count)] : p1;
                    const uint32_t hi = (uint32_t)(w0 >> 32);
                    const int32_t sp2 = (int32_t)(hi & 0x7FFFFFFFu), rp = (int32_t)(uint32_t)w0;
                    const bool dp = (hi >> 31) != 0u;
                    double qp = qe[p0];
                    double mx = 0.0;
                    if (!dp) mx = gu_dyna_max(gu_dyna_load(qe + (int64_t)sp2 * 4));
                    const double tgt = dp ? (double)rp : __dadd_rn((double)rp, __dmul_rn(a.gamma, mx));
                    qp = __dadd_rn(qp, __dmul_rn(a.alpha, __dsub_rn(tgt, qp)));
                    qe[p0] = qp;
                    if ((p0 >> 2) == s) gu_dyna_put(q, (uint32_t)p0 & 3u, qp);  // keep the row in VGPRs current
                    p0 = p1;
                    p1 = p2;
                    w0 = w1;
                }
            }
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
        a.count[e] = (int32_t)count;
        if (a.ret) {
            a.ret[e] = ret;
            a.episodes_fin[e] = fin;
        }
    }
    const uint64_t bits = __ballot(d != 0);
    if ((threadIdx.x & 63) == 0 && e < a.N) a.done_bits[e >> 6] = bits;
}

template <bool PLAN>
static void gu_dyna_dispatch(gu_engine *h, const DynaArgs &a)
{
    const int lds_bs = gu_lds_block(h, GU_BLOCK, 2);
    if (lds_bs)
        hipLaunchKernelGGL((gu_dyna_kernel<PLAN, true>), dim3(gu_blocks(h->N, lds_bs)), dim3(lds_bs), 2 * (size_t)h->cell_bytes, h->stream, a);
    else
        hipLaunchKernelGGL((gu_dyna_kernel<PLAN, false>), dim3(gu_blocks(h->N, GU_BLOCK)), dim3(GU_BLOCK), 0, h->stream, a);
}

int gu_launch_dyna(gu_engine *h, int64_t T, int32_t P, double alpha, double gamma, uint32_t eps_q16, uint32_t flags)
{
    const bool traj = flags & GU_F_TRAJECTORY, stats = flags & GU_F_STATS;
    const int64_t rows = traj ? h->traj_T * h->N : 0;
    DynaArgs a{};
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
    a.P = P;
    a.steps_taken = h->steps_taken;
    a.q = h->d_q;
    a.model = h->d_dyna_model;
    a.list = h->d_dyna_list;
    a.count = h->d_dyna_count;
    a.seen = h->d_dyna_seen;
    a.exact = h->dyna_exact ? 1 : 0;
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
    if (P > 0) gu_dyna_dispatch<true>(h, a);
    else gu_dyna_dispatch<false>(h, a);
    GU_HIP(hipGetLastError());
    h->steps_taken += (uint64_t)T;
    h->entry_table_ok = false;
    h->td_carry = false;
    if (traj) h->traj_written = 1;
    return gu_trail_after_rollout(h, T, traj ? 1 : 0, true);
}
