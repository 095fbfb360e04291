// gu_tabular.hpp -- the core of the batched tabular learners for gfx950 (gu_td.hip: Q-learning, SARSA and Expected SARSA; gu_dyna.hip:
// Dyna-Q; gu_sweep.hip: prioritized sweeping; gu_nstep.hip: n-step Q-learning and SARSA; gu_lambda.hip: SARSA(lambda) and Watkins's
// Q(lambda); gu_search.hip: rollout search; gu_explore.hip: UCB / Thompson; gu_mcts.hip: tree search; gu_is.hip: off-policy
// Monte-Carlo; gu_ac.hip: actor-critic; gu_reinforce.hip: REINFORCE with baseline); gu_double.hip (Double Q-learning, on a pair of
// tables) and gu_fa.hip (semi-gradient SARSA / Q-learning on features) use the lane without its table; gu_eval.hip (greedy evaluation)
// walks with the lane and learns nothing.
// N independent learners, learner e owns env e and its own float64 table Q_e[S][4], advanced T real steps per launch.  The
// semantics are build-defined (the reference has no tabular code) and stated in include/gu.h (gu_td_run, gu_dyna_run, gu_nstep_run).
//
// One lane per env, like the rollout.  Per real step the lane (TabLane)
//   - draws one word of RNG stream 4, keyed by its 64-bit step count t (epsilon test, explore action, tie break),
//   - moves with the engine's rule (gu_move on the staged cell map, absorbing terminal) or its overlay's (gu_tabular_overlay.hpp),
//   - reads the row Q[s'] (32 bytes: two 16-byte loads) -- the only dependent gather of the step -- and
//   - writes back the one updated entry Q[s][a] (8 bytes).
// The row of the current state stays in VGPRs from one step to the next; a wall bump (s' == s) forwards the updated entry
// instead of reading the row back, and a terminal s' (target = r) reads nothing.
// Table layout: learner-major, [N][S][4] -- a lane's row is one aligned 32-byte piece, so a step's gather is one memory
// transaction per lane; the rows of one wave's lanes are S * 32 bytes apart (no coalescing across lanes is possible anyway:
// the lanes sit in different states).  The host sees the same [n][S][4] (gu_td_get_q / gu_td_set_q copy it as it is).
// All arithmetic is float64 with one rounding per operation (__dadd_rn / __dmul_rn; the library builds with
// -ffp-contract=off as well), so the tables are bit-exact against the CPU restatements (tests/_td_oracle.py, _dyna_oracle.py).
// The kernels stay separate (their register footprints differ); each holds only its update rule around the lane code here.
#pragma once
#include "gu_rollout.hpp"  // (gu_map.hpp, gu_blocks, gu_lds_block)

#include <cmath>

// ---- the fields both kernels read (gu_tabular_args fills them) ----
struct TabArgs {
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
    double *q;  // [N][S][4]
    double alpha, gamma;
    uint32_t eps_q16;                       // explore iff (word >> 16) < eps_q16; 65536 = always
    int32_t *tr_obs, *tr_reward, *tr_done;  // GU_F_TRAJECTORY: [T][N] planes, as the rollout writes them (else nullptr)
    int32_t *ret, *episodes_fin;            // GU_F_STATS (else nullptr)
    uint64_t *done_bits;
    GridSel gs;
};

// ---- one Q row ----
struct QRow {
    double v0, v1, v2, v3;
};

__device__ __forceinline__ QRow gu_q_load(const double *row)
{
    const double2 lo = reinterpret_cast<const double2 *>(row)[0], hi = reinterpret_cast<const double2 *>(row)[1];
    return QRow{lo.x, lo.y, hi.x, hi.y};
}

// (selects, not an indexed array: the row must stay in registers)
__device__ __forceinline__ double gu_q_get(const QRow &q, uint32_t a)
{
    return a == 0u ? q.v0 : a == 1u ? q.v1 : a == 2u ? q.v2 : q.v3;
}

__device__ __forceinline__ void gu_q_put(QRow &q, uint32_t a, double v)
{
    q.v0 = a == 0u ? v : q.v0;
    q.v1 = a == 1u ? v : q.v1;
    q.v2 = a == 2u ? v : q.v2;
    q.v3 = a == 3u ? v : q.v3;
}

// the row maximum, folded left to right with `>` (a NaN entry other than the first never wins)
__device__ __forceinline__ double gu_q_max(const QRow &q)
{
    double mx = q.v0;
    mx = q.v1 > mx ? q.v1 : mx;
    mx = q.v2 > mx ? q.v2 : mx;
    return q.v3 > mx ? q.v3 : mx;
}

// epsilon-greedy on one row with one RNG word (include/gu.h, gu_td_run rule 2): explore iff (w >> 16) < eps_q16, then action
// w & 3; else the k-th (ascending) of the m actions whose value equals the row maximum exactly, k = (((w >> 2) & 0x3FFF) * m) >> 14.
// (m = 0 -- only a NaN in action 0 can make it -- falls back to w & 3.)
__device__ __forceinline__ uint32_t gu_q_action(const QRow &q, uint32_t w, uint32_t eps_q16)
{
    const double mx = gu_q_max(q);
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

// ---- the Dyna-Q model word of one (s, a) (gu_dyna.hip records and replays it, gu_sweep.hip sweeps over it): low half the reward
// (int32), high half s' | done << 31; all ones = never observed ----
#define GU_DYNA_UNSEEN (~0ull)

__device__ __forceinline__ uint64_t gu_dyna_pack(int32_t s2, int32_t r, int32_t d)
{
    return (uint64_t)(uint32_t)r | ((uint64_t)((uint32_t)s2 | ((uint32_t)d << 31)) << 32);
}

// ---- the overlay as the lane sees it.  The block of a kernel's arguments that gu_overlay_lane_args (gu_overlay.hip) fills from the slot: ----
struct OverlayLaneArgs {
    uint32_t param;         // gu_engine::overlay_param
    int32_t rows;           // rows of one learner's table (gu_engine::td_S: S << overlay_bits)
    uint32_t *word;         // [N] the envs' words (gu_engine::d_overlay_mask)
    uint32_t init, param2;  // gu_engine::overlay_init (the word of an env that has just been reset) and overlay_param2
};

// ... and no overlay, which lists what a kind supplies (gu_tabular_overlay.hpp holds the five): PLANES of a.cell (2 or 3) and MASKED (the
// table has a row per (cell, word)); load(): its parameters and the env's word, before begin(); begin(): what it derives from the word,
// and the word behind the move = the word; reset(): the word of an env just reset (`ep`: the episode count before the reset); commit():
// step() makes the word behind the move current; key() / key2(): the word and the one behind the move, for row() and row2(); store():
// the env's word, behind end().  A kind with a plane has move() too (TabLane::move), which takes the whole move in the engine's place.
struct NoOverlay {
    static constexpr int PLANES = 2;
    static constexpr bool MASKED = false;
    __device__ __forceinline__ void load(const OverlayLaneArgs &, int64_t) {}
    __device__ __forceinline__ void begin(const uint8_t *) {}
    __device__ __forceinline__ void reset(uint32_t, uint32_t) {}
    __device__ __forceinline__ void commit() {}
    __device__ __forceinline__ uint32_t key() const { return 0u; }
    __device__ __forceinline__ uint32_t key2() const { return 0u; }
    __device__ __forceinline__ void store(const OverlayLaneArgs &, int64_t) const {}
};

// ---- the lane: state, prologue, auto-reset, move, Q[s][a] update, record, epilogue ----
// A kernel constructs it (staging the map), runs begin .. end on live lanes and ballot on all; its own rule sits between move and step.
// ROWS = false (gu_fa.hip): the lane has no table of rows of its own -- begin / reset / next_row read nothing from a.q, and the
// kernel keeps `q` (for gu_fa.hip: the folded row of the current state) itself.
// OV (gu_td.hip and gu_eval.hip set it): the engine's overlay, one of the structs of gu_tabular_overlay.hpp.  The lane stages OV::PLANES planes,
// hands the rule of a move to `ov` and, under OV::MASKED, stands on row ov.key() * S + s of a table of `rows` rows; a wall bump may
// then keep the cell and change the row, so next_row() and update() compare ROWS, not cells.  The kernel calls load() before begin()
// and store() behind end().  The calm instantiations hold none of it.  (Where `ov` stands among the members decides the order of the
// loop's register copies in some instantiations: profiles/learner_overlay_asm.txt.)
template <bool LDS, bool ROWS = true, class OV = NoOverlay>
struct TabLane {
    static constexpr bool MASKED = OV::MASKED;
    CellMap m;
    const uint8_t *wd;  // OV::PLANES == 3: the overlay's plane, behind the two cell planes (gu_engine::d_overlay_cell)
    int32_t S, rows;  // MASKED: states, and rows of one learner's table (S << bits)
    OV ov;
    LaneGrid lg;
    int64_t e;
    uint32_t env, start_prefix, prefix, ep;
    uint64_t t;
    double *qe;
    int32_t s, r, d, ret, fin;
    QRow q;

    __device__ __forceinline__ TabLane(const TabArgs &a, uint8_t *smem)
    {
        m = gu_stage_map<LDS>(a.cell, a.cell_bytes, smem, a.gs, OV::PLANES);
        if (OV::PLANES == 3) wd = m.f + 2 * a.cell_bytes;
        if (MASKED) S = a.S;
        e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
        d = 0;
    }

    __device__ __forceinline__ void load(const OverlayLaneArgs &o) { rows = o.rows, ov.load(o, e); }

    __device__ __forceinline__ void begin(const TabArgs &a)
    {
        lg = gu_lane_grid<LDS>(a.gs, a.starts, a.n_starts, (uint32_t)e, m);
        env = a.env_id0 + (uint32_t)e;
        start_prefix = gu_rng_prefix(a.seed_prefix, env);  // stream 1: keyed by the episode count, no epoch
        t = a.steps_taken + (uint64_t)(int64_t)(int32_t)a.tcount[e];
        // stream 4: the epoch t >> 32 hashed behind the seed, hoisted; recomputed in the step that crosses a multiple of 2^32
        prefix = gu_rng_prefix(gu_rng_seed_prefix_epoch(a.seed_prefix, (uint32_t)(t >> 32)), env);
        qe = ROWS ? a.q + (MASKED ? e * rows : e * a.S) * 4 : nullptr;
        if (OV::PLANES == 3) ov.begin(wd);
        s = a.pos[e];
        r = a.reward[e];
        d = a.done[e];
        ep = a.episode[e];
        q = QRow{0.0, 0.0, 0.0, 0.0};
        if (ROWS && !d) q = gu_q_load(qe + row() * 4);
        ret = 0;
        fin = 0;
    }

    // lazy auto-reset, as gu_step_kernel does it under GU_F_AUTO_RESET
    __device__ __forceinline__ void reset(const TabArgs &a)
    {
        if (d) {
            s = lg.starts[gu_rng_start_index(start_prefix, ep, lg.n_starts)];
            ++ep;
            d = 0;
            ov.reset(start_prefix, ep - 1u);
            if (ROWS) q = gu_q_load(qe + row() * 4);
        }
    }

    // gu_eval.hip, in the place of begin(): the lane stands at the start of test episode k (include/gu.h: gu_td_evaluate, rules 1 and
    // 2) -- what reset() gives a freshly seeded env at episode count k, on cell s0 instead where s0 >= 0, at step count t0 of epoch
    // 0.  Nothing of the env's own state is read.  Call load() first.
    __device__ __forceinline__ void begin_test(const TabArgs &a, uint32_t k, uint32_t t0, int32_t s0)
    {
        lg = gu_lane_grid<LDS>(a.gs, a.starts, a.n_starts, (uint32_t)e, m);
        env = a.env_id0 + (uint32_t)e;
        start_prefix = gu_rng_prefix(a.seed_prefix, env);
        t = t0;
        prefix = gu_rng_prefix(gu_rng_seed_prefix_epoch(a.seed_prefix, 0u), env);
        qe = a.q + (MASKED ? e * rows : e * a.S) * 4;
        ep = k;
        r = ret = fin = 0;
        d = 1;
        reset(a);
        if (s0 >= 0) {
            s = s0;
            q = gu_q_load(qe + row() * 4);
        }
        d = (m.f[s] >> GU_CELL_TERM_BIT) & 1;
    }

    // the table row the lane stands on, and the one it stands on behind move()
    __device__ __forceinline__ int64_t row() const { return MASKED ? (int64_t)ov.key() * S + s : (int64_t)s; }
    __device__ __forceinline__ int64_t row2(int32_t s2) const { return MASKED ? (int64_t)ov.key2() * S + s2 : (int64_t)s2; }

    // the stream-4 word of step t
    __device__ __forceinline__ uint32_t word() const { return gu_rng_word(prefix, GU_RNG_STREAM_TD, (uint32_t)t); }

    // take action ua from s: sets r and d, advances t (re-keying stream 4 where t crosses a multiple of 2^32), returns s'
    __device__ __forceinline__ int32_t move(const TabArgs &a, uint32_t ua)
    {
        int32_t s2;
        if constexpr (OV::PLANES == 3) {
            s2 = ov.template move<LDS>(*this, a, ua);  // the overlay's rule in the place of the engine's
        } else {
            s2 = gu_move(s, m.f[s], ua, gu_delta<LDS>(ua, a.lut, a.W));
            r = m.r[s2];
            d = (m.f[s2] >> GU_CELL_TERM_BIT) & 1;
        }
        ++t;
        if ((uint32_t)t == 0u) prefix = gu_rng_prefix(gu_rng_seed_prefix_epoch(a.seed_prefix, (uint32_t)(t >> 32)), env);
        return s2;
    }

    // pre-update Q[s']: the row in registers on a wall bump; not needed behind a terminal s'
    __device__ __forceinline__ QRow next_row(int32_t s2) const
    {
        QRow n = q;
        if (ROWS && !d && (MASKED ? row2(s2) != row() : s2 != s)) n = gu_q_load(qe + row2(s2) * 4);
        return n;
    }

    // Q[s][ua] += alpha (target - Q[s][ua]) at entry sa = s * 4 + ua, forwarded into n (the row of s') on a wall bump
    __device__ __forceinline__ void update(const TabArgs &a, int64_t sa, uint32_t ua, int32_t s2, QRow &n, double target)
    {
        double qa = gu_q_get(q, ua);
        qa = __dadd_rn(qa, __dmul_rn(a.alpha, __dsub_rn(target, qa)));
        qe[sa] = qa;
        if (MASKED ? row2(s2) == row() : s2 == s) gu_q_put(n, ua, qa);
    }

    // the lane stands in s' with row n: the trajectory row and the statistics of step i
    __device__ __forceinline__ void step(const TabArgs &a, int32_t i, int32_t s2, const QRow &n)
    {
        q = n;
        s = s2;
        ov.commit();
        if (a.tr_obs) {
            const int64_t row = (int64_t)i * a.N + e;
            a.tr_obs[row] = s2;
            a.tr_reward[row] = r;
            a.tr_done[row] = d;
        }
        ret += r;
        fin += d;
    }

    __device__ __forceinline__ void store(const OverlayLaneArgs &o) const { ov.store(o, e); }

    __device__ __forceinline__ void end(const TabArgs &a) const
    {
        a.pos[e] = s;
        a.reward[e] = r;
        a.done[e] = d;
        a.episode[e] = ep;
        if (a.ret) {
            a.ret[e] = ret;
            a.episodes_fin[e] = fin;
        }
    }

    // every lane of the wave, live or not, joins the ballot of done flags
    __device__ __forceinline__ void ballot(const TabArgs &a) const
    {
        const uint64_t bits = __ballot(d != 0);
        if ((threadIdx.x & 63) == 0 && e < a.N) a.done_bits[e >> 6] = bits;
    }
};

// ---- host side ----
// What the learners' entry points share: gu_td.hip, gu_dyna.hip, gu_sweep.hip, gu_nstep.hip, gu_lambda.hip, gu_search.hip, gu_explore.hip,
// gu_mcts.hip, gu_is.hip, gu_ac.hip, gu_reinforce.hip and gu_fa.hip each hold their own extern "C" functions and their gu_*_free;
// the checks, copies and stores they have in common are here.

// the tables that more than one learner's entry points need, present and of this grid's size
#define GU_NEED_Q(h) GU_REQUIRE(GU_HAS_Q(h), GU_ERR_STATE, "no Q tables: call gu_td_init first")
// ... gu_td_run and the table copies alone know the overlays' masks: S << F rows under fruit, S << D under doors (include/gu.h:
// gu_set_fruit, gu_set_doors; GU_TD_ROWS: gu_internal.hpp)
#define GU_NEED_TD_Q(h) GU_REQUIRE(GU_HAS_TD_Q(h), GU_ERR_STATE, "no Q tables: call gu_td_init first")
#define GU_NEED_AC(h) GU_REQUIRE(GU_HAS_AC(h), GU_ERR_STATE, "no actor-critic tables: call gu_ac_init first")

// tables of `bytes` for the engine's envs: what is left has to hold the trajectory buffer and the scratch of other calls too, so
// keep 1 GiB of headroom
static inline int gu_tabular_fits(gu_engine *h, size_t bytes, const char *what)
{
    size_t free_b = 0, total_b = 0;
    GU_HIP(hipMemGetInfo(&free_b, &total_b));
    GU_REQUIRE(bytes + ((size_t)1 << 30) <= free_b, GU_ERR_NOMEM, "%s of %lld envs x %d states need %.2f GiB, %.2f GiB are free", what,
               (long long)h->N, h->S, bytes / 1073741824.0, free_b / 1073741824.0);
    return GU_OK;
}

// the checks of a learner launch of T real steps; P < 0: one update per step, else gu_dyna_run (P + 1 per step)
static inline int gu_tabular_check(gu_engine *h, const char *fn, int64_t T, int32_t P, uint32_t eps_q16, double alpha, double gamma, uint32_t flags)
{
    if (P < 0)
        GU_REQUIRE(T >= 0 && T <= 100000000, GU_ERR_INVALID, "T %lld out of range (0 .. 1e8)", (long long)T);
    else
        GU_REQUIRE(T >= 0 && T <= 100000000 && T * (int64_t)(P + 1) <= 100000000, GU_ERR_INVALID,
                   "T %lld x (P + 1) = %lld updates out of range (0 .. 1e8)", (long long)T, (long long)T * (P + 1));
    GU_REQUIRE(eps_q16 <= 65536u, GU_ERR_INVALID, "eps_q16 %u above 65536", eps_q16);
    GU_REQUIRE(std::isfinite(alpha) && std::isfinite(gamma), GU_ERR_INVALID, "alpha and gamma must be finite");
    GU_REQUIRE((flags & ~(GU_F_TRAJECTORY | GU_F_STATS)) == 0, GU_ERR_INVALID, "%s accepts GU_F_TRAJECTORY and GU_F_STATS only (flags 0x%x)", fn, flags);
    if (flags & GU_F_TRAJECTORY)
        GU_REQUIRE(h->d_traj && T <= h->traj_T, GU_ERR_STATE, "trajectory buffer holds %lld rows, need %lld: call gu_reserve_trajectory",
                   (long long)h->traj_T, (long long)T);
    GU_REQUIRE(!h->trail_cap || (flags & GU_F_TRAJECTORY), GU_ERR_UNSUPPORTED, "the agent trail is on (gu_trail_enable): %s must write rows (GU_F_TRAJECTORY) to feed it", fn);
    return GU_OK;
}

// the budget of a searching launch (gu_search_run, gu_mcts_run): T real steps of at most `moves` moves each, `formula` says which
static inline int gu_move_budget(int64_t T, int64_t moves, const char *formula)
{
    GU_REQUIRE(T * moves <= 100000000, GU_ERR_INVALID, "T %lld x (%s) = %lld moves out of range (0 .. 1e8)", (long long)T, formula,
               (long long)(T * moves));
    return GU_OK;
}

static inline int gu_env_range(gu_engine *h, int64_t env0, int64_t n)
{
    GU_REQUIRE(env0 >= 0 && n >= 0 && env0 + n <= h->N, GU_ERR_INVALID, "envs [%lld, %lld) outside 0 .. %lld", (long long)env0,
               (long long)(env0 + n), (long long)h->N);
    return GU_OK;
}

// Envs env0 .. env0+n-1 of a device array of `row` elements per env, to the host (hipMemcpyDeviceToHost) or from it, behind everything
// queued on the engine's stream (sync = false: the caller has waited already).  Copies nothing for n == 0 or a NULL host pointer.
template <class T>
static int gu_env_copy(gu_engine *h, hipMemcpyKind dir, const T *host, T *dev, int64_t env0, int64_t n, size_t row, bool sync = true)
{
    if (sync) GU_HIP(hipStreamSynchronize(h->stream));
    if (!n || !host) return GU_OK;
    T *at = dev + (size_t)env0 * row;
    const size_t bytes = (size_t)n * row * sizeof(T);
    if (dir == hipMemcpyDeviceToHost)
        GU_HIP(hipMemcpy(const_cast<T *>(host), at, bytes, hipMemcpyDeviceToHost));
    else
        GU_HIP(hipMemcpy(at, host, bytes, hipMemcpyHostToDevice));
    return GU_OK;
}

// ---- episode buffers (gu_reinforce.hip, gu_is.hip): step-major [cap][N] entries of 8 bytes {s*4+a, word} and [N] counts ----
// storage for L entries per env of the learner `owner` (GU_CARRY_*), allocated on first use (a call with another L drops the buffer
// anyway: nothing to keep)
static int gu_episode_reserve(gu_engine *h, int32_t *&buf, int32_t *&cnt, int32_t &cap, int owner, int32_t L)
{
    if (cap >= L) return GU_OK;
    const size_t slots = (size_t)h->N * (size_t)L;
    GU_HIP(hipStreamSynchronize(h->stream));
    GU_TRY(gu_tabular_fits(h, slots * 2 * sizeof(int32_t) + (size_t)h->N * sizeof(int32_t), "episode buffers"));
    gu_release(buf, cnt);
    cap = 0;
    gu_carry_release(h, owner);
    GU_HIP(hipMalloc(&buf, slots * 2 * sizeof(int32_t)));
    GU_HIP(hipMalloc(&cnt, (size_t)h->N * sizeof(int32_t)));
    cap = L;
    return GU_OK;
}

// The buffers of envs env0 .. env0+n-1 of the learner `owner` (GU_CARRY_*) as [n][pitch] rows, entries behind an env's count as
// -1 / 0.  The L entries per env of its carry are live (it owns none: the buffer was dropped and reads as empty, whatever the device
// copy still holds).  The entry's word is the reward, or, `packed`, reward * 8 + class.
static int gu_episode_read(gu_engine *h, const int32_t *buf, const int32_t *cnt, int owner, int32_t pitch, int64_t env0, int64_t n,
                           int32_t *sa, int32_t *reward, int32_t *cls, bool packed, int32_t *count)
{
    const int32_t L = gu_carry_key(h, owner);
    std::vector<int32_t> c(n), w((size_t)n * (size_t)L * 2);
    GU_HIP(hipStreamSynchronize(h->stream));
    if (n && L) {
        GU_HIP(hipMemcpy(c.data(), cnt + env0, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
        GU_HIP(hipMemcpy2D(w.data(), (size_t)n * 8, buf + (size_t)env0 * 2, (size_t)h->N * 8, (size_t)n * 8, (size_t)L,
                           hipMemcpyDeviceToHost));  // rows k = 0 .. L-1 of [L][N], columns env0 .. env0+n-1
    }
    for (int64_t e = 0; e < n; ++e)
        for (int32_t j = 0; j < pitch; ++j) {
            const size_t i = (size_t)e * pitch + j, b = ((size_t)j * n + e) * 2;
            const bool live = j < c[e];
            if (sa) sa[i] = live ? w[b] : -1;
            if (reward) reward[i] = live ? (packed ? w[b + 1] >> 3 : w[b + 1]) : 0;
            if (cls) cls[i] = live ? w[b + 1] & 7 : 0;
        }
    if (count)
        for (int64_t e = 0; e < n; ++e) count[e] = c[e];
    return GU_OK;
}

// ---- schedule tables (gu_explore_set_tables: U | B; gu_mcts_set_tables: U | B | I): nv vectors of C entries, one after the other
// in one device array of whole 16-byte pieces (the LDS kernels stage it so), zero behind the last entry ----
static int gu_schedule_upload(gu_engine *h, double *&tab, int32_t &tab_C, int32_t C, const double *const *v, int nv)
{
    GU_REQUIRE(C >= 2 && C <= GU_EXPLORE_MAX_C, GU_ERR_INVALID, "table size %d out of range (2 .. %d)", C, GU_EXPLORE_MAX_C);
    GU_REQUIRE(v[0] != nullptr && v[1] != nullptr && (nv < 3 || v[2] != nullptr), GU_ERR_INVALID, "%s is NULL", nv < 3 ? "U or B" : "U, B or I");
    for (int32_t k = 0; k < C; ++k) {
        bool ok = true;
        for (int i = 0; i < nv; ++i) ok = ok && std::isfinite(v[i][k]) && v[i][k] >= 0.0;
        if (nv < 3)
            GU_REQUIRE(ok, GU_ERR_INVALID, "entry %d (U %g, B %g): every entry must be finite and not negative", k, v[0][k], v[1][k]);
        else
            GU_REQUIRE(ok, GU_ERR_INVALID, "entry %d (U %g, B %g, I %g): every entry must be finite and not negative", k, v[0][k], v[1][k], v[2][k]);
    }
    GU_HIP(hipStreamSynchronize(h->stream));
    if (tab_C != C) {
        gu_release(tab);
        tab_C = 0;
        const size_t bytes = ((size_t)C * nv * sizeof(double) + 15) & ~(size_t)15;
        GU_HIP(hipMalloc(&tab, bytes));
        GU_HIP(hipMemset(tab, 0, bytes));
        tab_C = C;
    }
    for (int i = 0; i < nv; ++i) GU_HIP(hipMemcpy(tab + (size_t)i * C, v[i], (size_t)C * sizeof(double), hipMemcpyHostToDevice));
    return GU_OK;
}

static inline void gu_tabular_args(gu_engine *h, TabArgs &a, int64_t T, double alpha, double gamma, uint32_t eps_q16, uint32_t flags)
{
    const bool traj = flags & GU_F_TRAJECTORY, stats = flags & GU_F_STATS;
    const int64_t rows = traj ? h->traj_T * h->N : 0;
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
}

// launch the LDS instantiation where every block uses one grid whose planes fit, else the L2 one; blocks of at most `bs` lanes,
// and `lane_lds` bytes of dynamic LDS per lane after the planes (gu_lambda.hip's ring; none for the other learners)
// (`planes`: 3 for the windy instantiations, whose a.cell carries the wind plane behind the two cell planes; `ny`: the launch's second
// dimension -- gu_eval.hip's test episodes; the lanes of every blockIdx.y are the same N envs)
template <class A>
static int gu_tabular_launch(gu_engine *h, void (*lds)(A), void (*l2)(A), const A &a, int bs = GU_BLOCK, size_t lane_lds = 0, int planes = 2, unsigned ny = 1)
{
    const int lds_bs = gu_lds_block(h, bs, planes);
    if (lds_bs) {
        const size_t bytes = (size_t)planes * (size_t)h->cell_bytes + lane_lds * (size_t)lds_bs;
        if (bytes > 64 * 1024) GU_HIP(hipFuncSetAttribute((const void *)lds, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
        hipLaunchKernelGGL(lds, dim3(gu_blocks(h->N, lds_bs), ny), dim3(lds_bs), bytes, h->stream, a);
    } else {
        hipLaunchKernelGGL(l2, dim3(gu_blocks(h->N, bs), ny), dim3(bs), lane_lds * (size_t)bs, h->stream, a);
    }
    GU_HIP(hipGetLastError());
    return GU_OK;
}

// after a launch of T steps: the engine's step count, what the launch leaves for the next one of its kind (`leave`; nothing: every
// carry ends here), rows and statistics, and the agent trail (an error of the trail's still leaves the carry: the launch ran)
static inline int gu_tabular_after(gu_engine *h, int64_t T, uint32_t flags, GuCarry leave = {})
{
    const bool traj = flags & GU_F_TRAJECTORY;
    gu_envs_touched(h, (uint64_t)T);
    h->carry = leave;
    if (traj) h->traj_written = 1;
    const int rc = gu_trail_after_rollout(h, T, traj ? 1 : 0, true);
    if (rc == GU_OK) {
        h->stats_valid = (flags & GU_F_STATS) != 0;
        if (traj) h->traj_kind = 1;
    }
    return rc;
}
