// gu_reinforce.hip -- batched tabular REINFORCE with baseline (Monte-Carlo policy gradient) for gfx950 (Sutton & Barto 13.3/13.4;
// include/gu.h: gu_reinforce_run; restated on the CPU by tests/_reinforce_oracle.py).  The lane, its RNG word, the move, the
// trajectory rows and the statistics are gu_tabular.hpp's; the softmax, its exp and the reciprocal 1 / Z are gu_softmax.hpp's; the
// tables are gu_ac.hip's (preferences [N][S][4] as the actor, values [N][S] as the baseline).  What is here is the episode buffer
// and the backward pass at a segment's end.
//
// ONE LOOP, TWO LANE MODES.  Episodes end at different steps in different lanes, so a backward pass written as an inner loop
// would make the other lanes of the wave wait for each lane's pass in turn.  Instead every turn of the loop a lane does one
// unit of work:
//   act  : one real step (rules 1-4): the softmax of the row it stands on, the action, the move, the gather of H[s'], the
//          append to the buffer, the trajectory row;
//   walk : one backward update (rule 5) of the entry k it has reached: the gather of H[s_k] and V[s_k], the softmax of that
//          row, the updates of V[s_k] and H[s_k].
// Both units spend most of their time in the same code -- gu_softmax_row (4 gu_exp) and gu_recip14 on one 32-byte row -- which
// sits between a short head and a short tail per mode, so lanes in different modes share it.  A lane leaves the loop when its
// T real steps are done and no pass is running; no lane waits for another lane's episode end.
//
// BUFFER: step-major, [L][N] entries of 8 bytes {s*4+a, r} (int2: one store per real step, one load per backward update; S
// needs no limit of its own).  Lanes whose counts agree -- all of them until the first episode of the wave ends, and on a maze,
// where few episodes end before L steps, nearly always -- append to and walk back through consecutive words: 512 bytes per
// wave and entry.  Lanes whose counts differ touch a line each, which is what the lane-major layout [N][L] does for every
// append of every lane.  Measured (profiles/reinforce_rate.json): level with lane-major on the open 8x8
// grid, ahead on the 32x32 maze for L > 1 from 65 536 learners on.  The walk reads entry k-1 while it works on entry k (the newest
// entry is still in registers when the pass starts), which takes the entry's load out of the chain entry -> row -> softmax.
// Between launches the count lives in d_rf_cnt; it is read only when this launch directly follows a gu_reinforce_run with the
// same L (gu_engine::carry).
//
// TabLane keeps the row of the current state in VGPRs.  A pass may rewrite it (an entry with s_k == s'), and only then: the
// walk notes it and the next act unit reloads the row (a terminal step's reset loads its row anyway).
#include "gu_softmax.hpp"

struct RfArgs : TabArgs {
    double *v;        // [N][S] state values, the baseline (TabArgs::q holds the preferences, TabArgs::alpha the actor's rate)
    double alpha_b;   // the baseline's rate
    int2 *buf;        // [L][N] the episode buffers, entry k of env e at k * N + e, oldest first: {s*4+a, r}
    int32_t *cnt;     // [N] their entries between launches
    int32_t L;        // segment length, 1 .. GU_REINFORCE_MAX
    int32_t carry;    // 1: this launch directly follows a gu_reinforce_run with the same L -- start from cnt
};

template <bool LDS>
__global__ void __launch_bounds__(GU_BLOCK) gu_reinforce_kernel(const RfArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    TabLane<LDS> L(a, smem);
    if (L.e < a.N) {
        L.begin(a);
        double *ve = a.v + L.e * a.S;
        int2 *be = a.buf + L.e;  // entry k at be[k * N]
        int32_t cnt = a.carry ? a.cnt[L.e] : 0;
        int32_t i = 0;         // real steps done
        int32_t k = -1;        // walk mode: the entry to update (>= 0), else act mode
        bool stale = false;    // the pass rewrote H[s] of the state the lane stands in
        int2 ent = make_int2(0, 0), ent_next = make_int2(0, 0);  // entry k, entry k-1
        double G = 0.0;
        while (i < a.T || k >= 0) {
            const bool walk = k >= 0;
            // ---- head: the row to take the softmax of
            QRow h;
            double vk = 0.0;
            int32_t sk = 0;
            if (walk) {
                sk = ent.x >> 2;
                h = gu_q_load(L.qe + (int64_t)sk * 4);
                vk = ve[sk];
                if (k > 0) ent_next = be[(int64_t)(k - 1) * a.N];  // one turn ahead
            } else {
                L.reset(a);
                if (stale) L.q = gu_q_load(L.qe + (int64_t)L.s * 4);
                stale = false;
                h = L.q;
            }
            // ---- shared: rule 2
            const SoftRow p = gu_softmax_row(h);
            const double iz = gu_recip14(p.Z);
            // ---- tails
            if (walk) {
                // 5. one entry of the backward pass
                const uint32_t ua = (uint32_t)ent.x & 3u;
                G = __dadd_rn((double)ent.y, __dmul_rn(a.gamma, G));
                const double delta = __dsub_rn(G, vk);
                ve[sk] = __dadd_rn(vk, __dmul_rn(a.alpha_b, delta));
                const double g = __dmul_rn(a.alpha, delta);
                h.v0 = __dadd_rn(h.v0, __dmul_rn(g, __dsub_rn(ua == 0u ? 1.0 : 0.0, __dmul_rn(p.e0, iz))));
                h.v1 = __dadd_rn(h.v1, __dmul_rn(g, __dsub_rn(ua == 1u ? 1.0 : 0.0, __dmul_rn(p.e1, iz))));
                h.v2 = __dadd_rn(h.v2, __dmul_rn(g, __dsub_rn(ua == 2u ? 1.0 : 0.0, __dmul_rn(p.e2, iz))));
                h.v3 = __dadd_rn(h.v3, __dmul_rn(g, __dsub_rn(ua == 3u ? 1.0 : 0.0, __dmul_rn(p.e3, iz))));
                double2 *row = reinterpret_cast<double2 *>(L.qe + (int64_t)sk * 4);
                row[0] = make_double2(h.v0, h.v1);
                row[1] = make_double2(h.v2, h.v3);
                stale = stale || (sk == L.s && !L.d);
                ent = ent_next;
                --k;  // -1 behind the oldest entry: back to act mode, the buffer is empty
            } else {
                // 3. action, move, append
                const uint32_t ua = gu_softmax_action(p, L.word());
                const int32_t s2 = L.move(a, ua);
                const QRow n = L.next_row(s2);  // (inside a segment the tables do not change: the row in registers on a wall bump)
                ent = make_int2(L.s * 4 + (int32_t)ua, L.r);
                be[(int64_t)cnt * a.N] = ent;
                ++cnt;
                L.step(a, i, s2, n);
                ++i;
                // 4-5. segment end: the pass starts at the newest entry, which is still in registers
                if (L.d || cnt == a.L) {
                    G = L.d ? 0.0 : ve[s2];
                    k = cnt - 1;
                    cnt = 0;
                }
            }
        }
        L.end(a);
        a.cnt[L.e] = cnt;
    }
    L.ballot(a);
}

static int gu_launch_reinforce(gu_engine *h, int64_t T, int32_t L, double alpha_actor, double alpha_baseline, double gamma, uint32_t flags)
{
    RfArgs a{};
    gu_tabular_args(h, a, T, alpha_actor, gamma, 0u, flags);
    a.q = h->d_ac_h;
    a.v = h->d_ac_v;
    a.alpha_b = alpha_baseline;
    a.buf = reinterpret_cast<int2 *>(h->d_rf_buf);
    a.cnt = h->d_rf_cnt;
    a.L = L;
    a.carry = gu_carry_is(h, GU_CARRY_REINFORCE, L) ? 1 : 0;
    const int rc = gu_tabular_launch(h, gu_reinforce_kernel<true>, gu_reinforce_kernel<false>, a);
    return rc != GU_OK ? rc : gu_tabular_after(h, T, flags, GuCarry{GU_CARRY_REINFORCE, L});
}

void gu_reinforce_free(gu_engine *h)
{
    gu_release(h->d_rf_buf, h->d_rf_cnt);
    h->rf_cap = 0;
    gu_carry_release(h, GU_CARRY_REINFORCE);
}

extern "C" {

int gu_reinforce_run(gu_handle h, int64_t T, int32_t L, double alpha_actor, double alpha_baseline, double gamma, uint32_t flags)
{
    GU_ENTER(h);
    GU_NO_OVERLAY(h, "gu_reinforce_run");
    GU_NEED_GRID(h);
    GU_NEED_AC(h);
    GU_REQUIRE(L >= 1 && L <= GU_REINFORCE_MAX, GU_ERR_INVALID, "L %d out of range (1 .. %d)", L, GU_REINFORCE_MAX);
    GU_REQUIRE(std::isfinite(alpha_baseline), GU_ERR_INVALID, "alpha_baseline must be finite");
    int rc = gu_tabular_check(h, "gu_reinforce_run", T, -1, 0u, alpha_actor, gamma, flags);
    if (rc != GU_OK || T == 0) return rc;
    GU_TRY(gu_episode_reserve(h, h->d_rf_buf, h->d_rf_cnt, h->rf_cap, GU_CARRY_REINFORCE, L));
    return gu_launch_reinforce(h, T, L, alpha_actor, alpha_baseline, gamma, flags);
}

int gu_reinforce_get_episode(gu_handle h, int64_t env0, int64_t n, int32_t *sa, int32_t *reward, int32_t *count)
{
    GU_ENTER(h);
    GU_NEED_GRID(h);
    GU_TRY(gu_env_range(h, env0, n));
    return gu_episode_read(h, h->d_rf_buf, h->d_rf_cnt, GU_CARRY_REINFORCE, GU_REINFORCE_MAX, env0, n, sa, reward, nullptr, false, count);
}

}  // extern "C"
