// gu_is.hip -- batched off-policy every-visit Monte-Carlo control with weighted importance sampling for gfx950 (Sutton & Barto
// 5.7; include/gu.h: gu_is_run; restated on the CPU by tests/_is_oracle.py).  The lane, its RNG word, the move, the trajectory
// rows and the statistics are gu_tabular.hpp's; the tables are gu_td.hip's (Q [N][S][4]) plus the cumulative weights C of the same
// shape; RECIP is gu_softmax.hpp's gu_is_recip (gu_recip14 on the mantissa).  What is here is the episode buffer, the class of the
// behaviour action and the backward pass at a segment's end, which stops at the first entry that is no longer greedy.
//
// ONE LOOP, TWO LANE MODES (gu_reinforce.hip's structure).  Every turn of the loop a lane does one unit of work:
//   act  : one real step (rules 1-4): the fold of the row it stands on, the epsilon-greedy action and its class, the move, the
//          gather of Q[s'], the append to the buffer, the trajectory row;
//   walk : one entry of the backward pass (rule 5): the gather of Q[s_k], C[s_k][a_k] and the ratio row of the entry's class, the
//          updates of both entries, the fold of the row as it is now, the greedy test and the new weight.
// A pass that ends early or late in one lane never makes the other lanes of the wave wait.  What the two units share is the
// fold of one row -- its maximum, the four equality flags, their count m -- which the act unit needs for the tie rule and the
// class and the walk unit for the greedy test and m_now; it sits between a head and a tail per mode.  The walk's head is the
// expensive half (the reciprocal: four Newton steps and three integer corrections); the act's tail is (RNG word, move, rows).
//
// BUFFER: step-major, [L][N] entries of 8 bytes {s*4+a, r*8+c} (the class c = 0 .. 4 in the low three bits of the second word,
// the reward, an int8, above them: one store per real step, one load per walk unit; S needs no limit of its own).  The walk
// reads entry k-1 while it works on entry k; the newest entry is still in registers when the pass starts.  Between launches the
// count lives in d_is_cnt; it is read only when this launch directly follows a gu_is_run with the same L (gu_engine::carry).
//
// RATIOS: the 20 doubles R[m][c] come from the host, transposed to [c][m-1]: the class is known with the entry, so the walk's
// head loads the 32-byte row of its class beside the Q row (160 bytes in all: they stay in the cache) and the tail picks by
// m_now with three selects.  No division, and no indexed access to kernel arguments.
//
// TabLane keeps the row of the current state in VGPRs.  A pass may rewrite it (an entry with s_k == s'), and only then: the walk
// notes it and the next act unit reloads the row (a terminal step's reset loads its row anyway).
#include "gu_softmax.hpp"

struct IsArgs : TabArgs {
    double *c;         // [N][S][4] cumulative weights
    const double *R;   // [5][4] the ratios, R[c * 4 + m - 1]
    double w_cap;      // the pass ends unless 2^-256 <= W < w_cap
    int2 *buf;         // [L][N] the episode buffers, entry k of env e at k * N + e, oldest first: {s*4+a, r*8+c}
    int32_t *cnt;      // [N] their entries between launches
    int32_t L;         // segment length, 1 .. GU_IS_MAX
    int32_t carry;     // 1: this launch directly follows a gu_is_run with the same L -- start from cnt
};

template <bool LDS>
__global__ void __launch_bounds__(GU_BLOCK) gu_is_kernel(const IsArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    TabLane<LDS> L(a, smem);
    if (L.e < a.N) {
        L.begin(a);
        double *ce = a.c + L.e * a.S * 4;
        int2 *be = a.buf + L.e;  // entry k at be[k * N]
        int32_t cnt = a.carry ? a.cnt[L.e] : 0;
        int32_t i = 0;         // real steps done
        int32_t k = -1;        // walk mode: the entry to update (>= 0), else act mode
        bool stale = false;    // the pass rewrote Q[s] of the state the lane stands in
        int2 ent = make_int2(0, 0), ent_next = make_int2(0, 0);  // entry k, entry k-1
        double G = 0.0, W = 1.0;
        while (i < a.T || k >= 0) {
            const bool walk = k >= 0;
            // ---- heads: the row to fold
            QRow h, rr = QRow{0.0, 0.0, 0.0, 0.0};
            uint32_t uk = 0u;
            if (walk) {
                // 5. one entry of the backward pass: G, C, Q
                const int64_t sa = ent.x;
                const int32_t sk = ent.x >> 2;
                uk = (uint32_t)ent.x & 3u;
                h = gu_q_load(L.qe + (int64_t)sk * 4);
                const double c_old = ce[sa];
                rr = gu_q_load(a.R + (ent.y & 7) * 4);
                if (k > 0) ent_next = be[(int64_t)(k - 1) * a.N];  // one turn ahead
                G = __dadd_rn((double)(ent.y >> 3), __dmul_rn(a.gamma, G));
                const double c_new = __dadd_rn(c_old, W);
                ce[sa] = c_new;
                double qa = gu_q_get(h, uk);
                qa = __dadd_rn(qa, __dmul_rn(__dmul_rn(W, gu_is_recip(c_new)), __dsub_rn(G, qa)));
                L.qe[sa] = qa;
                gu_q_put(h, uk, qa);
                stale = stale || (sk == L.s && !L.d);
            } else {
                L.reset(a);
                if (stale) L.q = gu_q_load(L.qe + (int64_t)L.s * 4);
                stale = false;
                h = L.q;
            }
            // ---- shared: the fold of the row (gu_q_max, the flags of gu_q_action and their count)
            const double mx = gu_q_max(h);
            const uint32_t e0 = h.v0 == mx, e1 = h.v1 == mx, e2 = h.v2 == mx, e3 = h.v3 == mx;
            const uint32_t m = e0 + e1 + e2 + e3;
            // ---- tails
            if (walk) {
                // the greedy test on the row as it is now, then the weight
                const bool greedy = (uk == 0u ? e0 : uk == 1u ? e1 : uk == 2u ? e2 : e3) != 0u;
                W = __dmul_rn(W, m <= 1u ? rr.v0 : m == 2u ? rr.v1 : m == 3u ? rr.v2 : rr.v3);
                const bool on = greedy && W >= 0x1p-256 && W < a.w_cap;
                ent = ent_next;
                k = on ? k - 1 : -1;  // -1 behind the oldest entry or at an early end: back to act mode, the buffer is empty
            } else {
                // 2. the behaviour action (gu_q_action's rule on the flags above) and its class
                const uint32_t w = L.word();
                const uint32_t kk = (((w >> 2) & 0x3FFFu) * m) >> 14;
                uint32_t ua = w & 3u;
                ua = (e0 && kk == 0u) ? 0u : ua;
                ua = (e1 && kk == e0) ? 1u : ua;
                ua = (e2 && kk == e0 + e1) ? 2u : ua;
                ua = (e3 && kk == e0 + e1 + e2) ? 3u : ua;
                ua = (w >> 16) < a.eps_q16 ? (w & 3u) : ua;
                const uint32_t cls = (ua == 0u ? e0 : ua == 1u ? e1 : ua == 2u ? e2 : e3) ? m : 0u;
                // 3. move, append
                const int32_t s2 = L.move(a, ua);
                const QRow n = L.next_row(s2);  // (inside a segment the tables do not change: the row in registers on a wall bump)
                ent = make_int2(L.s * 4 + (int32_t)ua, L.r * 8 + (int32_t)cls);
                be[(int64_t)cnt * a.N] = ent;
                ++cnt;
                L.step(a, i, s2, n);
                ++i;
                // 4-5. segment end: the pass starts at the newest entry, which is still in registers
                if (L.d || cnt == a.L) {
                    G = L.d ? 0.0 : gu_q_max(n);
                    W = 1.0;
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

static int gu_launch_is(gu_engine *h, int64_t T, int32_t L, double gamma, uint32_t eps_q16, double w_cap, uint32_t flags)
{
    IsArgs a{};
    gu_tabular_args(h, a, T, 0.0, gamma, eps_q16, flags);
    a.c = h->d_is_c;
    a.R = h->d_is_R;
    a.w_cap = w_cap;
    a.buf = reinterpret_cast<int2 *>(h->d_is_buf);
    a.cnt = h->d_is_cnt;
    a.L = L;
    a.carry = gu_carry_is(h, GU_CARRY_IS, L) ? 1 : 0;
    const int rc = gu_tabular_launch(h, gu_is_kernel<true>, gu_is_kernel<false>, a);
    return rc != GU_OK ? rc : gu_tabular_after(h, T, flags, GuCarry{GU_CARRY_IS, L});
}

void gu_is_free(gu_engine *h)
{
    gu_release(h->d_is_c, h->d_is_R, h->d_is_buf, h->d_is_cnt);
    h->is_S = 0;
    h->is_eps = -1;
    h->is_cap = 0;
    gu_carry_release(h, GU_CARRY_IS);
}

// R[m][c] = pi(a|s) / b(a|s) for the tie-uniform greedy target (1 / m_now) and the epsilon-greedy behaviour at action time (c of the
// row's maxima tied, the action one of them; c = 0: not one of them), laid out for the kernel as R[c * 4 + m - 1]
static void gu_is_ratios(uint32_t eps_q16, double *R)
{
    const double eps = (double)eps_q16 / 65536.0;
    for (int c = 0; c <= 4; ++c) {
        const double b = c == 0 ? eps * 0.25 : (1.0 - eps) / (double)c + eps * 0.25;
        for (int m = 1; m <= 4; ++m) R[c * 4 + m - 1] = b == 0.0 ? 0.0 : (1.0 / (double)m) / b;
    }
}

#define GU_NEED_WEIGHTS(h) GU_REQUIRE(GU_HAS_WEIGHTS(h), GU_ERR_STATE, "no cumulative weights: call gu_is_init first")

extern "C" {

int gu_is_init(gu_handle h)
{
    GU_ENTER(h);
    GU_NEED_GRID(h);
    GU_NEED_Q(h);
    gu_tabular_drop_carry(h);
    const size_t bytes = (size_t)h->N * (size_t)h->S * 4 * sizeof(double);
    GU_HIP(hipStreamSynchronize(h->stream));
    if (!h->d_is_c || h->is_S != h->S) {
        gu_is_free(h);
        GU_TRY(gu_tabular_fits(h, bytes, "cumulative weights"));
        GU_HIP(hipMalloc(&h->d_is_c, bytes));
        GU_HIP(hipMalloc(&h->d_is_R, 20 * sizeof(double)));
        h->is_S = h->S;
    }
    GU_HIP(hipMemsetAsync(h->d_is_c, 0, bytes, h->stream));
    GU_HIP(hipStreamSynchronize(h->stream));
    return GU_OK;
}

int gu_is_run(gu_handle h, int64_t T, int32_t L, double gamma, uint32_t eps_q16, double w_cap, uint32_t flags)
{
    GU_ENTER(h);
    GU_NO_OVERLAY(h, "gu_is_run");
    GU_NEED_GRID(h);
    GU_NEED_Q(h);
    GU_NEED_WEIGHTS(h);
    GU_REQUIRE(L >= 1 && L <= GU_IS_MAX, GU_ERR_INVALID, "L %d out of range (1 .. %d)", L, GU_IS_MAX);
    GU_REQUIRE(w_cap >= 1.0 && w_cap <= 0x1p256, GU_ERR_INVALID, "w_cap %g outside [1, 2^256]", w_cap);
    int rc = gu_tabular_check(h, "gu_is_run", T, -1, eps_q16, 0.0, gamma, flags);
    if (rc != GU_OK || T == 0) return rc;
    GU_TRY(gu_episode_reserve(h, h->d_is_buf, h->d_is_cnt, h->is_cap, GU_CARRY_IS, L));
    if (h->is_eps != (int64_t)eps_q16) {  // (a launch still in flight reads the table of its own epsilon)
        double R[20];
        gu_is_ratios(eps_q16, R);
        GU_HIP(hipStreamSynchronize(h->stream));
        h->is_eps = -1;
        GU_HIP(hipMemcpy(h->d_is_R, R, sizeof(R), hipMemcpyHostToDevice));
        h->is_eps = (int64_t)eps_q16;
    }
    return gu_launch_is(h, T, L, gamma, eps_q16, w_cap, flags);
}

static int gu_is_range(gu_engine *h, int64_t env0, int64_t n, const void *c)
{
    GU_NEED_GRID(h);
    GU_NEED_Q(h);
    GU_NEED_WEIGHTS(h);
    GU_REQUIRE(c != nullptr, GU_ERR_INVALID, "c is NULL");
    return gu_env_range(h, env0, n);
}

int gu_is_get(gu_handle h, int64_t env0, int64_t n, double *c)
{
    GU_ENTER(h);
    GU_TRY(gu_is_range(h, env0, n, c));
    return gu_env_copy(h, hipMemcpyDeviceToHost, c, h->d_is_c, env0, n, (size_t)h->S * 4);
}

int gu_is_set(gu_handle h, int64_t env0, int64_t n, const double *c)
{
    GU_ENTER(h);
    GU_TRY(gu_is_range(h, env0, n, c));
    const size_t row = (size_t)h->S * 4, k = (size_t)n * row;
    for (size_t i = 0; i < k; ++i)
        GU_REQUIRE(std::isfinite(c[i]) && c[i] >= 0.0, GU_ERR_INVALID, "c[%zu] = %g: every entry must be finite and not negative", i, c[i]);
    gu_tabular_drop_carry(h);
    return gu_env_copy(h, hipMemcpyHostToDevice, c, h->d_is_c, env0, n, row);
}

int gu_is_get_episode(gu_handle h, int64_t env0, int64_t n, int32_t *sa, int32_t *reward, int32_t *cls, int32_t *count)
{
    GU_ENTER(h);
    GU_NEED_GRID(h);
    GU_TRY(gu_env_range(h, env0, n));
    return gu_episode_read(h, h->d_is_buf, h->d_is_cnt, GU_CARRY_IS, GU_IS_MAX, env0, n, sa, reward, cls, true, count);
}

}  // extern "C"
