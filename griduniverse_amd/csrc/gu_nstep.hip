// gu_nstep.hip -- batched tabular n-step Q-learning and n-step SARSA for gfx950 (Sutton & Barto ch. 7; include/gu.h: gu_nstep_run;
// restated on the CPU by tests/_nstep_oracle.py).  The lane, the Q-row rules, the table layout and the rounding are
// gu_tabular.hpp's; what is here is the window of pending transitions and the n-step update rule.
//
// The window of a lane -- at most n - 1 pending (s*4+a, r) between iterations, oldest first -- is a shift register of
// compile-time capacity C in VGPRs (ws / wr, indexed by constants only: a runtime-indexed array would live in scratch).  One
// instantiation per capacity 1, 4 and 16; the launch picks the smallest that holds n.  Per iteration:
//   - the pair to update first, (s_0, a_0) -- slot 0, or the pair just chosen when the window is empty -- is known before the
//     move, so its 8-byte entry is loaded at the top and lands in the shadow of the Q[s'] gather: one dependent gather per step,
//     as in gu_td_kernel;
//   - the new transition goes into slot cnt (selects over the C slots);
//   - a full window (cnt == n) folds its n rewards into the bootstrap in a loop over the slots below n: n is a kernel argument,
//     so that test is uniform and the loop costs n float64 multiply-add pairs, not C;
//   - the update of (s_0, a_0) is stored and forwarded into the register row of s' where it lies there (s_0 == s', the wall bump
//     included); slot 0 is dropped by a shift;
//   - at a terminal s' the window is flushed oldest first, each entry's return a bootstrap-free Horner sum; every update after
//     the first reloads its entry, which sees the stores before it (one lane's memory operations to one address complete in
//     order), so a repeated pair compounds.  The row in registers needs no forwarding there: the next iteration resets and
//     loads its row.
// Between launches the window lives in d_nstep_sa / d_nstep_r ([N][GU_NSTEP_MAX]) and d_nstep_cnt, SARSA's a' in d_td_next; they
// are read only when this launch directly follows one of the same method and n (gu_engine::carry).
#include "gu_tabular.hpp"

struct NstepArgs : TabArgs {
    int32_t *w_sa, *w_r;  // [N][GU_NSTEP_MAX] the window, oldest first
    int32_t *w_cnt;       // [N] its entries
    int8_t *next_a;       // [N] SARSA: the action carried to the next launch (-1: none)
    int32_t n;            // 1 .. C
    int32_t carry;        // 1: this launch directly follows one of the same method and n -- start with the window and next_a
};

// Horner over slots k = lim-1 .. 0 (lim <= n <= C; n uniform, lim per lane): G = r_k + gamma * G, one rounding per operation
template <int C>
__device__ __forceinline__ double gu_nstep_fold(const int32_t (&wr)[C], int32_t n, int32_t lim, double gamma, double G)
{
#pragma unroll
    for (int k = C - 1; k >= 0; --k)
        if (k < n) G = k < lim ? __dadd_rn((double)wr[k], __dmul_rn(gamma, G)) : G;
    return G;
}

// drop slot 0
template <int C>
__device__ __forceinline__ void gu_nstep_shift(int32_t (&ws)[C], int32_t (&wr)[C])
{
#pragma unroll
    for (int k = 0; k + 1 < C; ++k) {
        ws[k] = ws[k + 1];
        wr[k] = wr[k + 1];
    }
}

template <bool SARSA, int C, bool LDS>
__global__ void __launch_bounds__(GU_BLOCK) gu_nstep_kernel(const NstepArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    TabLane<LDS> L(a, smem);
    if (L.e < a.N) {
        L.begin(a);
        const int32_t n = a.n;
        const int64_t w0 = L.e * GU_NSTEP_MAX;
        int32_t ws[C], wr[C], cnt = 0, act = -1;
#pragma unroll
        for (int k = 0; k < C; ++k) ws[k] = wr[k] = 0;
        if (a.carry) {
            cnt = a.w_cnt[L.e];
#pragma unroll
            for (int k = 0; k < C; ++k) {
                ws[k] = a.w_sa[w0 + k];
                wr[k] = a.w_r[w0 + k];
            }
            if (SARSA) act = (int32_t)a.next_a[L.e];
        }
        for (int32_t i = 0; i < a.T; ++i) {
            if (L.d) act = -1;  // a reset drops the carried action (the window is empty here: the terminal step flushed it)
            L.reset(a);
            if (act < 0) act = (int32_t)gu_q_action(L.q, L.word(), a.eps_q16);
            const uint32_t ua = (uint32_t)act;
            const int32_t sa = L.s * 4 + act;
            int32_t sa0 = cnt > 0 ? ws[0] : sa;
            double q0 = L.qe[sa0];  // goes out ahead of the Q[s'] gather
            const int32_t s2 = L.move(a, ua);
            QRow nr = L.next_row(s2);
#pragma unroll
            for (int k = 0; k < C; ++k) {
                ws[k] = k == cnt ? sa : ws[k];
                wr[k] = k == cnt ? L.r : wr[k];
            }
            ++cnt;
            int32_t a2 = -1;
            if (!L.d) {
                double B;
                if (SARSA) {
                    a2 = (int32_t)gu_q_action(nr, L.word(), a.eps_q16);
                    B = gu_q_get(nr, (uint32_t)a2);
                } else {
                    B = gu_q_max(nr);
                }
                if (cnt == n) {
                    const double G = gu_nstep_fold(wr, n, n, a.gamma, B);
                    q0 = __dadd_rn(q0, __dmul_rn(a.alpha, __dsub_rn(G, q0)));
                    L.qe[sa0] = q0;
                    if ((sa0 >> 2) == s2) gu_q_put(nr, (uint32_t)sa0 & 3u, q0);
                    gu_nstep_shift(ws, wr);
                    --cnt;
                }
            } else {
                // flush, oldest first.  Starting the fold from 0.0 gives the newest entry r exactly (gamma is finite, so
                // gamma * 0.0 is a zero, and r + (+-0.0) is r -- +0.0 for r = 0 -- in round-to-nearest).
                for (;;) {
                    const double G = gu_nstep_fold(wr, n, cnt, a.gamma, 0.0);
                    q0 = __dadd_rn(q0, __dmul_rn(a.alpha, __dsub_rn(G, q0)));
                    L.qe[sa0] = q0;
                    gu_nstep_shift(ws, wr);
                    if (--cnt == 0) break;
                    sa0 = ws[0];
                    q0 = L.qe[sa0];
                }
            }
            act = a2;
            L.step(a, i, s2, nr);
        }
        L.end(a);
        a.w_cnt[L.e] = cnt;
#pragma unroll
        for (int k = 0; k < C; ++k) {
            a.w_sa[w0 + k] = ws[k];
            a.w_r[w0 + k] = wr[k];
        }
        if (SARSA) a.next_a[L.e] = (int8_t)act;
    }
    L.ballot(a);
}

template <bool SARSA, int C>
static int gu_nstep_launch_c(gu_engine *h, const NstepArgs &a)
{
    return gu_tabular_launch(h, gu_nstep_kernel<SARSA, C, true>, gu_nstep_kernel<SARSA, C, false>, a);
}

template <bool SARSA>
static int gu_nstep_launch_m(gu_engine *h, const NstepArgs &a)
{
    return a.n == 1 ? gu_nstep_launch_c<SARSA, 1>(h, a) : a.n <= 4 ? gu_nstep_launch_c<SARSA, 4>(h, a) : gu_nstep_launch_c<SARSA, GU_NSTEP_MAX>(h, a);
}

// the carry key of a gu_nstep_run (never 0): the next launch keeps the window only under the same method and n
static inline int32_t gu_nstep_key(int32_t method, int32_t n) { return 1 + method + 2 * n; }

static int gu_launch_nstep(gu_engine *h, int64_t T, int32_t method, int32_t n, double alpha, double gamma, uint32_t eps_q16, uint32_t flags)
{
    NstepArgs a{};
    gu_tabular_args(h, a, T, alpha, gamma, eps_q16, flags);
    const int32_t key = gu_nstep_key(method, n);
    a.w_sa = h->d_nstep_sa;
    a.w_r = h->d_nstep_r;
    a.w_cnt = h->d_nstep_cnt;
    a.next_a = h->d_td_next;
    a.n = n;
    a.carry = gu_carry_is(h, GU_CARRY_NSTEP, key) ? 1 : 0;
    const int rc = method == 1 ? gu_nstep_launch_m<true>(h, a) : gu_nstep_launch_m<false>(h, a);
    return rc != GU_OK ? rc : gu_tabular_after(h, T, flags, GuCarry{GU_CARRY_NSTEP, key});
}

void gu_nstep_free(gu_engine *h)
{
    gu_release(h->d_nstep_sa, h->d_nstep_r, h->d_nstep_cnt);
    gu_carry_release(h, GU_CARRY_NSTEP);
}

extern "C" {

int gu_nstep_run(gu_handle h, int64_t T, int32_t method, int32_t n, double alpha, double gamma, uint32_t eps_q16, uint32_t flags)
{
    GU_ENTER(h);
    GU_NO_OVERLAY(h, "gu_nstep_run");
    GU_NEED_GRID(h);
    GU_NEED_Q(h);
    GU_REQUIRE(method == 0 || method == 1, GU_ERR_INVALID, "method %d: 0 = n-step Q-learning, 1 = n-step SARSA", method);
    GU_REQUIRE(n >= 1 && n <= GU_NSTEP_MAX, GU_ERR_INVALID, "n %d out of range (1 .. %d)", n, GU_NSTEP_MAX);
    int rc = gu_tabular_check(h, "gu_nstep_run", T, -1, eps_q16, alpha, gamma, flags);
    if (rc != GU_OK || T == 0) return rc;
    if (!h->d_nstep_sa) {
        const size_t slots = (size_t)h->N * GU_NSTEP_MAX;
        GU_HIP(hipStreamSynchronize(h->stream));
        GU_TRY(gu_tabular_fits(h, 2 * slots * sizeof(int32_t) + (size_t)h->N * sizeof(int32_t), "n-step windows"));
        GU_HIP(hipMalloc(&h->d_nstep_sa, slots * sizeof(int32_t)));
        GU_HIP(hipMalloc(&h->d_nstep_r, slots * sizeof(int32_t)));
        GU_HIP(hipMalloc(&h->d_nstep_cnt, (size_t)h->N * sizeof(int32_t)));
    }
    return gu_launch_nstep(h, T, method, n, alpha, gamma, eps_q16, flags);
}

int gu_nstep_get_window(gu_handle h, int64_t env0, int64_t n, int32_t *sa, int32_t *reward, int32_t *count)
{
    GU_ENTER(h);
    GU_NEED_GRID(h);
    GU_TRY(gu_env_range(h, env0, n));
    const size_t k = (size_t)n * GU_NSTEP_MAX;
    std::vector<int32_t> c(n), w_sa(k), w_r(k);
    GU_HIP(hipStreamSynchronize(h->stream));
    if (gu_carry_key(h, GU_CARRY_NSTEP)) {  // (a dropped window reads as empty, whatever the device copy still holds)
        GU_TRY(gu_env_copy(h, hipMemcpyDeviceToHost, c.data(), h->d_nstep_cnt, env0, n, 1, false));
        GU_TRY(gu_env_copy(h, hipMemcpyDeviceToHost, w_sa.data(), h->d_nstep_sa, env0, n, GU_NSTEP_MAX, false));
        GU_TRY(gu_env_copy(h, hipMemcpyDeviceToHost, w_r.data(), h->d_nstep_r, env0, n, GU_NSTEP_MAX, false));
    }
    for (int64_t e = 0; e < n; ++e)
        for (int32_t j = 0; j < GU_NSTEP_MAX; ++j) {
            const size_t i = (size_t)e * GU_NSTEP_MAX + j;
            if (sa) sa[i] = j < c[e] ? w_sa[i] : -1;
            if (reward) reward[i] = j < c[e] ? w_r[i] : 0;
        }
    if (count)
        for (int64_t e = 0; e < n; ++e) count[e] = c[e];
    return GU_OK;
}

}  // extern "C"
