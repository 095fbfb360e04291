// gu_lambda.hip -- batched tabular SARSA(lambda) and Watkins's Q(lambda) for gfx950 (Sutton & Barto ch. 12, replacing traces
// truncated after K steps; include/gu.h: gu_lambda_run; restated on the CPU by tests/_lambda_oracle.py).  The lane, the Q-row
// rules, the table layout and the rounding are gu_tabular.hpp's; what is here is the trace window and the backward-view update.
//
// The window of a lane -- the pairs s*4+a of ages 1 .. K-1 between iterations -- is a per-lane ring of C int32 slots in LDS,
// stored slot-major across the lanes of the block (slot k of lane x at ring[k * blockDim.x + x]: a wave's 64 lanes read 64
// consecutive words, no two on one bank within a half-wave).  One instantiation per capacity C = 1, 8, 32 and 64; the launch picks
// the smallest that holds K (C = 1 needs no ring: the window is only the pair just taken).  The ring is indexed by the
// wave-uniform iteration counter i: the entry inserted at iteration i sits in slot i mod C, so the entry of age j sits in slot
// (i - j) mod C, and aging is the increment of i.  A slot index and its coefficient P_j are therefore uniform across the wave,
// and the loop over j < K is a uniform loop with per-lane predicates.  Emptying a window (an episode end, the Watkins cut)
// writes nothing: `from`, the first iteration whose entry is live, moves past it.  A replaced pair (rule 5) is overwritten
// with -1 in its slot.  Per iteration:
//   - the pairs of ages 1 .. 8 are read and their entries loaded at the top, in the shadow of the Q[s'] gather (for C <= 8 that
//     is the whole window): one dependent gather per step, as in gu_td_kernel;
//   - after g = alpha * delta, every live pair of age j < K with P_j != 0 is updated, Q[p] += g * P_j, stored at once, and
//     forwarded into the register row of s' where it lies there (the wall bump included); the ages beyond 8 go in groups of 8,
//     each group's loads issued together before its stores (the pairs are distinct, so no load can see a store of its group).
//     Those groups wait on g, so each is one more dependent round trip per step (K = 32: three, K = 64: seven); holding every
//     entry of a 64-slot window in registers or next to its pair in LDS would cost more occupancy than the LDS ring already
//     does (DESIGN.md §14 has the measured rates).
// Between launches the window lives in d_lambda_w ([N][GU_LAMBDA_MAX], index = age), SARSA's a' in d_td_next; they are read
// only when this launch directly follows one of the same method and K (gu_engine::carry).
#include "gu_tabular.hpp"

struct LambdaArgs : TabArgs {
    int32_t *w;               // [N][GU_LAMBDA_MAX] the window, index = age (-1: none); ages >= K are not written
    int8_t *next_a;           // [N] SARSA: the action carried to the next launch (-1: none)
    int32_t K;                // 1 .. C
    int32_t Kp;               // the ages j < Kp have P_j != 0 (1 <= Kp <= K)
    int32_t carry;            // 1: this launch directly follows one of the same method and K -- start with the window and next_a
    double P[GU_LAMBDA_MAX];  // P_0 = 1, P_j = P_{j-1} * (gamma * lambda)
};

constexpr int GU_LAMBDA_GROUP = 8;  // window entries loaded together

// one group of ages j0 .. j0+7: read the pairs (dropping a live copy of the new pair sa: rule 5) and load the entries of the live
// pairs with P_j != 0 (p[u] = -1 for the others)
template <int C>
__device__ __forceinline__ void gu_lambda_gather(const LambdaArgs &a, int32_t *ring, uint32_t bs, int32_t i, int32_t from, int32_t j0,
                                                 int32_t sa, const double *qe, int32_t (&p)[GU_LAMBDA_GROUP], double (&v)[GU_LAMBDA_GROUP])
{
#pragma unroll
    for (int u = 0; u < GU_LAMBDA_GROUP; ++u) {
        const int32_t j = j0 + u;
        int32_t x = -1;
        if (j < a.K) {
            const uint32_t slot = (uint32_t)(i - j) & (uint32_t)(C - 1);
            x = i - j >= from ? ring[slot * bs] : -1;
            if (x == sa) {
                ring[slot * bs] = -1;
                x = -1;
            }
        }
        p[u] = j < a.Kp ? x : -1;
        v[u] = p[u] >= 0 ? qe[p[u]] : 0.0;
    }
}

// ... and their updates Q[p] += g * P_j, stored and forwarded into nr (the row of s') where they lie there
__device__ __forceinline__ void gu_lambda_apply(const LambdaArgs &a, int32_t j0, double g, int32_t s2, double *qe,
                                                const int32_t (&p)[GU_LAMBDA_GROUP], const double (&v)[GU_LAMBDA_GROUP], QRow &nr)
{
#pragma unroll
    for (int u = 0; u < GU_LAMBDA_GROUP; ++u) {
        if (p[u] >= 0) {
            const double x = __dadd_rn(v[u], __dmul_rn(g, a.P[j0 + u]));
            qe[p[u]] = x;
            if ((p[u] >> 2) == s2) gu_q_put(nr, (uint32_t)p[u] & 3u, x);
        }
    }
}

template <bool SARSA, int C, bool LDS>
__global__ void __launch_bounds__(GU_BLOCK) gu_lambda_kernel(const LambdaArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    TabLane<LDS> L(a, smem);
    const uint32_t bs = blockDim.x;
    int32_t *ring = reinterpret_cast<int32_t *>(smem + (LDS ? 2 * a.cell_bytes : 0)) + threadIdx.x;  // slot k at ring[k * bs]
    if (L.e < a.N) {
        L.begin(a);
        const int64_t w0 = L.e * GU_LAMBDA_MAX;
        int32_t act = (SARSA && a.carry) ? (int32_t)a.next_a[L.e] : -1;
        int32_t from = -C;  // entries inserted at iterations >= from are live (a carried entry of age k sits at iteration -k)
        if (C > 1)
            for (int32_t k = 1; k < C; ++k) ring[((uint32_t)(-k) & (uint32_t)(C - 1)) * bs] = (a.carry && k < a.K) ? a.w[w0 + k] : -1;
        for (int32_t i = 0; i < a.T; ++i) {
            if (L.d) act = -1;  // a reset drops the carried action (the window is empty here: the terminal step emptied it)
            L.reset(a);
            if (act < 0) act = (int32_t)gu_q_action(L.q, L.word(), a.eps_q16);
            const uint32_t ua = (uint32_t)act;
            const double qsa = gu_q_get(L.q, ua);
            if (!SARSA && !(qsa == gu_q_max(L.q))) from = i;  // Watkins: a non-greedy action cuts the traces before it
            const int32_t sa = L.s * 4 + act;
            int32_t p[GU_LAMBDA_GROUP];
            double v[GU_LAMBDA_GROUP];
            if (C > 1) gu_lambda_gather<C>(a, ring, bs, i, from, 1, sa, L.qe, p, v);  // goes out ahead of the Q[s'] gather
            const int32_t s2 = L.move(a, ua);
            QRow nr = L.next_row(s2);
            int32_t a2 = -1;
            double mval = 0.0;
            if (SARSA) {
                if (!L.d) {
                    a2 = (int32_t)gu_q_action(nr, L.word(), a.eps_q16);
                    mval = gu_q_get(nr, (uint32_t)a2);
                }
            } else {
                mval = gu_q_max(nr);
            }
            const double target = L.d ? (double)L.r : __dadd_rn((double)L.r, __dmul_rn(a.gamma, mval));
            const double g = __dmul_rn(a.alpha, __dsub_rn(target, qsa));
            // age 0, (s, a) itself: P_0 = 1 and g * 1.0 is g, so this is gu_td_kernel's update
            const double q0 = __dadd_rn(qsa, g);
            L.qe[sa] = q0;
            if (s2 == L.s) gu_q_put(nr, ua, q0);
            if (C > 1) {
                gu_lambda_apply(a, 1, g, s2, L.qe, p, v, nr);
                for (int32_t j0 = 1 + GU_LAMBDA_GROUP; j0 < a.K; j0 += GU_LAMBDA_GROUP) {
                    gu_lambda_gather<C>(a, ring, bs, i, from, j0, sa, L.qe, p, v);
                    gu_lambda_apply(a, j0, g, s2, L.qe, p, v, nr);
                }
                ring[((uint32_t)i & (uint32_t)(C - 1)) * bs] = sa;
            }
            if (L.d) from = i + 1;  // the episode ended: the window is emptied
            act = a2;
            L.step(a, i, s2, nr);
        }
        L.end(a);
        // the window by age: after T iterations the entry of age j sits in slot (T - j) mod C
        a.w[w0] = -1;
        if (C > 1)
            for (int32_t j = 1; j < a.K; ++j) a.w[w0 + j] = a.T - j >= from ? ring[((uint32_t)(a.T - j) & (uint32_t)(C - 1)) * bs] : -1;
        if (SARSA) a.next_a[L.e] = (int8_t)act;
    }
    L.ballot(a);
}

template <bool SARSA, int C>
static int gu_lambda_launch_c(gu_engine *h, const LambdaArgs &a)
{
    // The ring takes C * 4 bytes of LDS per lane, so at C = 64 LDS, not registers, bounds the occupancy: 256 bytes per lane leave
    // room for 512 lanes per CU (2 waves per SIMD) when the map is staged in LDS too -- four blocks of 128 lanes, as many lanes as
    // two blocks of 256 -- and for 640 (five blocks of 128) when the map is read from L2.  C = 32 (128 bytes per lane) leaves room
    // for 1024 lanes.  C = 1 launches as gu_td_kernel does.
    return gu_tabular_launch(h, gu_lambda_kernel<SARSA, C, true>, gu_lambda_kernel<SARSA, C, false>, a, C > 32 ? 128 : GU_BLOCK,
                             C > 1 ? (size_t)C * sizeof(int32_t) : 0);
}

template <bool SARSA>
static int gu_lambda_launch_m(gu_engine *h, const LambdaArgs &a)
{
    return a.K == 1    ? gu_lambda_launch_c<SARSA, 1>(h, a)
           : a.K <= 8  ? gu_lambda_launch_c<SARSA, 8>(h, a)
           : a.K <= 32 ? gu_lambda_launch_c<SARSA, 32>(h, a)
                       : gu_lambda_launch_c<SARSA, GU_LAMBDA_MAX>(h, a);
}

// the carry key of a gu_lambda_run (never 0): the next launch keeps the window only under the same method and K
static inline int32_t gu_lambda_key(int32_t method, int32_t K) { return 1 + method + 2 * K; }

static int gu_launch_lambda(gu_engine *h, int64_t T, int32_t method, int32_t K, double alpha, double gamma, double lambda, uint32_t eps_q16,
                     uint32_t flags)
{
    LambdaArgs a{};
    gu_tabular_args(h, a, T, alpha, gamma, eps_q16, flags);
    const int32_t key = gu_lambda_key(method, K);
    a.w = h->d_lambda_w;
    a.next_a = h->d_td_next;
    a.K = K;
    a.carry = gu_carry_is(h, GU_CARRY_LAMBDA, key) ? 1 : 0;
    // the coefficients, one rounding per multiply (the library builds with -ffp-contract=off)
    const double c = gamma * lambda;
    a.P[0] = 1.0;
    a.Kp = 1;
    for (int32_t j = 1; j < K; ++j) {
        a.P[j] = a.P[j - 1] * c;
        if (a.Kp == j && a.P[j] != 0.0) a.Kp = j + 1;
    }
    const int rc = method == 1 ? gu_lambda_launch_m<true>(h, a) : gu_lambda_launch_m<false>(h, a);
    return rc != GU_OK ? rc : gu_tabular_after(h, T, flags, GuCarry{GU_CARRY_LAMBDA, key});
}

void gu_lambda_free(gu_engine *h)
{
    gu_release(h->d_lambda_w);
    gu_carry_release(h, GU_CARRY_LAMBDA);
}

extern "C" {

int gu_lambda_run(gu_handle h, int64_t T, int32_t method, int32_t K, double alpha, double gamma, double lambda, uint32_t eps_q16,
                  uint32_t flags)
{
    GU_ENTER(h);
    GU_NO_OVERLAY(h, "gu_lambda_run");
    GU_NEED_GRID(h);
    GU_NEED_Q(h);
    GU_REQUIRE(method == 0 || method == 1, GU_ERR_INVALID, "method %d: 0 = Watkins's Q(lambda), 1 = SARSA(lambda)", method);
    GU_REQUIRE(K >= 1 && K <= GU_LAMBDA_MAX, GU_ERR_INVALID, "K %d out of range (1 .. %d)", K, GU_LAMBDA_MAX);
    GU_REQUIRE(lambda >= 0.0 && lambda <= 1.0, GU_ERR_INVALID, "lambda %g outside [0, 1]", lambda);
    int rc = gu_tabular_check(h, "gu_lambda_run", T, -1, eps_q16, alpha, gamma, flags);
    if (rc != GU_OK || T == 0) return rc;
    if (!h->d_lambda_w) {
        const size_t slots = (size_t)h->N * GU_LAMBDA_MAX;
        GU_HIP(hipStreamSynchronize(h->stream));
        GU_TRY(gu_tabular_fits(h, slots * sizeof(int32_t), "trace windows"));
        GU_HIP(hipMalloc(&h->d_lambda_w, slots * sizeof(int32_t)));
    }
    return gu_launch_lambda(h, T, method, K, alpha, gamma, lambda, eps_q16, flags);
}

int gu_lambda_get_window(gu_handle h, int64_t env0, int64_t n, int32_t *sa)
{
    GU_ENTER(h);
    GU_NEED_GRID(h);
    GU_TRY(gu_env_range(h, env0, n));
    GU_REQUIRE(sa != nullptr || n == 0, GU_ERR_INVALID, "sa is NULL");
    const int32_t key = gu_carry_key(h, GU_CARRY_LAMBDA), K = key ? (key - 1) / 2 : 0;  // (gu_lambda_key; 0: the window was dropped)
    GU_HIP(hipStreamSynchronize(h->stream));
    if (K) GU_TRY(gu_env_copy(h, hipMemcpyDeviceToHost, sa, h->d_lambda_w, env0, n, GU_LAMBDA_MAX, false));
    for (int64_t e = 0; e < n; ++e)  // (a dropped window reads as empty, whatever the device copy still holds; ages >= K are not written)
        for (int32_t j = K; j < GU_LAMBDA_MAX; ++j) sa[(size_t)e * GU_LAMBDA_MAX + j] = -1;
    return GU_OK;
}

}  // extern "C"
