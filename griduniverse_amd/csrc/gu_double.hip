// gu_double.hip -- batched tabular Double Q-learning for gfx950 (Sutton & Barto 6.7; include/gu.h: gu_double_run; restated on the
// CPU by tests/_double_oracle.py).  Learner e owns env e and a PAIR of float64 tables A_e, B_e: it acts epsilon-greedily on A + B,
// and a coin per step says which of the two learns -- from the other's estimate of its own greedy action at s'.  The lane, its RNG
// word, the move, the trajectory rows and the statistics are gu_tabular.hpp's (TabLane without its Q-row loads: a single row's
// load, forward and write-back do not fit a pair); what is here is the pair, the coin and the rule.
//
// Pairs: learner-major [N][S][2][4] -- the A row and the B row of one state are one aligned 64-byte piece, half a 128-byte line, so
// a step's only dependent gather is still one memory transaction per lane: four 16-byte loads issued together.  The host sees the
// same layout (gu_double_get_q / gu_double_set_q copy it as it is).  The pair of the current state stays in VGPRs from step to step
// (16 of them); a wall bump forwards the updated entry into it, a terminal s' reads nothing, and a step writes the one entry it
// changed (8 bytes).  N * S * 64 bytes pass 4 GiB at 65536 envs x 1024 states: every offset is 64 bits wide.
// The coin is bit 0 of the word of RNG stream 10 at the step's count t -- one more hash per step, independent of the stream-4 one.
#include "gu_tabular.hpp"

#include <algorithm>

struct DoubleArgs : TabArgs {
    double *dq;  // [N][S][2][4]
};

__device__ __forceinline__ void gu_pair_load(const double *p, QRow &A, QRow &B)
{
    const double2 *v = reinterpret_cast<const double2 *>(p);
    const double2 a0 = v[0], a1 = v[1], b0 = v[2], b1 = v[3];
    A = QRow{a0.x, a0.y, a1.x, a1.y};
    B = QRow{b0.x, b0.y, b1.x, b1.y};
}

__device__ __forceinline__ QRow gu_q_pick(bool second, const QRow &x, const QRow &y)
{
    return QRow{second ? y.v0 : x.v0, second ? y.v1 : x.v1, second ? y.v2 : x.v2, second ? y.v3 : x.v3};
}

template <bool LDS>
__global__ void __launch_bounds__(GU_BLOCK) gu_double_kernel(const DoubleArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    TabLane<LDS, false> L(a, smem);
    if (L.e < a.N) {
        L.begin(a);
        double *pe = a.dq + L.e * (int64_t)a.S * 8;
        QRow A{0.0, 0.0, 0.0, 0.0}, B{0.0, 0.0, 0.0, 0.0};  // A_e[s], B_e[s]
        if (!L.d) gu_pair_load(pe + (int64_t)L.s * 8, A, B);
        for (int32_t i = 0; i < a.T; ++i) {
            if (L.d) {
                L.reset(a);
                gu_pair_load(pe + (int64_t)L.s * 8, A, B);
            }
            // ---- rules 1 and 2: the action on A + B, and the coin (both words at the count before the move)
            const QRow ab{__dadd_rn(A.v0, B.v0), __dadd_rn(A.v1, B.v1), __dadd_rn(A.v2, B.v2), __dadd_rn(A.v3, B.v3)};
            const uint32_t ua = gu_q_action(ab, L.word(), a.eps_q16);
            const bool coin = gu_rng_word(L.prefix, GU_RNG_STREAM_DOUBLE, (uint32_t)L.t) & 1u;  // false: A learns from B; true: B from A
            // ---- rule 3
            const int32_t s2 = L.move(a, ua);
            const bool bump = s2 == L.s;
            QRow nA = A, nB = B;
            if (!L.d && !bump) gu_pair_load(pe + (int64_t)s2 * 8, nA, nB);
            // ---- rule 4: X learns, Y estimates
            const QRow X = gu_q_pick(coin, nA, nB), Y = gu_q_pick(coin, nB, nA);
            const double mx = gu_q_max(X);
            const uint32_t as = X.v0 == mx ? 0u : X.v1 == mx ? 1u : X.v2 == mx ? 2u : X.v3 == mx ? 3u : 0u;
            const double est = gu_q_get(Y, as);
            const double target = L.d ? (double)L.r : __dadd_rn((double)L.r, __dmul_rn(a.gamma, est));
            double qa = coin ? gu_q_get(B, ua) : gu_q_get(A, ua);
            qa = __dadd_rn(qa, __dmul_rn(a.alpha, __dsub_rn(target, qa)));
            // ---- rule 5
            pe[(int64_t)L.s * 8 + (coin ? 4 : 0) + ua] = qa;
            gu_q_put(nA, (bump && !coin) ? ua : 4u, qa);  // (4: no entry)
            gu_q_put(nB, (bump && coin) ? ua : 4u, qa);
            A = nA;
            B = nB;
            L.step(a, i, s2, L.q);
        }
        L.end(a);
    }
    L.ballot(a);
}

__global__ void __launch_bounds__(256) gu_double_fill_kernel(double *__restrict__ q, size_t n, double v)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) q[i] = v;
}

static int gu_launch_double(gu_engine *h, int64_t T, double alpha, double gamma, uint32_t eps_q16, uint32_t flags)
{
    DoubleArgs a{};
    gu_tabular_args(h, a, T, alpha, gamma, eps_q16, flags);
    a.q = nullptr;
    a.dq = h->d_dq;
    const int rc = gu_tabular_launch(h, gu_double_kernel<true>, gu_double_kernel<false>, a, GU_BLOCK, 0, 2);
    return rc != GU_OK ? rc : gu_tabular_after(h, T, flags);
}

void gu_double_free(gu_engine *h)
{
    gu_release(h->d_dq);
    h->dq_S = 0;
}

#define GU_NEED_PAIRS(h) GU_REQUIRE(GU_HAS_PAIRS(h), GU_ERR_STATE, "no pairs of Q tables: call gu_double_init first")

extern "C" {

int gu_double_init(gu_handle h, double q0)
{
    GU_ENTER(h);
    GU_NEED_GRID(h);
    GU_REQUIRE(std::isfinite(q0), GU_ERR_INVALID, "q0 must be finite");
    const size_t n = (size_t)h->N * (size_t)h->S * 8, bytes = n * sizeof(double);
    if (!h->d_dq || h->dq_S != h->S) {
        GU_HIP(hipStreamSynchronize(h->stream));
        gu_double_free(h);
        GU_TRY(gu_tabular_fits(h, bytes, "pairs of Q tables"));
        GU_HIP(hipMalloc(&h->d_dq, bytes));
        h->dq_S = h->S;
    }
    const unsigned blocks = (unsigned)std::min<size_t>((n + 255) / 256, (size_t)h->n_cu * 16);
    hipLaunchKernelGGL(gu_double_fill_kernel, dim3(blocks), dim3(256), 0, h->stream, h->d_dq, n, q0);
    GU_HIP(hipGetLastError());
    GU_HIP(hipStreamSynchronize(h->stream));
    return GU_OK;
}

int gu_double_run(gu_handle h, int64_t T, double alpha, double gamma, uint32_t eps_q16, uint32_t flags)
{
    GU_ENTER(h);
    GU_NO_OVERLAY(h, "gu_double_run");
    GU_NEED_GRID(h);
    GU_NEED_PAIRS(h);
    int rc = gu_tabular_check(h, "gu_double_run", T, -1, eps_q16, alpha, gamma, flags);
    if (rc != GU_OK || T == 0) return rc;
    return gu_launch_double(h, T, alpha, gamma, eps_q16, flags);
}

static int gu_double_range(gu_engine *h, int64_t env0, int64_t n, const void *q)
{
    GU_NEED_GRID(h);
    GU_NEED_PAIRS(h);
    GU_REQUIRE(q != nullptr, GU_ERR_INVALID, "q is NULL");
    return gu_env_range(h, env0, n);
}

int gu_double_get_q(gu_handle h, int64_t env0, int64_t n, double *q)
{
    GU_ENTER(h);
    GU_TRY(gu_double_range(h, env0, n, q));
    return gu_env_copy(h, hipMemcpyDeviceToHost, q, h->d_dq, env0, n, (size_t)h->S * 8);
}

int gu_double_set_q(gu_handle h, int64_t env0, int64_t n, const double *q)
{
    GU_ENTER(h);
    GU_TRY(gu_double_range(h, env0, n, q));
    return gu_env_copy(h, hipMemcpyHostToDevice, q, h->d_dq, env0, n, (size_t)h->S * 8);
}

}  // extern "C"
