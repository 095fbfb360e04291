// gu_td.hip -- batched tabular Q-learning and SARSA for gfx950 (include/gu.h: gu_td_run; restated on the CPU by
// tests/_td_oracle.py).  The lane, the Q-row rules, the layout and the rounding are gu_tabular.hpp's; what is here is the update
// rule: Q-learning bootstraps on max_a Q[s'][a], SARSA draws its next action a' from Q[s'] with the next stream-4 word (unless s'
// is terminal), bootstraps on Q[s'][a'] and takes a' in the next step -- across launches too, through next_a.
#include "gu_tabular.hpp"

#include <algorithm>

struct TdArgs : TabArgs {
    int8_t *next_a;  // [N] SARSA: the action carried to the next launch (-1: none)
    int32_t carry;   // 1: this launch directly follows a SARSA launch on the same engine -- start with next_a
};

template <bool SARSA, bool LDS>
__global__ void __launch_bounds__(GU_BLOCK) gu_td_kernel(const TdArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    TabLane<LDS> L(a, smem);
    if (L.e < a.N) {
        L.begin(a);
        int32_t act = (SARSA && a.carry) ? (int32_t)a.next_a[L.e] : -1;
        for (int32_t i = 0; i < a.T; ++i) {
            if (L.d) act = -1;  // a reset drops the carried action
            L.reset(a);
            if (act < 0) act = (int32_t)gu_q_action(L.q, L.word(), a.eps_q16);
            const uint32_t ua = (uint32_t)act;
            const int32_t s2 = L.move(a, ua);
            QRow n = L.next_row(s2);
            int32_t a2 = -1;
            double mval = 0.0;
            if (SARSA) {
                if (!L.d) {
                    a2 = (int32_t)gu_q_action(n, L.word(), a.eps_q16);
                    mval = gu_q_get(n, (uint32_t)a2);
                }
            } else {
                mval = gu_q_max(n);
            }
            const double target = L.d ? (double)L.r : __dadd_rn((double)L.r, __dmul_rn(a.gamma, mval));
            L.update(a, (int64_t)L.s * 4 + ua, ua, s2, n, target);
            act = a2;
            L.step(a, i, s2, n);
        }
        L.end(a);
        if (SARSA) a.next_a[L.e] = (int8_t)act;
    }
    L.ballot(a);
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

int gu_launch_td(gu_engine *h, int64_t T, int32_t method, double alpha, double gamma, uint32_t eps_q16, uint32_t flags)
{
    TdArgs a{};
    gu_tabular_args(h, a, T, alpha, gamma, eps_q16, flags);
    a.next_a = h->d_td_next;
    a.carry = (method == 1 && h->td_carry) ? 1 : 0;
    const int rc = method == 1 ? gu_tabular_launch(h, gu_td_kernel<true, true>, gu_td_kernel<true, false>, a)
                               : gu_tabular_launch(h, gu_td_kernel<false, true>, gu_td_kernel<false, false>, a);
    return rc != GU_OK ? rc : gu_tabular_after(h, T, flags, method == 1);
}
