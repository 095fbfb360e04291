// gu_td.hip -- batched tabular Q-learning, SARSA and Expected SARSA for gfx950 (include/gu.h: gu_td_run, gu_esarsa_run; restated on
// the CPU by tests/_td_oracle.py and tests/_double_oracle.py).  The lane, the Q-row rules, the layout and the rounding are
// gu_tabular.hpp's, the overlays' rules gu_tabular_overlay.hpp's; what is here is the update rule: Q-learning bootstraps on max_a Q[s'][a], SARSA draws its next action a' from
// Q[s'] with the next stream-4 word (unless s' is terminal), bootstraps on Q[s'][a'] and takes a' in the next step -- across launches
// too, through next_a.  Expected SARSA acts as Q-learning does and bootstraps on the mean of Q[s'] under the epsilon-greedy policy:
// pe * (the row's sum) + pg * (its maximum), pe = eps / 4 and pg = 1 - eps from the host -- no division, whatever the number of ties.
#include "gu_tabular_overlay.hpp"  // (gu_tabular.hpp)

#include <algorithm>

struct TdArgs : TabArgs {
    int8_t *next_a;  // [N] SARSA: the action carried to the next launch (-1: none)
    int32_t carry;   // 1: this launch directly follows a SARSA launch on the same engine -- start with next_a
    OverlayLaneArgs ov;  // the engine's overlay (gu_overlay_lane_args; a.cell then holds three planes)
    double pe, pg;    // TD_ESARSA: eps_q16 * 2^-18 and (65536 - eps_q16) * 2^-16, both exact
};

enum TdRule { TD_Q = 0, TD_SARSA = 1, TD_ESARSA = 2 };  // (the first two are gu_td_run's method numbers)

// OV: the engine's overlay (gu_tabular_overlay.hpp); under a MASKED one the table has S << bits rows and the lane learns on row word * S + s
template <TdRule RULE, bool LDS, class OV = NoOverlay>
__global__ void __launch_bounds__(GU_BLOCK) gu_td_kernel(const TdArgs a)
{
    constexpr bool SARSA = RULE == TD_SARSA;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    TabLane<LDS, true, OV> L(a, smem);
    if (L.e < a.N) {
        L.load(a.ov);
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
            } else if (RULE == TD_ESARSA) {
                const double sum = __dadd_rn(__dadd_rn(__dadd_rn(n.v0, n.v1), n.v2), n.v3);
                mval = __dadd_rn(__dmul_rn(a.pe, sum), __dmul_rn(a.pg, gu_q_max(n)));
            } else {
                mval = gu_q_max(n);
            }
            const double target = L.d ? (double)L.r : __dadd_rn((double)L.r, __dmul_rn(a.gamma, mval));
            L.update(a, L.row() * 4 + ua, ua, s2, n, target);
            act = a2;
            L.step(a, i, s2, n);
        }
        L.end(a);
        L.store(a.ov);
        if (SARSA) a.next_a[L.e] = (int8_t)act;
    }
    L.ballot(a);
}

__global__ void __launch_bounds__(256) gu_td_fill_kernel(double *__restrict__ q, size_t n, double v)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) q[i] = v;
}

static int gu_td_fill(gu_engine *h, double q0)  // every entry of every table = q0 (async)
{
    const size_t n = (size_t)h->N * (size_t)h->td_S * 4;
    const unsigned blocks = (unsigned)std::min<size_t>((n + 255) / 256, (size_t)h->n_cu * 16);
    hipLaunchKernelGGL(gu_td_fill_kernel, dim3(blocks), dim3(256), 0, h->stream, h->d_q, n, q0);
    GU_HIP(hipGetLastError());
    return GU_OK;
}

static int gu_launch_td(gu_engine *h, int64_t T, int32_t method, double alpha, double gamma, uint32_t eps_q16, uint32_t flags)
{
    TdArgs a{};
    gu_tabular_args(h, a, T, alpha, gamma, eps_q16, flags);
    a.next_a = h->d_td_next;
    a.carry = (method == 1 && gu_carry_is(h, GU_CARRY_TD_SARSA, 0)) ? 1 : 0;
    gu_overlay_lane_args(h, a, a.ov);
    a.pe = (double)eps_q16 * 0x1p-18, a.pg = (double)(65536u - eps_q16) * 0x1p-16;
    // the overlay and the rule become template arguments here, each once (Expected SARSA is calm only: gu_esarsa_run refuses an overlay)
    int rc = GU_OK;
    auto launch = [&](auto ov) {
        using OV = decltype(ov);
        gu_pick<TD_Q, TD_SARSA, TD_ESARSA>(method, [&](auto rule) {
            constexpr TdRule RULE = (TdRule) decltype(rule)::value;
            if constexpr (RULE != TD_ESARSA || OV::PLANES == 2)
                rc = gu_tabular_launch(h, gu_td_kernel<RULE, true, OV>, gu_td_kernel<RULE, false, OV>, a, GU_BLOCK, 0, OV::PLANES);
        });
    };
    switch (h->overlay) {
    case GU_OVERLAY_WIND: h->overlay_param ? launch(WindOverlay<true>{}) : launch(WindOverlay<false>{}); break;  // (gusts or none)
    case GU_OVERLAY_FRUIT: launch(FruitOverlay{}); break;
    case GU_OVERLAY_DOORS: launch(DoorOverlay{}); break;
    case GU_OVERLAY_BOXES: launch(BoxOverlay{}); break;
    case GU_OVERLAY_ERRANDS: launch(ErrandOverlay{}); break;
    default: launch(NoOverlay{});
    }
    return rc != GU_OK ? rc : gu_tabular_after(h, T, flags, method == 1 ? GuCarry{GU_CARRY_TD_SARSA, 0} : GuCarry{});
}

static void gu_td_free(gu_engine *h)
{
    gu_release(h->d_q, h->d_td_next);
    h->td_S = 0;
    gu_carry_release(h, GU_CARRY_TD_SARSA);
}

static void gu_td_drop(gu_engine *h)  // the Q tables and what hangs on them
{
    gu_td_free(h);
    gu_nstep_free(h);
    gu_lambda_free(h);
    gu_search_free(h);
    gu_mcts_free(h);  // (gu_mcts_init again)
}

void gu_td_rows_changed(gu_engine *h, int32_t bits)
{
    if (h->td_S && (int64_t)h->td_S != ((int64_t)h->S << bits)) gu_td_drop(h);
}

void gu_learners_drop(gu_engine *h, int32_t S)
{
    const bool all = S == 0;
    if (all || (h->td_S && h->td_S != S)) {  // Q tables of another state count belong to another grid: gu_td_init again
        gu_td_drop(h);
    }
    if (all || (h->is_S && h->is_S != S)) gu_is_free(h);  // ... and the cumulative weights: gu_is_init again
    if (all || (h->explore_S && h->explore_S != S)) gu_explore_free(h);  // ... and the visit counts: gu_explore_init again
    if (all || (h->dq_S && h->dq_S != S)) gu_double_free(h);  // ... and the pairs of Double Q-learning: gu_double_init again
    if (all || (h->dyna_S && h->dyna_S != S)) gu_dyna_free(h);  // ... and so does a Dyna-Q model: gu_dyna_init again
    if (all || (h->ac_S && h->ac_S != S)) gu_ac_free(h);  // ... and actor-critic tables (with the REINFORCE buffers): gu_ac_init again
    if (all || (h->fa_S && h->fa_S != S)) gu_fa_free(h);  // ... and features and weights: gu_fa_init again
    if (all) {  // the schedule tables outlive every grid
        gu_release(h->d_explore_tab, h->d_mcts_tab);
        h->explore_C = h->mcts_C = 0;
    }
}

extern "C" {

int gu_td_init(gu_handle h, double q0)
{
    GU_ENTER(h);
    GU_NEED_GRID(h);
    GU_REQUIRE(std::isfinite(q0), GU_ERR_INVALID, "q0 must be finite");
    gu_tabular_drop_carry(h);
    // under fruit a table has a row per (cell, mask): S << F of them (gu_set_fruit), which ten fruits multiply by 1024
    GU_REQUIRE(h->overlay != GU_OVERLAY_BOXES || h->overlay_bits <= 10, GU_ERR_INVALID,
               "boxes of %d bits (boxes x bits per box): gu_td_init learns on S << bits rows and takes at most 10 bits", h->overlay_bits);
    GU_REQUIRE(h->overlay != GU_OVERLAY_ERRANDS || h->overlay_bits <= 10, GU_ERR_INVALID,
               "errands of %d bits (fruits + progress + instruction): gu_td_init learns on S << bits rows and takes at most 10 bits", h->overlay_bits);
    GU_REQUIRE(h->overlay_bits <= 10, GU_ERR_INVALID, "%d fruits: gu_td_init learns on S << F rows and takes at most 10 fruits", h->overlay_bits);
    GU_REQUIRE(GU_TD_ROWS(h) <= 0x7FFFFFFF, GU_ERR_INVALID, "%d states x 2^%d masks: more than 2^31 - 1 rows", h->S, h->overlay_bits);
    const int32_t rows = (int32_t)GU_TD_ROWS(h);
    const size_t bytes = (size_t)h->N * (size_t)rows * 4 * sizeof(double);
    if (!h->d_q || h->td_S != rows) {
        GU_HIP(hipStreamSynchronize(h->stream));
        gu_td_free(h);
        GU_TRY(gu_tabular_fits(h, bytes, "Q tables"));
        GU_HIP(hipMalloc(&h->d_q, bytes));
        GU_HIP(hipMalloc(&h->d_td_next, (size_t)h->N));
        h->td_S = rows;
    }
    GU_HIP(hipMemsetAsync(h->d_td_next, 0xFF, (size_t)h->N, h->stream));
    GU_TRY(gu_td_fill(h, q0));
    GU_HIP(hipStreamSynchronize(h->stream));
    return GU_OK;
}

int gu_td_run(gu_handle h, int64_t T, int32_t method, double alpha, double gamma, uint32_t eps_q16, uint32_t flags)
{
    GU_ENTER(h);
    GU_NEED_GRID(h);
    GU_NEED_TD_Q(h);
    GU_REQUIRE(method == 0 || method == 1, GU_ERR_INVALID, "method %d: 0 = Q-learning, 1 = SARSA", method);
    int rc = gu_tabular_check(h, "gu_td_run", T, -1, eps_q16, alpha, gamma, flags);
    if (rc != GU_OK || T == 0) return rc;
    return gu_launch_td(h, T, method, alpha, gamma, eps_q16, flags);
}

int gu_esarsa_run(gu_handle h, int64_t T, double alpha, double gamma, uint32_t eps_q16, uint32_t flags)
{
    GU_ENTER(h);
    GU_NO_OVERLAY(h, "gu_esarsa_run");
    GU_NEED_GRID(h);
    GU_NEED_Q(h);
    int rc = gu_tabular_check(h, "gu_esarsa_run", T, -1, eps_q16, alpha, gamma, flags);
    if (rc != GU_OK || T == 0) return rc;
    return gu_launch_td(h, T, TD_ESARSA, alpha, gamma, eps_q16, flags);
}

static int gu_td_range(gu_engine *h, int64_t env0, int64_t n, const void *q)
{
    GU_NEED_GRID(h);
    GU_NEED_TD_Q(h);
    GU_REQUIRE(q != nullptr, GU_ERR_INVALID, "q is NULL");
    return gu_env_range(h, env0, n);
}

int gu_td_get_q(gu_handle h, int64_t env0, int64_t n, double *q)
{
    GU_ENTER(h);
    GU_TRY(gu_td_range(h, env0, n, q));
    return gu_env_copy(h, hipMemcpyDeviceToHost, q, h->d_q, env0, n, (size_t)h->td_S * 4);
}

int gu_td_set_q(gu_handle h, int64_t env0, int64_t n, const double *q)
{
    GU_ENTER(h);
    GU_TRY(gu_td_range(h, env0, n, q));
    gu_tabular_drop_carry(h);
    return gu_env_copy(h, hipMemcpyHostToDevice, q, h->d_q, env0, n, (size_t)h->td_S * 4);
}

}  // extern "C"
