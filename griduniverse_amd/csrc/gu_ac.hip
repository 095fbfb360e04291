// gu_ac.hip -- batched tabular one-step actor-critic with a softmax policy for gfx950 (Sutton & Barto 13.5; include/gu.h:
// gu_ac_run; restated on the CPU by tests/_ac_oracle.py).  The lane, its RNG word, the move, the trajectory rows and the
// statistics are gu_tabular.hpp's; the softmax, its exp and the reciprocal 1 / Z are gu_softmax.hpp's.  What is here is the
// critic (one float64 state value per (env, state)) and the actor (one float64 preference row per (env, state)).
//
// Tables: preferences [N][S][4] in TabArgs::q -- TabLane addresses, loads and keeps the row of the current state exactly as it
// does a Q row -- and values [N][S] beside it.  Per real step the lane
//   - computes the softmax of the row it holds (4 gu_exp, 1 reciprocal) and draws its action from the stream-4 word of t,
//   - moves, then gathers H[s'] (two 16-byte loads) and V[s'] (8 bytes) together: one dependent round trip, none behind a
//     terminal s', and none on a wall bump (s' == s), where the updated row and value are forwarded in registers instead,
//   - writes V[s] (8 bytes) and the whole row H[s] (32 bytes: two 16-byte stores).
#include "gu_softmax.hpp"

#include <algorithm>

struct AcArgs : TabArgs {
    double *v;        // [N][S] state values (TabArgs::q holds the preferences, TabArgs::alpha the actor's rate)
    double alpha_c;   // the critic's rate
};

template <bool LDS>
__global__ void __launch_bounds__(GU_BLOCK) gu_ac_kernel(const AcArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    TabLane<LDS> L(a, smem);
    if (L.e < a.N) {
        L.begin(a);
        double *ve = a.v + L.e * a.S;
        double vs = L.d ? 0.0 : ve[L.s];  // V[s], kept with the row of s
        for (int32_t i = 0; i < a.T; ++i) {
            const bool reset = L.d != 0;
            L.reset(a);
            if (reset) vs = ve[L.s];
            // 2-3. policy and action
            const SoftRow p = gu_softmax_row(L.q);
            const uint32_t ua = gu_softmax_action(p, L.word());
            // 4. move; the gathers of H[s'] and V[s'] go out together
            const int32_t s2 = L.move(a, ua);
            QRow n = L.next_row(s2);
            double v2 = vs;
            if (!L.d && s2 != L.s) v2 = ve[s2];
            const double iz = gu_recip14(p.Z);
            // 5-6. TD error and critic
            const double target = L.d ? (double)L.r : __dadd_rn((double)L.r, __dmul_rn(a.gamma, v2));
            const double delta = __dsub_rn(target, vs);
            const double vn = __dadd_rn(vs, __dmul_rn(a.alpha_c, delta));
            ve[L.s] = vn;
            // 7. actor: H[s][b] += g ([b = a] - pi_b), pi_b = e_b / Z
            const double g = __dmul_rn(a.alpha, delta);
            QRow h = L.q;
            h.v0 = __dadd_rn(h.v0, __dmul_rn(g, __dsub_rn(ua == 0u ? 1.0 : 0.0, __dmul_rn(p.e0, iz))));
            h.v1 = __dadd_rn(h.v1, __dmul_rn(g, __dsub_rn(ua == 1u ? 1.0 : 0.0, __dmul_rn(p.e1, iz))));
            h.v2 = __dadd_rn(h.v2, __dmul_rn(g, __dsub_rn(ua == 2u ? 1.0 : 0.0, __dmul_rn(p.e2, iz))));
            h.v3 = __dadd_rn(h.v3, __dmul_rn(g, __dsub_rn(ua == 3u ? 1.0 : 0.0, __dmul_rn(p.e3, iz))));
            double2 *row = reinterpret_cast<double2 *>(L.qe + (int64_t)L.s * 4);
            row[0] = make_double2(h.v0, h.v1);
            row[1] = make_double2(h.v2, h.v3);
            // 8. wall bump: the next step sees the updated row and value
            if (s2 == L.s) {
                n = h;
                v2 = vn;
            }
            L.step(a, i, s2, n);
            vs = v2;
        }
        L.end(a);
    }
    L.ballot(a);
}

__global__ void __launch_bounds__(256) gu_ac_fill_kernel(double *__restrict__ p, size_t n, double x)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = x;
}

static void gu_ac_fill_one(gu_engine *h, double *p, size_t n, double x)
{
    const unsigned blocks = (unsigned)std::max<size_t>(1, std::min<size_t>((n + 255) / 256, (size_t)h->n_cu * 16));
    hipLaunchKernelGGL(gu_ac_fill_kernel, dim3(blocks), dim3(256), 0, h->stream, p, n, x);
}

static int gu_ac_fill(gu_engine *h, double h0, double v0)
{
    const size_t nv = (size_t)h->N * (size_t)h->ac_S;
    gu_ac_fill_one(h, h->d_ac_h, nv * 4, h0);
    gu_ac_fill_one(h, h->d_ac_v, nv, v0);
    GU_HIP(hipGetLastError());
    return GU_OK;
}

static int gu_launch_ac(gu_engine *h, int64_t T, double alpha_actor, double alpha_critic, double gamma, uint32_t flags)
{
    AcArgs a{};
    gu_tabular_args(h, a, T, alpha_actor, gamma, 0u, flags);
    a.q = h->d_ac_h;
    a.v = h->d_ac_v;
    a.alpha_c = alpha_critic;
    const int rc = gu_tabular_launch(h, gu_ac_kernel<true>, gu_ac_kernel<false>, a);
    return rc != GU_OK ? rc : gu_tabular_after(h, T, flags);
}

void gu_ac_free(gu_engine *h)
{
    gu_release(h->d_ac_h, h->d_ac_v);
    h->ac_S = 0;
    gu_reinforce_free(h);
}

extern "C" {

int gu_ac_init(gu_handle h, double h0, double v0)
{
    GU_ENTER(h);
    GU_NEED_GRID(h);
    GU_REQUIRE(std::isfinite(h0) && std::isfinite(v0), GU_ERR_INVALID, "h0 and v0 must be finite");
    gu_tabular_drop_carry(h);
    if (!h->d_ac_h || h->ac_S != h->S) {
        GU_HIP(hipStreamSynchronize(h->stream));
        gu_ac_free(h);
        const size_t states = (size_t)h->N * (size_t)h->S;
        GU_TRY(gu_tabular_fits(h, states * 5 * sizeof(double), "actor-critic tables"));
        GU_HIP(hipMalloc(&h->d_ac_h, states * 4 * sizeof(double)));
        GU_HIP(hipMalloc(&h->d_ac_v, states * sizeof(double)));
        h->ac_S = h->S;
    }
    GU_TRY(gu_ac_fill(h, h0, v0));  // every preference = h0, every value = v0 (async)
    GU_HIP(hipStreamSynchronize(h->stream));
    return GU_OK;
}

int gu_ac_run(gu_handle h, int64_t T, double alpha_actor, double alpha_critic, double gamma, uint32_t flags)
{
    GU_ENTER(h);
    GU_NO_OVERLAY(h, "gu_ac_run");
    GU_NEED_GRID(h);
    GU_NEED_AC(h);
    GU_REQUIRE(std::isfinite(alpha_critic), GU_ERR_INVALID, "alpha_critic must be finite");
    int rc = gu_tabular_check(h, "gu_ac_run", T, -1, 0u, alpha_actor, gamma, flags);
    if (rc != GU_OK || T == 0) return rc;
    return gu_launch_ac(h, T, alpha_actor, alpha_critic, gamma, flags);
}

static int gu_ac_range(gu_engine *h, int64_t env0, int64_t n, const void *pref, const void *v)
{
    GU_NEED_GRID(h);
    GU_NEED_AC(h);
    GU_REQUIRE(pref != nullptr || v != nullptr, GU_ERR_INVALID, "pref and v are both NULL");
    return gu_env_range(h, env0, n);
}

int gu_ac_get(gu_handle h, int64_t env0, int64_t n, double *pref, double *v)
{
    GU_ENTER(h);
    GU_TRY(gu_ac_range(h, env0, n, pref, v));
    GU_TRY(gu_env_copy(h, hipMemcpyDeviceToHost, pref, h->d_ac_h, env0, n, (size_t)h->S * 4));
    return gu_env_copy(h, hipMemcpyDeviceToHost, v, h->d_ac_v, env0, n, (size_t)h->S, false);
}

int gu_ac_set(gu_handle h, int64_t env0, int64_t n, const double *pref, const double *v)
{
    GU_ENTER(h);
    GU_TRY(gu_ac_range(h, env0, n, pref, v));
    const size_t S = (size_t)h->S, k = (size_t)n * S;
    if (pref)
        for (size_t i = 0; i < 4 * k; ++i) GU_REQUIRE(std::isfinite(pref[i]), GU_ERR_INVALID, "pref[%zu] is not finite", i);
    if (v)
        for (size_t i = 0; i < k; ++i) GU_REQUIRE(std::isfinite(v[i]), GU_ERR_INVALID, "v[%zu] is not finite", i);
    gu_tabular_drop_carry(h);
    GU_TRY(gu_env_copy(h, hipMemcpyHostToDevice, pref, h->d_ac_h, env0, n, S * 4));
    return gu_env_copy(h, hipMemcpyHostToDevice, v, h->d_ac_v, env0, n, S, false);
}

}  // extern "C"
