// gu_eval.hip -- batched greedy evaluation of the learners' tables for gfx950 (include/gu.h: gu_td_evaluate; restated on the CPU by
// tests/_eval_oracle.py).  Env e walks K test episodes of at most L steps on its table Q_e, with the move rule the learners use: the
// lane is gu_tabular.hpp's TabLane, the overlays' rules gu_tabular_overlay.hpp's.  What is here is the walk: the first maximum of the
// row, the move, the sums -- no update, no RNG word for the action, and nothing of the engine's state read or written (begin_test()
// stands in for begin(); end(), store(), step() and ballot() are not called).
// One lane per (env, test episode): a 2-D launch with blockIdx.y = k, so the lane's env, its grid and its LDS image still follow from
// blockIdx.x alone, and the device sees K x N lanes where a learner launch has N.  Per step the lane reads the row Q[row2(s')] (32
// bytes: the one dependent gather; the row in registers on a bump) and stores nothing.  A wave leaves the step loop when its last lane
// has ended (one ballot and one scalar branch per step); lanes that ended earlier idle under the exec mask.  The six results are
// written once per lane, coalesced as [k][e] planes, into scratch memory and copied out from there.
#include "gu_tabular_overlay.hpp"  // (gu_tabular.hpp)

struct EvalArgs : TabArgs {  // (T: the L of gu_td_evaluate; gamma: its discount)
    OverlayLaneArgs ov;    // the engine's overlay (gu_overlay_lane_args; a.cell then holds three planes)
    const int32_t *first;  // [K][N] start cells in the place of the drawn ones, or nullptr
    int32_t *o_ret, *o_len, *o_outcome, *o_end;  // [K][N] each
    uint32_t *o_word;
    double *o_disc;
};

// the first of the actions whose value equals the row maximum (rule 3): selects from the last to the first, so the lowest wins; 0 where
// none compares equal
__device__ __forceinline__ uint32_t gu_q_first_max(const QRow &q)
{
    const double mx = gu_q_max(q);
    uint32_t a = 0u;
    a = q.v3 == mx ? 3u : a;
    a = q.v2 == mx ? 2u : a;
    a = q.v1 == mx ? 1u : a;
    return q.v0 == mx ? 0u : a;
}

template <bool LDS, class OV>
__global__ void __launch_bounds__(GU_BLOCK) gu_eval_kernel(const EvalArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    TabLane<LDS, true, OV> L(a, smem);
    const bool live = L.e < a.N;
    const uint32_t k = blockIdx.y;
    const int64_t at = (int64_t)k * a.N + L.e;
    int32_t len = 0;
    double disc = 0.0, w = 1.0;
    L.d = 1;  // (a lane past the batch has ended)
    if (live) {
        L.load(a.ov);
        L.begin_test(a, k, k * (uint32_t)a.T, a.first ? a.first[at] : -1);
    }
    for (int32_t i = 0; i < a.T; ++i) {
        if (__ballot(!L.d) == 0ull) break;
        if (!L.d) {
            const uint32_t ua = gu_q_first_max(L.q);
            const int32_t s2 = L.move(a, ua);
            const QRow n = L.next_row(s2);
            L.q = n;
            L.s = s2;
            L.ov.commit();
            L.ret += L.r;
            disc = __dadd_rn(disc, __dmul_rn(w, (double)L.r));
            w = __dmul_rn(w, a.gamma);
            ++len;
        }
    }
    if (live) {
        const int32_t term = (L.m.f[L.s] >> GU_CELL_TERM_BIT) & 1;
        a.o_ret[at] = L.ret;
        a.o_len[at] = len;
        a.o_outcome[at] = !L.d ? 0 : !term ? 3 : L.m.r[L.s] > 0 ? 1 : 2;
        a.o_end[at] = L.s;
        a.o_word[at] = OV::MASKED ? L.ov.key() : 0u;
        a.o_disc[at] = disc;
    }
}

#define GU_EVAL_MAX_K 65535            /* gridDim.y */
#define GU_EVAL_MAX_LANES (1 << 24)    /* K * N: 28 bytes of results and 4 of start cells each, 512 MiB of scratch at most */

extern "C" int gu_td_evaluate(gu_handle h, int32_t K, int32_t L, double gamma, const int32_t *first_state, int32_t *ret, int32_t *len,
                              int32_t *outcome, int32_t *end, uint32_t *word, double *disc)
{
    GU_ENTER(h);
    GU_NEED_GRID(h);
    GU_NEED_TD_Q(h);
    GU_REQUIRE(K >= 1 && L >= 1 && (int64_t)K * L <= 100000000, GU_ERR_INVALID, "K %d x L %d = %lld steps out of range (K >= 1, L >= 1, K x L <= 1e8)", K, L,
               (long long)K * L);
    GU_REQUIRE(K <= GU_EVAL_MAX_K && (int64_t)K * h->N <= GU_EVAL_MAX_LANES, GU_ERR_INVALID,
               "K %d x %lld envs = %lld test episodes: at most %d per env and %d in all", K, (long long)h->N, (long long)K * h->N, GU_EVAL_MAX_K, GU_EVAL_MAX_LANES);
    GU_REQUIRE(std::isfinite(gamma), GU_ERR_INVALID, "gamma must be finite");
    const size_t kn = (size_t)K * (size_t)h->N;
    if (first_state)
        for (size_t i = 0; i < kn; ++i)
            GU_REQUIRE(first_state[i] >= 0 && first_state[i] < h->S, GU_ERR_INVALID, "first_state[%lld][%lld] = %d outside 0 .. %d", (long long)(i / (size_t)h->N),
                       (long long)(i % (size_t)h->N), first_state[i], h->S - 1);
    GU_TRY(gu_ensure_scratch(h, kn * 32));
    EvalArgs a{};
    gu_tabular_args(h, a, L, 0.0, gamma, 0u, 0u);
    gu_overlay_lane_args(h, a, a.ov);
    a.o_disc = reinterpret_cast<double *>(h->d_scratch);
    a.o_ret = reinterpret_cast<int32_t *>(a.o_disc + kn);
    a.o_len = a.o_ret + kn, a.o_outcome = a.o_len + kn, a.o_end = a.o_outcome + kn;
    a.o_word = reinterpret_cast<uint32_t *>(a.o_end + kn);
    int32_t *d_first = reinterpret_cast<int32_t *>(a.o_word + kn);
    GU_HIP(hipStreamSynchronize(h->stream));
    if (first_state) GU_HIP(hipMemcpy(d_first, first_state, kn * sizeof(int32_t), hipMemcpyHostToDevice));
    a.first = first_state ? d_first : nullptr;
    // the overlay becomes a template argument here, as in gu_launch_td
    int rc = GU_OK;
    auto launch = [&](auto ov) {
        using OV = decltype(ov);
        rc = gu_tabular_launch(h, gu_eval_kernel<true, OV>, gu_eval_kernel<false, OV>, a, GU_BLOCK, 0, OV::PLANES, (unsigned)K);
    };
    switch (h->overlay) {
    case GU_OVERLAY_WIND: h->overlay_param ? launch(WindOverlay<true>{}) : launch(WindOverlay<false>{}); break;  // (gusts or none)
    case GU_OVERLAY_FRUIT: launch(FruitOverlay{}); break;
    case GU_OVERLAY_DOORS: launch(DoorOverlay{}); break;
    case GU_OVERLAY_BOXES: launch(BoxOverlay{}); break;
    case GU_OVERLAY_ERRANDS: launch(ErrandOverlay{}); break;
    default: launch(NoOverlay{});
    }
    GU_TRY(rc);
    GU_HIP(hipStreamSynchronize(h->stream));
    if (disc) GU_HIP(hipMemcpy(disc, a.o_disc, kn * sizeof(double), hipMemcpyDeviceToHost));
    int32_t *const dst[5] = {ret, len, outcome, end, reinterpret_cast<int32_t *>(word)};
    for (int i = 0; i < 5; ++i)
        if (dst[i]) GU_HIP(hipMemcpy(dst[i], a.o_ret + (size_t)i * kn, kn * sizeof(int32_t), hipMemcpyDeviceToHost));
    return GU_OK;
}
