// gu_explore.hip -- batched count-based exploration for gfx950: UCB and Thompson-style Q-learning (include/gu.h: gu_explore_run;
// restated on the CPU by tests/_explore_oracle.py).  Learner e owns env e, its gu_td_* table and a table of visit counts
// N_e[S][4]; it learns by gu_td_kernel's Q-learning step and chooses its non-exploring actions greedily on a SCORE row: the Q row
// plus a bonus that shrinks with the counts (mode 0), or plus noise whose width shrinks with them (mode 1).  The lane, the Q-row
// rules and the rounding are gu_tabular.hpp's; what is here is the count row, the two schedule tables and the score.
//
// COUNTS: uint32, learner-major [N][S][4] -- a lane's row is one aligned 16-byte piece.  The lane keeps the count row of the state
// it stands in in VGPRs beside the Q row.  The count row of s' is loaded where next_row loads the Q row and under the same
// conditions: an independent 16-byte gather in the shadow of the 32-byte one (both addresses come from s' alone).  A wall bump
// forwards the incremented count, a terminal s' reads nothing, and a step writes back the one count it changed (4 bytes).
//
// THE SCHEDULE IS DATA: U[C] and B[C], float64, shared by all learners, turn counts into the bonus u * B[n_b], u = U[n_s], both
// indices clamped to C - 1 -- the kernel has no log, sqrt or division, only float64 multiplies and adds with one rounding each.
// The LDS kernels stage U | B (16 C bytes) behind the cell planes when planes + tables stay within the share of a CU's LDS that
// leaves room for 2048 lanes (80 bytes per lane: 20 KiB for a block of 256, which holds a 32x32 map and tables of 1024), so the
// tables never cost a wave of occupancy; larger tables -- and the L2-map kernels -- read them through L2, where 5 loads per step
// of a table that every wave of the chip shares stay cache hits.
//
// MODE 1 draws four approximate normals per step from ONE hashed word of RNG stream 7 (counter t, keyed like stream 4): x_0 is the
// word, x_{b+1} = gu_rng_sample_next(x_b), z_b = (the sum of the four bytes of x_b) - 510 -- an Irwin-Hall sum, variance 21845; the
// host folds 1 / sqrt(21845) into B.  The byte sum is one v_sad_u8.
// Every lane computes the score row, exploring or not (gu_q_action drops it behind the epsilon test): the table reads and the
// stream-7 hash are wave-uniform code, and a per-lane branch around them would run both sides in most waves anyway.
#include "gu_tabular.hpp"

struct ExploreArgs : TabArgs {
    uint32_t *cnt;      // [N][S][4] visit counts
    const double *tab;  // U[C] | B[C]
    int32_t C;
    int32_t tab_lds;    // bytes of tab the LDS kernels stage behind the planes (0: read it through L2)
};

__device__ __forceinline__ uint32_t gu_cnt_get(const uint4 &c, uint32_t a)
{
    return a == 0u ? c.x : a == 1u ? c.y : a == 2u ? c.z : c.w;
}

__device__ __forceinline__ void gu_cnt_put(uint4 &c, uint32_t a, uint32_t v)
{
    c.x = a == 0u ? v : c.x;
    c.y = a == 1u ? v : c.y;
    c.z = a == 2u ? v : c.z;
    c.w = a == 3u ? v : c.w;
}

// u and the four B entries of count row c from table t (U | B), indices clamped to C - 1
__device__ __forceinline__ void gu_explore_lookup(const double *t, uint32_t C, const uint4 &c, double &u, QRow &b)
{
    const uint32_t top = C - 1u;
    u = t[min(c.x + c.y + c.z + c.w, top)];  // (counts saturate at GU_EXPLORE_COUNT_MAX: the sum fits 32 bits)
    t += C;
    b = QRow{t[min(c.x, top)], t[min(c.y, top)], t[min(c.z, top)], t[min(c.w, top)]};
}

// the Irwin-Hall variate of word x: the sum of its four bytes, centred
__device__ __forceinline__ double gu_explore_z(uint32_t x) { return (double)((int32_t)__builtin_amdgcn_sad_u8(x, 0u, 0u) - 510); }

template <int MODE, bool LDS>
__global__ void __launch_bounds__(GU_BLOCK) gu_explore_kernel(const ExploreArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const double *ltab = reinterpret_cast<const double *>(smem + 2 * a.cell_bytes);
    if (LDS && a.tab_lds)  // (the barrier behind the planes, in TabLane's constructor, covers these stores too)
        for (int32_t i = threadIdx.x * 16; i < a.tab_lds; i += blockDim.x * 16)
            *reinterpret_cast<uint4 *>(smem + 2 * a.cell_bytes + i) = *reinterpret_cast<const uint4 *>(reinterpret_cast<const uint8_t *>(a.tab) + i);
    TabLane<LDS> L(a, smem);
    if (L.e < a.N) {
        L.begin(a);
        uint32_t *ne = a.cnt + L.e * (int64_t)a.S * 4;
        uint4 c = make_uint4(0u, 0u, 0u, 0u);  // N_e[s]
        if (!L.d) c = *reinterpret_cast<const uint4 *>(ne + (int64_t)L.s * 4);
        for (int32_t i = 0; i < a.T; ++i) {
            if (L.d) {
                L.reset(a);
                c = *reinterpret_cast<const uint4 *>(ne + (int64_t)L.s * 4);
            }
            const uint32_t w = L.word();
            // ---- rule 3: the score row
            double u;
            QRow b;
            if (LDS && a.tab_lds)
                gu_explore_lookup(ltab, (uint32_t)a.C, c, u, b);
            else
                gu_explore_lookup(a.tab, (uint32_t)a.C, c, u, b);
            QRow p{__dmul_rn(u, b.v0), __dmul_rn(u, b.v1), __dmul_rn(u, b.v2), __dmul_rn(u, b.v3)};
            if (MODE == 1) {
                const uint32_t x0 = gu_rng_word(L.prefix, GU_RNG_STREAM_EXPLORE, (uint32_t)L.t);
                const uint32_t x1 = gu_rng_sample_next(x0), x2 = gu_rng_sample_next(x1), x3 = gu_rng_sample_next(x2);
                p = QRow{__dmul_rn(p.v0, gu_explore_z(x0)), __dmul_rn(p.v1, gu_explore_z(x1)), __dmul_rn(p.v2, gu_explore_z(x2)),
                         __dmul_rn(p.v3, gu_explore_z(x3))};
            }
            const QRow sc{__dadd_rn(L.q.v0, p.v0), __dadd_rn(L.q.v1, p.v1), __dadd_rn(L.q.v2, p.v2), __dadd_rn(L.q.v3, p.v3)};
            const uint32_t ua = gu_q_action(sc, w, a.eps_q16);
            // ---- rule 4: the count, on exploring steps too
            const uint32_t cn = min(gu_cnt_get(c, ua) + 1u, (uint32_t)GU_EXPLORE_COUNT_MAX);
            const int64_t sa = (int64_t)L.s * 4 + ua;
            // ---- rule 5: gu_td_kernel's Q-learning step, the count row of s' beside the Q row
            const int32_t s2 = L.move(a, ua);
            QRow n = L.next_row(s2);
            gu_cnt_put(c, ua, cn);  // (forwarded on a wall bump; replaced otherwise, or by the reset behind a terminal s')
            if (!L.d && s2 != L.s) c = *reinterpret_cast<const uint4 *>(ne + (int64_t)s2 * 4);
            const double target = L.d ? (double)L.r : __dadd_rn((double)L.r, __dmul_rn(a.gamma, gu_q_max(n)));
            L.update(a, sa, ua, s2, n, target);
            ne[sa] = cn;
            L.step(a, i, s2, n);
        }
        L.end(a);
    }
    L.ballot(a);
}

template <int MODE>
static int gu_explore_launch(gu_engine *h, ExploreArgs &a)
{
    const int lds_bs = gu_lds_block(h, GU_BLOCK, 2);
    if (lds_bs) {
        // the tables go into LDS only where LDS then still admits 2048 lanes per CU (the wave limit): lds_per_cu / 2048 bytes per lane
        const size_t planes = 2 * (size_t)h->cell_bytes, tab = (size_t)a.C * 2 * sizeof(double);
        const size_t budget = (size_t)h->lds_per_cu / 2048 * (size_t)lds_bs;
        a.tab_lds = planes + tab <= budget ? (int32_t)tab : 0;
        hipLaunchKernelGGL((gu_explore_kernel<MODE, true>), dim3(gu_blocks(h->N, lds_bs)), dim3(lds_bs), planes + (size_t)a.tab_lds, h->stream, a);
    } else {
        a.tab_lds = 0;
        hipLaunchKernelGGL((gu_explore_kernel<MODE, false>), dim3(gu_blocks(h->N, GU_BLOCK)), dim3(GU_BLOCK), 0, h->stream, a);
    }
    GU_HIP(hipGetLastError());
    return GU_OK;
}

static int gu_launch_explore(gu_engine *h, int64_t T, int32_t mode, double alpha, double gamma, uint32_t eps_q16, uint32_t flags)
{
    ExploreArgs a{};
    gu_tabular_args(h, a, T, alpha, gamma, eps_q16, flags);
    a.cnt = h->d_explore_n;
    a.tab = h->d_explore_tab;
    a.C = h->explore_C;
    const int rc = mode == 1 ? gu_explore_launch<1>(h, a) : gu_explore_launch<0>(h, a);
    return rc != GU_OK ? rc : gu_tabular_after(h, T, flags);
}

void gu_explore_free(gu_engine *h)
{
    gu_release(h->d_explore_n);
    h->explore_S = 0;
}

#define GU_NEED_COUNTS(h) GU_REQUIRE(GU_HAS_COUNTS(h), GU_ERR_STATE, "no visit counts: call gu_explore_init first")

extern "C" {

int gu_explore_init(gu_handle h)
{
    GU_ENTER(h);
    GU_NEED_GRID(h);
    GU_NEED_Q(h);
    const size_t bytes = (size_t)h->N * (size_t)h->S * 4 * sizeof(uint32_t);
    if (!h->d_explore_n || h->explore_S != h->S) {
        GU_HIP(hipStreamSynchronize(h->stream));
        gu_explore_free(h);
        GU_TRY(gu_tabular_fits(h, bytes, "visit counts"));
        GU_HIP(hipMalloc(&h->d_explore_n, bytes));
        h->explore_S = h->S;
    }
    GU_HIP(hipMemsetAsync(h->d_explore_n, 0, bytes, h->stream));
    GU_HIP(hipStreamSynchronize(h->stream));
    return GU_OK;
}

int gu_explore_set_tables(gu_handle h, int32_t C, const double *U, const double *B)
{
    GU_ENTER(h);
    const double *v[] = {U, B};
    return gu_schedule_upload(h, h->d_explore_tab, h->explore_C, C, v, 2);
}

int gu_explore_run(gu_handle h, int64_t T, int32_t mode, double alpha, double gamma, uint32_t eps_q16, uint32_t flags)
{
    GU_ENTER(h);
    GU_NO_OVERLAY(h, "gu_explore_run");
    GU_NEED_GRID(h);
    GU_NEED_Q(h);
    GU_NEED_COUNTS(h);
    GU_REQUIRE(GU_HAS_EXPLORE_TABLES(h), GU_ERR_STATE, "no exploration tables: call gu_explore_set_tables first");
    GU_REQUIRE(mode == 0 || mode == 1, GU_ERR_INVALID, "mode %d: 0 = UCB, 1 = Thompson", mode);
    int rc = gu_tabular_check(h, "gu_explore_run", T, -1, eps_q16, alpha, gamma, flags);
    if (rc != GU_OK || T == 0) return rc;
    return gu_launch_explore(h, T, mode, alpha, gamma, eps_q16, flags);
}

static int gu_explore_range(gu_engine *h, int64_t env0, int64_t n, const void *counts)
{
    GU_NEED_GRID(h);
    GU_NEED_COUNTS(h);
    GU_REQUIRE(counts != nullptr, GU_ERR_INVALID, "counts is NULL");
    return gu_env_range(h, env0, n);
}

int gu_explore_get_counts(gu_handle h, int64_t env0, int64_t n, uint32_t *counts)
{
    GU_ENTER(h);
    GU_TRY(gu_explore_range(h, env0, n, counts));
    return gu_env_copy(h, hipMemcpyDeviceToHost, counts, h->d_explore_n, env0, n, (size_t)h->S * 4);
}

int gu_explore_set_counts(gu_handle h, int64_t env0, int64_t n, const uint32_t *counts)
{
    GU_ENTER(h);
    GU_TRY(gu_explore_range(h, env0, n, counts));
    const size_t row = (size_t)h->S * 4, k = (size_t)n * row;
    for (size_t i = 0; i < k; ++i)
        GU_REQUIRE(counts[i] <= GU_EXPLORE_COUNT_MAX, GU_ERR_INVALID, "count %u of env %lld above the cap 0x%X", counts[i],
                   (long long)(env0 + (int64_t)(i / row)), GU_EXPLORE_COUNT_MAX);
    return gu_env_copy(h, hipMemcpyHostToDevice, counts, h->d_explore_n, env0, n, row);
}

}  // extern "C"
