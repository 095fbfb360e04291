// gu_fa.hip -- batched episodic semi-gradient SARSA and semi-gradient Q-learning over K active binary features per state for
// gfx950 (Sutton & Barto 10.1; include/gu.h: gu_fa_run; restated on the CPU by tests/_fa_oracle.py).  Learner e owns env e and a
// weight table w_e[F][4]; the action values are computed, not stored: Q_e(s) = the sum of the K rows w_e[phi[s][k]], folded in
// column order.  The lane, its RNG word, the move, the trajectory rows and the statistics are gu_tabular.hpp's (TabLane without
// its Q-row loads); what is here is the feature table, the K-row gather, the update of K entries and its forwarding.
//
// Weights: learner-major [N][F][4], so a lane's K rows are K independent aligned 32-byte pieces (two 16-byte loads each) issued
// together behind the one read of phi[s'].
// phi: [S][K], shared by all envs.  The LDS kernels keep a uint16 copy behind the cell planes when F <= 65536 and planes + copy
// fit 64 KiB (8 KiB for 32x32 cells, K = 4); otherwise -- and in the L2 kernels -- the lane reads the int32 table through L2.
// Per step the lane holds, in VGPRs, the K rows of the state it stands in, their K feature indices and the folded sum.  After the
// move it sets the K entries it is about to update aside and turns the rows of s into those of s' in place: slot k is gathered
// only where phi[s'][k] != phi[s][k] (columns are slots: gu_fa_init refuses a table that has one index in two columns, so K compares
// suffice; neighbouring cells share most of their tiles, a wall bump shares all, and nothing is read behind a terminal s').  It folds
// the rows (pre-update: the bootstrap), writes the K updated entries, puts the new entry into every row it kept and folds the
// patched rows again in rule order: Q + c * g is another double.
// K is a compile-time parameter, every K in 1 .. GU_FA_MAX_K has its own instantiation: a padded slot would add + 0.0, which turns
// -0.0 into +0.0.
#include "gu_tabular.hpp"

#include <algorithm>

struct FaArgs : TabArgs {
    double *w;              // [N][F][4]
    const int32_t *phi;     // [S][K]
    const uint16_t *phi16;  // [S][K] as uint16, padded to whole 16 bytes (nullptr: F > 65536)
    int32_t F;
    int32_t phi_lds;        // bytes of phi16 the LDS kernels stage behind the planes (0: read phi through L2)
    int8_t *next_a;         // [N] SARSA: the action carried to the next launch (-1: none)
    int32_t carry;          // 1: this launch directly follows a SARSA gu_fa_run on this engine -- start with next_a
};

// the K feature indices of state s
template <int K, bool LDS>
__device__ __forceinline__ void gu_fa_phi(const FaArgs &a, const uint8_t *lphi, int32_t s, uint32_t (&f)[K])
{
    if (LDS && a.phi_lds) {
        const uint16_t *p = reinterpret_cast<const uint16_t *>(lphi) + s * K;
        if (K % 4 == 0) {
#pragma unroll
            for (int j = 0; j < K / 4; ++j) {
                const uint2 v = reinterpret_cast<const uint2 *>(p)[j];
                f[4 * j] = v.x & 0xFFFFu, f[4 * j + 1] = v.x >> 16, f[4 * j + 2] = v.y & 0xFFFFu, f[4 * j + 3] = v.y >> 16;
            }
        } else if (K % 2 == 0) {
#pragma unroll
            for (int j = 0; j < K / 2; ++j) {
                const uint32_t v = reinterpret_cast<const uint32_t *>(p)[j];
                f[2 * j] = v & 0xFFFFu, f[2 * j + 1] = v >> 16;
            }
        } else {
#pragma unroll
            for (int k = 0; k < K; ++k) f[k] = p[k];
        }
    } else {
        const int32_t *p = a.phi + (int64_t)s * K;
        if (K % 4 == 0) {
#pragma unroll
            for (int j = 0; j < K / 4; ++j) {
                const int4 v = reinterpret_cast<const int4 *>(p)[j];
                f[4 * j] = (uint32_t)v.x, f[4 * j + 1] = (uint32_t)v.y, f[4 * j + 2] = (uint32_t)v.z, f[4 * j + 3] = (uint32_t)v.w;
            }
        } else if (K % 2 == 0) {
#pragma unroll
            for (int j = 0; j < K / 2; ++j) {
                const int2 v = reinterpret_cast<const int2 *>(p)[j];
                f[2 * j] = (uint32_t)v.x, f[2 * j + 1] = (uint32_t)v.y;
            }
        } else {
#pragma unroll
            for (int k = 0; k < K; ++k) f[k] = (uint32_t)p[k];
        }
    }
}

template <int K>
__device__ __forceinline__ void gu_fa_gather(const double *we, const uint32_t (&f)[K], QRow (&r)[K])
{
#pragma unroll
    for (int k = 0; k < K; ++k) r[k] = gu_q_load(we + (int64_t)f[k] * 4);
}

// Q(s) from its K rows: row 0, then + row k for k = 1 .. K-1, one rounded add each
template <int K>
__device__ __forceinline__ QRow gu_fa_fold(const QRow (&r)[K])
{
    QRow q = r[0];
#pragma unroll
    for (int k = 1; k < K; ++k) {
        q.v0 = __dadd_rn(q.v0, r[k].v0);
        q.v1 = __dadd_rn(q.v1, r[k].v1);
        q.v2 = __dadd_rn(q.v2, r[k].v2);
        q.v3 = __dadd_rn(q.v3, r[k].v3);
    }
    return q;
}

template <int K, bool SARSA, bool LDS>
__global__ void __launch_bounds__(GU_BLOCK) gu_fa_kernel(const FaArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const uint8_t *lphi = smem + 2 * a.cell_bytes;
    if (LDS && a.phi_lds)  // (the barrier behind the planes, in TabLane's constructor, covers these stores too)
        for (int32_t i = threadIdx.x * 16; i < a.phi_lds; i += blockDim.x * 16)
            *reinterpret_cast<uint4 *>(smem + 2 * a.cell_bytes + i) = *reinterpret_cast<const uint4 *>(reinterpret_cast<const uint8_t *>(a.phi16) + i);
    TabLane<LDS, false> L(a, smem);
    if (L.e < a.N) {
        L.begin(a);
        double *we = a.w + L.e * (int64_t)a.F * 4;
        uint32_t f[K];  // phi[s]
        QRow w[K];      // the rows w_e[phi[s][k]]; L.q is their fold
#pragma unroll
        for (int k = 0; k < K; ++k) f[k] = 0u, w[k] = QRow{0.0, 0.0, 0.0, 0.0};
        if (!L.d) {
            gu_fa_phi<K, LDS>(a, lphi, L.s, f);
            gu_fa_gather<K>(we, f, w);
            L.q = gu_fa_fold<K>(w);
        }
        int32_t act = (SARSA && a.carry) ? (int32_t)a.next_a[L.e] : -1;
        for (int32_t i = 0; i < a.T; ++i) {
            if (L.d) {  // a reset drops the carried action
                act = -1;
                L.reset(a);
                gu_fa_phi<K, LDS>(a, lphi, L.s, f);
                gu_fa_gather<K>(we, f, w);
                L.q = gu_fa_fold<K>(w);
            }
            if (act < 0) act = (int32_t)gu_q_action(L.q, L.word(), a.eps_q16);
            const uint32_t ua = (uint32_t)act;
            const int32_t s2 = L.move(a, ua);
            // the entries of this step's update, then the rows of s' in place of those of s: slot k keeps its row where
            // phi[s'][k] == phi[s][k] (every slot on a wall bump; nothing is read behind a terminal s')
            double wa[K];
            uint32_t f2[K];
#pragma unroll
            for (int k = 0; k < K; ++k) wa[k] = gu_q_get(w[k], ua), f2[k] = f[k];
            QRow n = L.q;
            if (!L.d && s2 != L.s) {
                gu_fa_phi<K, LDS>(a, lphi, s2, f2);
#pragma unroll
                for (int k = 0; k < K; ++k)
                    if (f2[k] != f[k]) w[k] = gu_q_load(we + (int64_t)f2[k] * 4);
                n = gu_fa_fold<K>(w);  // Q(s') before the update: the bootstrap
            }
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
            const double g = __dmul_rn(a.alpha, __dsub_rn(target, gu_q_get(L.q, ua)));
            // the K entries; a kept row takes the new one, and Q(s') is folded again from the patched rows
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const double nv = __dadd_rn(wa[k], g);
                we[(int64_t)f[k] * 4 + ua] = nv;
                if (f2[k] == f[k]) gu_q_put(w[k], ua, nv);
                f[k] = f2[k];
            }
            n = gu_fa_fold<K>(w);
            act = a2;
            L.step(a, i, s2, n);
        }
        L.end(a);
        if (SARSA) a.next_a[L.e] = (int8_t)act;
    }
    L.ballot(a);
}

__global__ void __launch_bounds__(256) gu_fa_fill_kernel(double *__restrict__ w, size_t n, double v)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) w[i] = v;
}

static int gu_fa_fill(gu_engine *h, double w0)
{
    const size_t n = (size_t)h->N * (size_t)h->fa_F * 4;
    const unsigned blocks = (unsigned)std::max<size_t>(1, std::min<size_t>((n + 255) / 256, (size_t)h->n_cu * 16));
    hipLaunchKernelGGL(gu_fa_fill_kernel, dim3(blocks), dim3(256), 0, h->stream, h->d_fa_w, n, w0);
    GU_HIP(hipGetLastError());
    return GU_OK;
}

// q[i][s][.] = Q_{env0+i}(s), folded by the rule: one thread per (env, s) row
__global__ void __launch_bounds__(256) gu_fa_q_kernel(const double *__restrict__ w, const int32_t *__restrict__ phi, double *__restrict__ q,
                                                      int64_t rows, int32_t S, int32_t K, int32_t F)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows) return;
    const int64_t e = i / S;
    const int32_t s = (int32_t)(i - e * S);
    const double *we = w + e * (int64_t)F * 4;
    const int32_t *p = phi + (int64_t)s * K;
    QRow r = gu_q_load(we + (int64_t)p[0] * 4);
    for (int32_t k = 1; k < K; ++k) {
        const QRow x = gu_q_load(we + (int64_t)p[k] * 4);
        r.v0 = __dadd_rn(r.v0, x.v0);
        r.v1 = __dadd_rn(r.v1, x.v1);
        r.v2 = __dadd_rn(r.v2, x.v2);
        r.v3 = __dadd_rn(r.v3, x.v3);
    }
    double2 *out = reinterpret_cast<double2 *>(q + i * 4);
    out[0] = make_double2(r.v0, r.v1);
    out[1] = make_double2(r.v2, r.v3);
}

// the folded tables of envs env0 .. env0+n-1 into d_out [n][S][4] (async)
static int gu_fa_fold_q(gu_engine *h, int64_t env0, int64_t n, double *d_out)
{
    const int64_t rows = n * (int64_t)h->S;
    if (rows == 0) return GU_OK;
    hipLaunchKernelGGL(gu_fa_q_kernel, dim3(gu_blocks(rows, 256)), dim3(256), 0, h->stream, h->d_fa_w + (size_t)env0 * (size_t)h->fa_F * 4,
                       h->d_fa_phi, d_out, rows, h->S, h->fa_K, h->fa_F);
    GU_HIP(hipGetLastError());
    return GU_OK;
}

template <int K, bool SARSA>
static int gu_fa_launch(gu_engine *h, FaArgs &a)
{
    const int lds_bs = gu_lds_block(h, GU_BLOCK, 2);
    if (lds_bs) {
        const size_t planes = 2 * (size_t)h->cell_bytes;
        a.phi_lds = (h->d_fa_phi16 && planes + h->fa_phi16_bytes <= 64 * 1024) ? (int32_t)h->fa_phi16_bytes : 0;
        hipLaunchKernelGGL((gu_fa_kernel<K, SARSA, true>), dim3(gu_blocks(h->N, lds_bs)), dim3(lds_bs), planes + (size_t)a.phi_lds, h->stream, a);
    } else {
        a.phi_lds = 0;
        hipLaunchKernelGGL((gu_fa_kernel<K, SARSA, false>), dim3(gu_blocks(h->N, GU_BLOCK)), dim3(GU_BLOCK), 0, h->stream, a);
    }
    GU_HIP(hipGetLastError());
    return GU_OK;
}

template <int K>
static int gu_fa_launch_k(gu_engine *h, FaArgs &a, int32_t method)
{
    return method == 1 ? gu_fa_launch<K, true>(h, a) : gu_fa_launch<K, false>(h, a);
}

static int gu_launch_fa(gu_engine *h, int64_t T, int32_t method, double alpha, double gamma, uint32_t eps_q16, uint32_t flags)
{
    FaArgs a{};
    gu_tabular_args(h, a, T, alpha, gamma, eps_q16, flags);
    a.q = nullptr;
    a.w = h->d_fa_w;
    a.phi = h->d_fa_phi;
    a.phi16 = h->d_fa_phi16;
    a.F = h->fa_F;
    a.next_a = h->d_fa_next;
    a.carry = (method == 1 && gu_carry_is(h, GU_CARRY_FA_SARSA, 0)) ? 1 : 0;
    int rc = GU_ERR_INVALID;
    switch (h->fa_K) {
    case 1: rc = gu_fa_launch_k<1>(h, a, method); break;
    case 2: rc = gu_fa_launch_k<2>(h, a, method); break;
    case 3: rc = gu_fa_launch_k<3>(h, a, method); break;
    case 4: rc = gu_fa_launch_k<4>(h, a, method); break;
    case 5: rc = gu_fa_launch_k<5>(h, a, method); break;
    case 6: rc = gu_fa_launch_k<6>(h, a, method); break;
    case 7: rc = gu_fa_launch_k<7>(h, a, method); break;
    case 8: rc = gu_fa_launch_k<8>(h, a, method); break;
    }
    return rc != GU_OK ? rc : gu_tabular_after(h, T, flags, method == 1 ? GuCarry{GU_CARRY_FA_SARSA, 0} : GuCarry{});
}

void gu_fa_free(gu_engine *h)
{
    gu_release(h->d_fa_w, h->d_fa_phi, h->d_fa_phi16, h->d_fa_next);
    h->fa_phi16_bytes = 0;
    h->fa_S = h->fa_K = h->fa_F = 0;
    gu_carry_release(h, GU_CARRY_FA_SARSA);
}

#define GU_NEED_FA(h) GU_REQUIRE(GU_HAS_FA(h), GU_ERR_STATE, "no features: call gu_fa_init first")

extern "C" {

int gu_fa_init(gu_handle h, int32_t K, int32_t F, const int32_t *phi, double w0)
{
    GU_ENTER(h);
    GU_NEED_GRID(h);
    GU_REQUIRE(K >= 1 && K <= GU_FA_MAX_K, GU_ERR_INVALID, "K %d out of range (1 .. %d)", K, GU_FA_MAX_K);
    GU_REQUIRE(F >= 1 && F <= GU_FA_MAX_F, GU_ERR_INVALID, "F %d out of range (1 .. %d)", F, GU_FA_MAX_F);
    GU_REQUIRE(phi != nullptr, GU_ERR_INVALID, "phi is NULL");
    GU_REQUIRE(std::isfinite(w0), GU_ERR_INVALID, "w0 must be finite");
    const size_t S = (size_t)h->S, cells = S * (size_t)K;
    std::vector<int8_t> column((size_t)F, (int8_t)-1);  // the column each feature index occurs in
    for (size_t i = 0; i < cells; ++i) {
        const int32_t f = phi[i], k = (int32_t)(i % (size_t)K);
        GU_REQUIRE(f >= 0 && f < F, GU_ERR_INVALID, "phi[%zu][%d] = %d outside 0 .. %d", i / (size_t)K, k, f, F - 1);
        GU_REQUIRE(column[f] < 0 || column[f] == k, GU_ERR_INVALID, "feature %d occurs in columns %d and %d: a column is a slot of its own", f,
                   (int)column[f], k);
        column[f] = (int8_t)k;
    }
    gu_tabular_drop_carry(h);
    GU_HIP(hipStreamSynchronize(h->stream));
    if (!h->d_fa_w || h->fa_S != h->S || h->fa_K != K || h->fa_F != F) {
        gu_fa_free(h);
        const size_t bytes = (size_t)h->N * (size_t)F * 4 * sizeof(double);
        GU_TRY(gu_tabular_fits(h, bytes + cells * 6 + (size_t)h->N, "feature weights"));
        GU_HIP(hipMalloc(&h->d_fa_w, bytes));
        GU_HIP(hipMalloc(&h->d_fa_phi, cells * sizeof(int32_t)));
        GU_HIP(hipMalloc(&h->d_fa_next, (size_t)h->N));
        if (F <= 65536) {
            h->fa_phi16_bytes = (cells * sizeof(uint16_t) + 15) & ~(size_t)15;
            GU_HIP(hipMalloc(&h->d_fa_phi16, h->fa_phi16_bytes));
        }
        h->fa_S = h->S;
        h->fa_K = K;
        h->fa_F = F;
    }
    GU_HIP(hipMemcpy(h->d_fa_phi, phi, cells * sizeof(int32_t), hipMemcpyHostToDevice));
    if (h->d_fa_phi16) {
        std::vector<uint16_t> p16(h->fa_phi16_bytes / sizeof(uint16_t), (uint16_t)0);
        for (size_t i = 0; i < cells; ++i) p16[i] = (uint16_t)phi[i];
        GU_HIP(hipMemcpy(h->d_fa_phi16, p16.data(), h->fa_phi16_bytes, hipMemcpyHostToDevice));
    }
    GU_HIP(hipMemsetAsync(h->d_fa_next, 0xFF, (size_t)h->N, h->stream));
    GU_TRY(gu_fa_fill(h, w0));  // every weight = w0 (async)
    GU_HIP(hipStreamSynchronize(h->stream));
    return GU_OK;
}

int gu_fa_run(gu_handle h, int64_t T, int32_t method, double alpha, double gamma, uint32_t eps_q16, uint32_t flags)
{
    GU_ENTER(h);
    GU_NO_OVERLAY(h, "gu_fa_run");
    GU_NEED_GRID(h);
    GU_NEED_FA(h);
    GU_REQUIRE(method == 0 || method == 1, GU_ERR_INVALID, "method %d: 0 = Q-learning, 1 = SARSA", method);
    int rc = gu_tabular_check(h, "gu_fa_run", T, -1, eps_q16, alpha, gamma, flags);
    if (rc != GU_OK || T == 0) return rc;
    return gu_launch_fa(h, T, method, alpha, gamma, eps_q16, flags);
}

static int gu_fa_range(gu_engine *h, int64_t env0, int64_t n, const void *p, const char *name)
{
    GU_NEED_GRID(h);
    GU_NEED_FA(h);
    GU_REQUIRE(p != nullptr, GU_ERR_INVALID, "%s is NULL", name);
    return gu_env_range(h, env0, n);
}

int gu_fa_get_w(gu_handle h, int64_t env0, int64_t n, double *w)
{
    GU_ENTER(h);
    GU_TRY(gu_fa_range(h, env0, n, w, "w"));
    return gu_env_copy(h, hipMemcpyDeviceToHost, w, h->d_fa_w, env0, n, (size_t)h->fa_F * 4);
}

int gu_fa_set_w(gu_handle h, int64_t env0, int64_t n, const double *w)
{
    GU_ENTER(h);
    GU_TRY(gu_fa_range(h, env0, n, w, "w"));
    gu_tabular_drop_carry(h);
    return gu_env_copy(h, hipMemcpyHostToDevice, w, h->d_fa_w, env0, n, (size_t)h->fa_F * 4);
}

int gu_fa_get_q(gu_handle h, int64_t env0, int64_t n, double *q)
{
    GU_ENTER(h);
    int rc = gu_fa_range(h, env0, n, q, "q");
    if (rc != GU_OK || n == 0) return rc;
    // folded on the device in slices of at most 64 MiB, through the engine's scratch buffer
    const size_t row = (size_t)h->S * 4 * sizeof(double);
    const int64_t slice = std::max<int64_t>(1, (int64_t)(((size_t)64 << 20) / row));
    for (int64_t i = 0; i < n; i += slice) {
        const int64_t k = std::min<int64_t>(slice, n - i);
        GU_TRY(gu_ensure_scratch(h, (size_t)k * row));
        GU_TRY(gu_fa_fold_q(h, env0 + i, k, reinterpret_cast<double *>(h->d_scratch)));
        GU_HIP(hipStreamSynchronize(h->stream));
        GU_HIP(hipMemcpy(q + (size_t)i * (size_t)h->S * 4, h->d_scratch, (size_t)k * row, hipMemcpyDeviceToHost));
    }
    return GU_OK;
}

}  // extern "C"
