// gu_sweep.hip -- batched tabular prioritized sweeping for gfx950 (Sutton & Barto 8.4; include/gu.h: gu_sweep_run; restated on the
// CPU by tests/_sweep_oracle.py): learner e owns env e, its gu_td_* table, the Dyna-Q model that gu_dyna.hip fills (the same buffers)
// and a priority queue of observed pairs.  The real step learns nothing by itself: it records its outcome in the model and queues its
// pair under the size of its TD error; up to P planning updates per real step then take the pair with the largest key from the queue,
// update it from the model and queue its predecessors.
//
// The queue of a lane is a binary max-heap of 64-bit keys in HBM, the first per-lane state here that is a mutable ordered structure:
//   heap [N][4S+2] uint64   slots 1 .. size hold the keys (1-based: the children 2i, 2i+1 of slot i are one aligned 16-byte piece, so
//                           a level of the sift-down is one load); slot 0 holds two counters for tools/sweep_rate.py (low half: pops,
//                           high half: inserts that changed the queue, both modulo 2^32 since gu_sweep_init); slot 4S+1 pads the piece
//   pos  [N][4S]   int32    the slot of pair p, -1 while it is not queued
//   size [N]       int32
// A key is the priority's float64 pattern with its low 16 bits replaced by the pair index (include/gu.h), so keys are distinct, their
// order is total and what a pop returns does not depend on the heap's shape -- which is why the CPU restatement can be a dense array
// with an argmax.  A queued pair's key only grows (insert keeps the larger one), so an insert is a sift-up from pos[p] (or from a new
// last slot) and only the pop sifts down.  Both sifts move a hole, one store of a key and one of its pos per level, at most 16 levels
// (4S <= 65 536).
// Divergence: the lanes of a wave pop different pairs and sift to different depths.  The planning loop and both sift loops run while
// ANY lane of the wave still works (a ballot, as gu_dyna_pick's), with the finished lanes masked, so their conditions are scalar.
// Ordering: as in gu_dyna.hip, one lane's vector memory operations to one address complete in order -- a Q load issued after the
// store of an updated entry sees it, and so does a load of a heap slot or a pos entry after this lane's store to it.  No other lane
// touches a lane's table, model or queue.
// The row of the state the lane stands in stays in VGPRs; a planning update of an entry of that row forwards the value into it, so
// the next real step chooses its action from the table after planning.
#include "gu_tabular.hpp"

#include <algorithm>

#define GU_SWEEP_MAX_PAIRS 65536  // the pair index has 16 bits of the key

struct SweepArgs : TabArgs {
    int32_t P;
    uint64_t *model;  // [N][S*4]   (gu_dyna.hip)
    int32_t *list;    // [N][S*4]
    int32_t *count;   // [N]
    uint8_t *seen;    // [N][S]
    int32_t exact;    // 1: the seen bits decide what is observed; 0: compare every model word
    double theta;
    uint64_t *heap;  // [N][S*4+2]
    int32_t *hpos;   // [N][S*4]
    int32_t *size;   // [N]
};

typedef uint64_t gu_u64x2 __attribute__((ext_vector_type(2)));

// one lane's queue
struct SweepQueue {
    uint64_t *__restrict__ heap;  // the lane's row: slots 1 .. size
    int32_t *__restrict__ pos;
    int32_t size;
    uint32_t pops, inserts;

    // insert(p, x) of include/gu.h on the lanes with `on`: nothing unless x > theta and the truncated pattern is not zero; a pair that is
    // queued keeps the larger key.  Every lane of the wave that is in the caller's branch must call it (the loop condition is a ballot).
    __device__ __forceinline__ void insert(bool on, int32_t p, double x, double theta)
    {
        const uint64_t bits = (uint64_t)__double_as_longlong(x) >> 16;
        const uint64_t key = (bits << 16) | (uint64_t)(uint32_t)p;
        bool act = on && x > theta && bits != 0ull;  // (a NaN x fails x > theta)
        int32_t i = 0;
        if (act) {
            i = pos[p];
            if (i < 0)
                i = ++size;  // a new pair: the hole opens behind the last slot
            else
                act = heap[i] < key;  // its slot becomes the hole if the key grows
            inserts += act ? 1u : 0u;
        }
        bool up = act;
        while (__builtin_amdgcn_ballot_w64(up) != 0ull) {
            if (up) {
                const int32_t j = i >> 1;
                const uint64_t pk = j >= 1 ? heap[j] : ~0ull;
                if (pk < key) {  // the parent comes down into the hole
                    heap[i] = pk;
                    pos[pk & 0xFFFFull] = i;
                    i = j;
                } else {
                    up = false;
                }
            }
        }
        if (act) {
            heap[i] = key;
            pos[p] = i;
        }
    }

    // remove the pair with the largest key on the lanes with `on` (their queues are not empty); -1 on the others
    __device__ __forceinline__ int32_t pop(bool on)
    {
        int32_t p = -1, i = 1;
        uint64_t last = 0ull;
        bool down = false;
        if (on) {
            p = (int32_t)(heap[1] & 0xFFFFull);
            pos[p] = -1;
            last = heap[size];
            --size;
            ++pops;
            down = size > 0;  // the last key looks for its place from the root down
        }
        while (__builtin_amdgcn_ballot_w64(down) != 0ull) {
            if (down) {
                const int32_t c = 2 * i;
                if (c > size) {
                    down = false;
                } else {
                    const gu_u64x2 ch = *reinterpret_cast<const gu_u64x2 *>(heap + c);  // (slot size + 1 <= 4S + 1 is storage, its content stale)
                    const uint64_t k0 = ch.x, k1 = c < size ? ch.y : 0ull;
                    const bool right = k1 > k0;
                    const uint64_t km = right ? k1 : k0;
                    if (km > last) {  // the larger child comes up into the hole
                        heap[i] = km;
                        pos[km & 0xFFFFull] = i;
                        i = c + (right ? 1 : 0);
                    } else {
                        down = false;
                    }
                }
            }
        }
        if (on && size > 0) {
            heap[i] = last;
            pos[last & 0xFFFFull] = i;
        }
        return p;
    }
};

template <bool LDS>
__global__ void __launch_bounds__(GU_BLOCK) gu_sweep_kernel(const SweepArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    TabLane<LDS> L(a, smem);
    if (L.e < a.N) {
        L.begin(a);
        const int64_t e = L.e, SA = (int64_t)a.S * 4;
        double *qe = L.qe;
        uint64_t *__restrict__ me = a.model + e * SA;
        int32_t *__restrict__ le = a.list + e * SA;
        uint8_t *__restrict__ se = a.seen + e * (int64_t)a.S;
        uint32_t count = (uint32_t)a.count[e];
        SweepQueue Q;
        Q.heap = a.heap + e * (SA + 2);
        Q.pos = a.hpos + e * SA;
        Q.size = a.size[e];
        const uint64_t counters = Q.heap[0];
        Q.pops = (uint32_t)counters;
        Q.inserts = (uint32_t)(counters >> 32);
        for (int32_t i = 0; i < a.T; ++i) {
            // the real step: gu_td_kernel's choice and move, no update of Q[s][a]
            L.reset(a);
            const int32_t s = L.s;
            const uint32_t ua = gu_q_action(L.q, L.word(), a.eps_q16);
            const int32_t sa = s * 4 + (int32_t)ua;
            const int32_t s2 = L.move(a, ua);
            QRow n = L.next_row(s2);
            const uint32_t bits = a.exact ? (uint32_t)se[s] : 0u;
            const uint64_t seen = a.exact ? 0ull : me[sa];
            const double target = L.d ? (double)L.r : __dadd_rn((double)L.r, __dmul_rn(a.gamma, gu_q_max(n)));
            const double x = fabs(__dsub_rn(target, gu_q_get(L.q, ua)));
            // the model, as gu_dyna_kernel keeps it
            const uint64_t word = gu_dyna_pack(s2, L.r, L.d);
            if (a.exact) {
                if (!((bits >> ua) & 1u)) {
                    me[sa] = word;
                    le[count++] = sa;
                    se[s] = (uint8_t)(bits | (1u << ua));
                }
            } else {
                if (seen != word) me[sa] = word;
                if (seen == GU_DYNA_UNSEEN) le[count++] = sa;
            }
            Q.insert(true, sa, x, a.theta);
            // planning: up to P pops, while any lane of the wave has a pair queued
            for (int32_t j = 0; j < a.P && __builtin_amdgcn_ballot_w64(Q.size > 0) != 0ull; ++j) {
                const bool on = Q.size > 0;
                // The pair at the root is all the update needs: its model word, the row of S and the row of S' go out before the pop
                // sifts, and land while it does.  (The sift touches heap and pos only; Q changes behind it.)
                const int32_t p = on ? (int32_t)(Q.heap[1] & 0xFFFFull) : 0;
                const int32_t S = p >> 2;
                const uint32_t A = (uint32_t)p & 3u;
                uint64_t w = GU_DYNA_UNSEEN;
                QRow rs = QRow{0.0, 0.0, 0.0, 0.0}, r2 = rs;
                if (on) {
                    w = me[p];
                    rs = gu_q_load(qe + (int64_t)S * 4);
                }
                const uint32_t hi = (uint32_t)(w >> 32);
                const int32_t S2 = (int32_t)(hi & 0x7FFFFFFFu), R = (int32_t)(uint32_t)w;
                const bool D = (hi >> 31) != 0u;
                if (on && !D && S2 != S) r2 = gu_q_load(qe + (int64_t)S2 * 4);
                // ... and so do the seen bytes of the five candidate cells (see below)
                uint32_t cand = 0u;
#pragma unroll
                for (int32_t k = 0; k < 5; ++k) {
                    const int32_t c = S + (k == 0 ? 0 : k == 1 ? -a.W : k == 2 ? 1 : k == 3 ? a.W : -1);
                    const bool in = on && c >= 0 && c < a.S;
                    uint32_t sb = in ? 0xFu : 0u;
                    if (a.exact && in) sb = (uint32_t)se[c] & 0xFu;
                    cand |= sb << (4 * k);
                }
                Q.pop(on);
                double mS = 0.0;
                if (on) {
                    double qp = gu_q_get(rs, A);
                    const double mx = D ? 0.0 : gu_q_max(S2 == S ? rs : r2);
                    const double tgt = D ? (double)R : __dadd_rn((double)R, __dmul_rn(a.gamma, mx));
                    qp = __dadd_rn(qp, __dmul_rn(a.alpha, __dsub_rn(tgt, qp)));
                    qe[p] = qp;
                    gu_q_put(rs, A, qp);
                    if (S == s2) gu_q_put(n, A, qp);  // keep the row in VGPRs current
                    mS = gu_q_max(rs);
                }
                // the candidate predecessors of S: the observed pairs of S and its four neighbours by index whose model entry leads to S.
                // The five bytes of seen bits went out together, ahead of the pop (compare mode: every pair of a cell inside the grid is
                // a candidate); now per cell with a candidate its four model words and its Q row, 32 aligned bytes each, in one round
                // trip, then the inserts.
                for (int32_t k = 0; k < 5; ++k) {
                    const uint32_t sb = (cand >> (4 * k)) & 0xFu;
                    if (__builtin_amdgcn_ballot_w64(sb != 0u) == 0ull) continue;
                    const int32_t c = S + (k == 0 ? 0 : k == 1 ? -a.W : k == 2 ? 1 : k == 3 ? a.W : -1);
                    gu_u64x2 wlo = {GU_DYNA_UNSEEN, GU_DYNA_UNSEEN}, whi = wlo;
                    QRow qc = QRow{0.0, 0.0, 0.0, 0.0};
                    if (sb != 0u) {
                        const gu_u64x2 *mc = reinterpret_cast<const gu_u64x2 *>(me + (int64_t)c * 4);
                        wlo = mc[0];
                        whi = mc[1];
                        qc = gu_q_load(qe + (int64_t)c * 4);  // (behind the store of Q[S][A]: the row of c == S is the updated one)
                    }
                    for (uint32_t b = 0; b < 4u; ++b) {
                        const uint64_t wb = b == 0u ? wlo.x : b == 1u ? wlo.y : b == 2u ? whi.x : whi.y;
                        const uint32_t hb = (uint32_t)(wb >> 32);
                        // (an unobserved word reads as s' = 2^31 - 1: never a state)
                        const bool hit = ((sb >> b) & 1u) != 0u && (hb & 0x7FFFFFFFu) == (uint32_t)S;
                        const int32_t Rb = (int32_t)(uint32_t)wb;
                        const double tb = (hb >> 31) ? (double)Rb : __dadd_rn((double)Rb, __dmul_rn(a.gamma, mS));
                        Q.insert(hit, c * 4 + (int32_t)b, fabs(__dsub_rn(tb, gu_q_get(qc, b))), a.theta);
                    }
                }
            }
            L.step(a, i, s2, n);
        }
        a.count[e] = (int32_t)count;
        a.size[e] = Q.size;
        Q.heap[0] = (uint64_t)Q.pops | ((uint64_t)Q.inserts << 32);
        L.end(a);
    }
    L.ballot(a);
}

static int gu_launch_sweep(gu_engine *h, int64_t T, int32_t P, double theta, double alpha, double gamma, uint32_t eps_q16, uint32_t flags)
{
    SweepArgs a{};
    gu_tabular_args(h, a, T, alpha, gamma, eps_q16, flags);
    a.P = P;
    a.model = h->d_dyna_model;
    a.list = h->d_dyna_list;
    a.count = h->d_dyna_count;
    a.seen = h->d_dyna_seen;
    a.exact = h->dyna_exact ? 1 : 0;
    a.theta = theta;
    a.heap = h->d_sweep_heap;
    a.hpos = h->d_sweep_pos;
    a.size = h->d_sweep_size;
    const int rc = gu_tabular_launch(h, gu_sweep_kernel<true>, gu_sweep_kernel<false>, a);
    return rc != GU_OK ? rc : gu_tabular_after(h, T, flags);
}

// (the queue lives and dies with the model: gu_dyna_free releases both, gu_dyna_init clears both)
#define GU_NEED_SWEEP(h) \
    GU_REQUIRE(GU_HAS_SWEEP(h), GU_ERR_STATE, "no priority queue: call gu_sweep_init first")

// empty queues, counters at zero (queued on the engine's stream; nothing to do without a queue)
int gu_sweep_clear(gu_engine *h)
{
    if (!h->d_sweep_heap) return GU_OK;
    const size_t pairs = (size_t)h->N * (size_t)h->dyna_S * 4;
    GU_HIP(hipMemsetAsync(h->d_sweep_heap, 0, (pairs + 2 * (size_t)h->N) * sizeof(uint64_t), h->stream));
    GU_HIP(hipMemsetAsync(h->d_sweep_pos, 0xFF, pairs * sizeof(int32_t), h->stream));
    GU_HIP(hipMemsetAsync(h->d_sweep_size, 0, (size_t)h->N * sizeof(int32_t), h->stream));
    return GU_OK;
}

// the raw rows of envs env0 .. env0+n-1 on the host
static int gu_sweep_rows(gu_engine *h, int64_t env0, int64_t n, uint64_t *heap, int32_t *pos, int32_t *size)
{
    const size_t pairs = (size_t)h->S * 4;
    GU_HIP(hipStreamSynchronize(h->stream));
    GU_TRY(gu_env_copy(h, hipMemcpyDeviceToHost, heap, h->d_sweep_heap, env0, n, pairs + 2, false));
    GU_TRY(gu_env_copy(h, hipMemcpyDeviceToHost, pos, h->d_sweep_pos, env0, n, pairs, false));
    return gu_env_copy(h, hipMemcpyDeviceToHost, size, h->d_sweep_size, env0, n, 1, false);
}

extern "C" {

int gu_sweep_init(gu_handle h)
{
    GU_ENTER(h);
    GU_NEED_GRID(h);
    GU_REQUIRE((int64_t)h->S * 4 <= GU_SWEEP_MAX_PAIRS, GU_ERR_INVALID, "%d states: the queue's keys hold pair indices below %d (at most %d states)", h->S,
               GU_SWEEP_MAX_PAIRS, GU_SWEEP_MAX_PAIRS / 4);
    GU_TRY(gu_dyna_init(h));  // the model, allocated if need be, and a queue of this state count, both cleared (another state count: both dropped)
    if (h->d_sweep_heap) return GU_OK;
    const size_t pairs = (size_t)h->N * (size_t)h->S * 4;
    const size_t heap_bytes = (pairs + 2 * (size_t)h->N) * sizeof(uint64_t);
    gu_release(h->d_sweep_pos, h->d_sweep_size);  // (left behind by a call that ran out of memory)
    GU_TRY(gu_tabular_fits(h, heap_bytes + pairs * sizeof(int32_t) + (size_t)h->N * sizeof(int32_t), "priority queues"));
    GU_HIP(hipMalloc(&h->d_sweep_size, (size_t)h->N * sizeof(int32_t)));
    GU_HIP(hipMalloc(&h->d_sweep_pos, pairs * sizeof(int32_t)));
    GU_HIP(hipMalloc(&h->d_sweep_heap, heap_bytes));  // the last one: a heap means a whole queue
    GU_TRY(gu_sweep_clear(h));
    GU_HIP(hipStreamSynchronize(h->stream));
    return GU_OK;
}

int gu_sweep_run(gu_handle h, int64_t T, int32_t P, double theta, double alpha, double gamma, uint32_t eps_q16, uint32_t flags)
{
    GU_ENTER(h);
    GU_NO_OVERLAY(h, "gu_sweep_run");
    GU_NEED_GRID(h);
    GU_NEED_Q(h);
    GU_NEED_SWEEP(h);
    GU_REQUIRE(P >= 0 && P <= 256, GU_ERR_INVALID, "planning steps %d out of range (0 .. 256)", P);
    GU_REQUIRE(std::isfinite(theta) && theta >= 0.0, GU_ERR_INVALID, "theta must be finite and not negative");
    int rc = gu_tabular_check(h, "gu_sweep_run", T, P, eps_q16, alpha, gamma, flags);
    if (rc != GU_OK || T == 0) return rc;
    return gu_launch_sweep(h, T, P, theta, alpha, gamma, eps_q16, flags);
}

int gu_sweep_get_queue(gu_handle h, int64_t env0, int64_t n, uint64_t *key, int32_t *size)
{
    GU_ENTER(h);
    GU_NEED_GRID(h);
    GU_NEED_SWEEP(h);
    GU_TRY(gu_env_range(h, env0, n));
    const size_t pairs = (size_t)h->S * 4;
    std::vector<uint64_t> heap(key ? (size_t)n * (pairs + 2) : 0);
    std::vector<int32_t> sz((size_t)n);
    GU_TRY(gu_sweep_rows(h, env0, n, key ? heap.data() : nullptr, nullptr, sz.data()));
    for (int64_t e = 0; e < n; ++e) {
        if (size) size[e] = sz[e];
        if (!key) continue;
        uint64_t *out = key + (size_t)e * pairs;
        const uint64_t *row = heap.data() + (size_t)e * (pairs + 2);
        std::fill(out, out + pairs, 0ull);
        for (size_t i = 1; i <= std::min((size_t)std::max(sz[e], 0), pairs); ++i)
            if ((row[i] & 0xFFFFull) < pairs) out[row[i] & 0xFFFFull] = row[i];
    }
    return GU_OK;
}

int gu_diag_sweep_heap(gu_handle h, int64_t env0, int64_t n, uint64_t *heap, int32_t *pos)
{
    GU_ENTER(h);
    GU_NEED_GRID(h);
    GU_NEED_SWEEP(h);
    GU_TRY(gu_env_range(h, env0, n));
    return gu_sweep_rows(h, env0, n, heap, pos, nullptr);
}

}  // extern "C"
