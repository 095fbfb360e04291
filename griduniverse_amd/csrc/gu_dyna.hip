// gu_dyna.hip -- batched tabular Dyna-Q for gfx950 (Sutton & Barto 8.2; include/gu.h: gu_dyna_run; restated on the CPU by
// tests/_dyna_oracle.py): learner e learns into its gu_td_* table with gu_td_kernel's Q-learning step (gu_tabular.hpp: the lane,
// the Q-row rules, the table layout and the rounding) and keeps a learned model of its deterministic env, from which it replays
// P planning updates after every real step.
//
// The env is deterministic, so while the cells are the ones the model was cleared under (no grid install since gu_dyna_init), a pair's
// outcome never changes: the step loads the byte of seen bits of s (N * S bytes in all -- the 8-byte model words are 8 * 4 times
// more, and reading them every step cost the P = 0 path a third of gu_td_run's rate at 65 536 learners) and writes the model
// word, the list entry and the bit on a first observation only.  After a grid install that kept the model, the step loads the
// model word of (s, a) instead and stores it back when it differs.
// Model layout, learner-major like the tables:
//   model [N][S*4] uint64   one word per (s, a): low half the reward (int32), high half s' | done << 31; all ones = unobserved
//   list  [N][S*4] int32    the observed pairs s*4+a in the order of first observation (entries >= count stay -1)
//   count [N] int32
//   seen  [N][S] uint8      bit a of byte s: (s, a) observed
// so a planning update reads one list entry, one model word, the row Q[s'_p] (skipped when d_p) and the entry Q[s_p][a_p], and
// writes that entry back.  List and model do not change during planning, so both are software-pipelined: the list entry of
// update j+2 and the model word of update j+1 are in flight while update j gathers its Q row; what stays on the dependent
// chain per update is one Q gather and the store of the updated entry.  Q loads issued after a store to the same address see
// it (one lane's vector memory operations to one address complete in order), so a planning update reads what the updates
// before it wrote, as the semantics require.
// A planning update that writes an entry of the row kept in VGPRs forwards the value into it, so the next real step chooses
// its action from the table after planning.
#include "gu_tabular.hpp"

struct DynaArgs : TabArgs {
    int32_t P;
    uint64_t *model;  // [N][S*4]
    int32_t *list;    // [N][S*4]
    int32_t *count;   // [N]
    uint8_t *seen;    // [N][S] bit a of byte s: (s, a) observed
    int32_t exact;    // 1: the model holds only outcomes of the current cells (the seen bits decide); 0: compare every word
};

// stream-5 prefix of planning draw c (epoch c >> 32 hashed behind the seed, then the env)
__device__ __forceinline__ uint32_t gu_dyna_prefix(uint32_t seed_prefix, uint32_t env, uint64_t c)
{
    return gu_rng_prefix(gu_rng_seed_prefix_epoch(seed_prefix, (uint32_t)(c >> 32)), env);
}

// the list index drawn for planning update c: (word * count) >> 32.  The prefix of c's epoch is cached in (pre, epoch) and
// recomputed where c enters another epoch -- a wave-uniform test, the block out of line.
__device__ __forceinline__ uint32_t gu_dyna_pick(uint32_t &pre, uint32_t &epoch, uint32_t seed_prefix, uint32_t env, uint64_t c, uint32_t count)
{
    const uint32_t hi = (uint32_t)(c >> 32);
    if (__builtin_expect(__builtin_amdgcn_ballot_w64(hi != epoch) != 0ull, 0)) {
        const uint32_t p = gu_dyna_prefix(seed_prefix, env, c);
        pre = hi != epoch ? p : pre;
        epoch = hi;
    }
    return __umulhi(gu_rng_word(pre, GU_RNG_STREAM_DYNA, (uint32_t)c), count);
}

template <bool PLAN, bool LDS>
__global__ void __launch_bounds__(GU_BLOCK) gu_dyna_kernel(const DynaArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    TabLane<LDS> L(a, smem);
    if (L.e < a.N) {
        L.begin(a);
        const int64_t e = L.e, SA = (int64_t)a.S * 4;
        double *__restrict__ qe = L.qe;
        uint64_t *__restrict__ me = a.model + e * SA;
        int32_t *__restrict__ le = a.list + e * SA;
        uint8_t *__restrict__ se = a.seen + e * (int64_t)a.S;
        uint32_t count = (uint32_t)a.count[e];
        // stream 5: the prefix of the epoch of the first planning draw, then cached
        const uint64_t c0 = L.t * (uint64_t)a.P;
        uint32_t pre5 = PLAN ? gu_dyna_prefix(a.seed_prefix, L.env, c0) : 0u, epoch5 = (uint32_t)(c0 >> 32);
        for (int32_t i = 0; i < a.T; ++i) {
            L.reset(a);
            const int32_t s = L.s;
            const uint32_t ua = gu_q_action(L.q, L.word(), a.eps_q16);
            const int32_t sa = s * 4 + (int32_t)ua;
            const uint64_t t_old = L.t;
            const int32_t s2 = L.move(a, ua);
            QRow n = L.next_row(s2);
            // the model's load goes out behind the Q[s'] gather and lands in its shadow (issued at the top of the step, the wait
            // before the action choice would take its whole latency)
            const uint32_t bits = a.exact ? (uint32_t)se[s] : 0u;
            const uint64_t seen = a.exact ? 0ull : me[sa];
            // (the max only behind a non-terminal s': computed ahead of the select, it changes the register allocation)
            const double target = L.d ? (double)L.r : __dadd_rn((double)L.r, __dmul_rn(a.gamma, gu_q_max(n)));
            L.update(a, sa, ua, s2, n, target);
            // model update.  While the cells are those the model was cleared under, an observed pair's word can only be
            // written again with the same value: only a first observation writes (word, list entry, seen bit).  After a grid
            // install that kept the model, every observation is compared with the stored word.
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
            if (PLAN) {
                // planning: updates c = t_old * P + j, j = 0 .. P-1; pipeline: p0 = the list entry of update j, p1 = that of j+1,
                // w0 = the model word of update j
                const int32_t P = a.P;
                uint64_t c = t_old * (uint64_t)P;
                int32_t p0 = le[gu_dyna_pick(pre5, epoch5, a.seed_prefix, L.env, c, count)];
                int32_t p1 = P > 1 ? le[gu_dyna_pick(pre5, epoch5, a.seed_prefix, L.env, c + 1, count)] : p0;
                uint64_t w0 = me[p0];
                for (int32_t j = 0; j < P; ++j) {
                    const uint64_t w1 = j + 1 < P ? me[p1] : w0;
                    const int32_t p2 = j + 2 < P ? le[gu_dyna_pick(pre5, epoch5, a.seed_prefix, L.env, c + (uint64_t)(j + 2), count)] : p1;
                    const uint32_t hi = (uint32_t)(w0 >> 32);
                    const int32_t sp2 = (int32_t)(hi & 0x7FFFFFFFu), rp = (int32_t)(uint32_t)w0;
                    const bool dp = (hi >> 31) != 0u;
                    double qp = qe[p0];
                    double mx = 0.0;
                    if (!dp) mx = gu_q_max(gu_q_load(qe + (int64_t)sp2 * 4));
                    const double tgt = dp ? (double)rp : __dadd_rn((double)rp, __dmul_rn(a.gamma, mx));
                    qp = __dadd_rn(qp, __dmul_rn(a.alpha, __dsub_rn(tgt, qp)));
                    qe[p0] = qp;
                    if ((p0 >> 2) == s2) gu_q_put(n, (uint32_t)p0 & 3u, qp);  // keep the row in VGPRs current
                    p0 = p1;
                    p1 = p2;
                    w0 = w1;
                }
            }
            L.step(a, i, s2, n);
        }
        a.count[e] = (int32_t)count;
        L.end(a);
    }
    L.ballot(a);
}

static int gu_launch_dyna(gu_engine *h, int64_t T, int32_t P, double alpha, double gamma, uint32_t eps_q16, uint32_t flags)
{
    DynaArgs a{};
    gu_tabular_args(h, a, T, alpha, gamma, eps_q16, flags);
    a.P = P;
    a.model = h->d_dyna_model;
    a.list = h->d_dyna_list;
    a.count = h->d_dyna_count;
    a.seen = h->d_dyna_seen;
    a.exact = h->dyna_exact ? 1 : 0;
    const int rc = P > 0 ? gu_tabular_launch(h, gu_dyna_kernel<true, true>, gu_dyna_kernel<true, false>, a)
                         : gu_tabular_launch(h, gu_dyna_kernel<false, true>, gu_dyna_kernel<false, false>, a);
    return rc != GU_OK ? rc : gu_tabular_after(h, T, flags);
}

void gu_dyna_free(gu_engine *h)
{
    gu_release(h->d_dyna_model, h->d_dyna_list, h->d_dyna_count, h->d_dyna_seen);
    gu_release(h->d_sweep_heap, h->d_sweep_pos, h->d_sweep_size);  // gu_sweep.hip's queues hold pairs of this model
    h->dyna_S = 0;
    h->dyna_exact = false;
}

#define GU_NEED_DYNA(h) GU_REQUIRE(GU_HAS_DYNA(h), GU_ERR_STATE, "no Dyna-Q model: call gu_dyna_init first")

extern "C" {

int gu_dyna_init(gu_handle h)
{
    GU_ENTER(h);
    GU_NEED_GRID(h);
    gu_tabular_drop_carry(h);
    const size_t pairs = (size_t)h->N * (size_t)h->S * 4;
    if (!h->d_dyna_model || h->dyna_S != h->S) {
        GU_HIP(hipStreamSynchronize(h->stream));
        gu_dyna_free(h);
        const size_t bytes = pairs * (sizeof(uint64_t) + sizeof(int32_t)) + (size_t)h->N * (sizeof(int32_t) + (size_t)h->S);
        GU_TRY(gu_tabular_fits(h, bytes, "Dyna-Q models"));
        GU_HIP(hipMalloc(&h->d_dyna_model, pairs * sizeof(uint64_t)));
        GU_HIP(hipMalloc(&h->d_dyna_list, pairs * sizeof(int32_t)));
        GU_HIP(hipMalloc(&h->d_dyna_count, (size_t)h->N * sizeof(int32_t)));
        GU_HIP(hipMalloc(&h->d_dyna_seen, (size_t)h->N * (size_t)h->S));
        h->dyna_S = h->S;
    }
    h->dyna_exact = true;
    GU_HIP(hipMemsetAsync(h->d_dyna_model, 0xFF, pairs * sizeof(uint64_t), h->stream));
    GU_HIP(hipMemsetAsync(h->d_dyna_list, 0xFF, pairs * sizeof(int32_t), h->stream));
    GU_HIP(hipMemsetAsync(h->d_dyna_count, 0, (size_t)h->N * sizeof(int32_t), h->stream));
    GU_HIP(hipMemsetAsync(h->d_dyna_seen, 0, (size_t)h->N * (size_t)h->S, h->stream));
    GU_TRY(gu_sweep_clear(h));  // a queued pair must not outlive its model entry
    GU_HIP(hipStreamSynchronize(h->stream));
    return GU_OK;
}

int gu_dyna_run(gu_handle h, int64_t T, int32_t P, double alpha, double gamma, uint32_t eps_q16, uint32_t flags)
{
    GU_ENTER(h);
    GU_NO_OVERLAY(h, "gu_dyna_run");
    GU_NEED_GRID(h);
    GU_NEED_Q(h);
    GU_NEED_DYNA(h);
    GU_REQUIRE(P >= 0 && P <= 256, GU_ERR_INVALID, "planning steps %d out of range (0 .. 256)", P);
    int rc = gu_tabular_check(h, "gu_dyna_run", T, P, eps_q16, alpha, gamma, flags);
    if (rc != GU_OK || T == 0) return rc;
    return gu_launch_dyna(h, T, P, alpha, gamma, eps_q16, flags);
}

int gu_dyna_get_model(gu_handle h, int64_t env0, int64_t n, int32_t *next, int32_t *reward, int32_t *done, int32_t *list, int32_t *count)
{
    GU_ENTER(h);
    GU_NEED_GRID(h);
    GU_NEED_DYNA(h);
    GU_TRY(gu_env_range(h, env0, n));
    const size_t pairs = (size_t)h->S * 4, k = (size_t)n * pairs;
    GU_HIP(hipStreamSynchronize(h->stream));
    if (!n) return GU_OK;
    if (next || reward || done) {
        std::vector<uint64_t> words(k);
        GU_TRY(gu_env_copy(h, hipMemcpyDeviceToHost, words.data(), h->d_dyna_model, env0, n, pairs, false));
        for (size_t i = 0; i < k; ++i) {
            const uint64_t w = words[i];
            const bool seen = w != ~0ull;
            const uint32_t hi = (uint32_t)(w >> 32);
            if (next) next[i] = seen ? (int32_t)(hi & 0x7FFFFFFFu) : -1;
            if (reward) reward[i] = seen ? (int32_t)(uint32_t)w : 0;
            if (done) done[i] = seen ? (int32_t)(hi >> 31) : 0;
        }
    }
    GU_TRY(gu_env_copy(h, hipMemcpyDeviceToHost, list, h->d_dyna_list, env0, n, pairs, false));
    return gu_env_copy(h, hipMemcpyDeviceToHost, count, h->d_dyna_count, env0, n, 1, false);
}

}  // extern "C"
