// gu_search.hip -- batched simulation-based search for gfx950: Monte-Carlo rollouts at decision time (Sutton & Barto 8.10, "rollout
// algorithms"; include/gu.h: gu_search_run; restated on the CPU by tests/_search_oracle.py).  Learner e owns env e and its gu_td_*
// table; before each non-exploring real move it simulates M rollouts of depth D per action with the TRUE model -- the move rule on
// the staged cell map, the one the real step uses -- under an epsilon-greedy rollout policy on its table, bootstraps a truncated
// rollout on max Q at the leaf, takes the action with the largest summed return and learns from the real transition by
// gu_td_kernel's Q-learning step.  The lane, the Q-row rules and the rounding are gu_tabular.hpp's.
//
// ONE LOOP, TWO LANE MODES (gu_reinforce.hip's structure).  Rollouts end at different depths in different lanes and exploring
// lanes run none, so a search written as loops inside the real step would make every lane of the wave wait for the longest
// rollout of every action.  Instead every turn of the loop a lane does one unit of work:
//   act : the head of a real step (rule 1-3: reset, word, epsilon test); an exploring lane, or any lane with M = 0, takes its
//         real step in the same turn; a searching lane opens its search (the four first moves are taken as their action comes up);
//   sim : one simulated move of the rollout it is in.  The move that ends a rollout (terminal cell, or depth D: the leaf's row
//         and its maximum) also adds the return to the action's sum and begins the next rollout; the move that ends the last
//         rollout of action 3 chooses the action, and the lane takes its real step in the same turn.
// A lane carries (b, j, k, x, G, disc, acc, the score row) in registers, leaves when its T real steps are done, and never waits
// for another lane's rollout.  Nothing is written during a search, so the row of the current state that TabLane keeps stays valid.
//
// THE CHAIN of one simulated move: row Q[x] (32 bytes, two 16-byte loads) -> action -> cell lookup (LDS, or L2) -> next row.  The
// stream-6 word depends on the counter c alone and is hashed at the top of the turn, in the shadow of the row's load, which went out
// at the end of the turn before.  UNI (eps_sim_q16 == 65536: the uniform rollout policy, the textbook's default) needs no row
// until the leaf: its chain is the cell lookup alone.
//
// SKIPS, both byte-exact: an action whose first move is terminal scores (double)(M * r1) -- the M returns are the integer r1 each
// and every partial sum of at most 64 integers below 2^7 in magnitude is exact --; with D = 0 the M returns of an action are one
// value, computed once and added M - 1 times.
#include "gu_tabular.hpp"

struct SearchArgs : TabArgs {
    int32_t M, D;          // rollouts per action (0 .. GU_SEARCH_MAX_M), their depth (0 .. GU_SEARCH_MAX_D)
    uint32_t eps_sim_q16;  // the rollout policy's epsilon
    double *score;         // [N][4] the score row of the env's most recent searched iteration
    int64_t *sim_steps;    // [N] simulated moves of this launch
};

// the stream-6 word of simulated move c.  The prefix of c's epoch is cached in (pre, epoch) and recomputed where c enters
// another epoch -- a wave-uniform test, the block out of line (as gu_dyna_pick)
__device__ __forceinline__ uint32_t gu_search_word(uint32_t &pre, uint32_t &epoch, uint32_t seed_prefix, uint32_t env, uint64_t c)
{
    const uint32_t hi = (uint32_t)(c >> 32);
    if (__builtin_expect(__builtin_amdgcn_ballot_w64(hi != epoch) != 0ull, 0)) {
        const uint32_t p = gu_rng_prefix(gu_rng_seed_prefix_epoch(seed_prefix, hi), env);
        pre = hi != epoch ? p : pre;
        epoch = hi;
    }
    return gu_rng_word(pre, GU_RNG_STREAM_SEARCH, (uint32_t)c);
}

template <bool UNI, bool LDS>
__global__ void __launch_bounds__(GU_BLOCK) gu_search_kernel(const SearchArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    TabLane<LDS> L(a, smem);
    if (L.e < a.N) {
        L.begin(a);
        const int32_t M = a.M, D = a.D;
        const double *qe = L.qe;  // (not __restrict__: the real step's update writes the table the rollouts read)
        int32_t i = 0;          // real steps done
        bool sim = false;       // sim mode: inside rollout j of action b
        bool searched = false;  // sc holds the score row of a searched iteration of this launch
        uint32_t w = 0u;        // the stream-4 word of the real step being decided
        uint32_t b = 0u;        // the action being scored
        int32_t j = 0, k = 0;   // rollout of b, simulated moves of it done
        int32_t s1 = 0, r1 = 0; // the first move from (s, b)
        uint32_t f1 = 0u;
        int32_t x = 0;          // the rollout's state, its cell flags
        uint32_t fx = 0u;
        uint64_t c = 0ull;      // the counter of the next simulated move
        double G = 0.0, disc = 0.0, acc = 0.0;
        QRow sc{0.0, 0.0, 0.0, 0.0}, row{0.0, 0.0, 0.0, 0.0};
        int64_t nsim = 0;
        uint32_t epoch6 = (uint32_t)((L.t * 4ull * (uint64_t)M * (uint64_t)D) >> 32);
        uint32_t pre6 = gu_rng_prefix(gu_rng_seed_prefix_epoch(a.seed_prefix, epoch6), L.env);

        // rollout j of action b begins behind its first move
        auto begin_rollout = [&]() {
            G = (double)r1;
            disc = a.gamma;
            x = s1;
            fx = f1;
            k = 0;
            c = ((L.t * 4ull + (uint64_t)b) * (uint64_t)M + (uint64_t)(uint32_t)j) * (uint64_t)D;
            if (!UNI) row = gu_q_load(qe + (int64_t)x * 4);
        };
        // from action b on: the first move of each action in turn.  An action whose rollouts simulate nothing is scored on the
        // spot; the first one that needs simulated moves begins its rollout 0.  Ends with b == 4 when no action is left.
        auto open = [&]() {
            for (; b < 4u; ++b) {
                s1 = gu_move(L.s, L.m.f[L.s], b, gu_delta<LDS>(b, a.lut, a.W));
                f1 = L.m.f[s1];
                r1 = L.m.r[s1];
                double tot;
                if ((f1 >> GU_CELL_TERM_BIT) & 1u) {
                    tot = (double)(M * r1);
                } else if (D == 0) {
                    const double g0 = __dadd_rn((double)r1, __dmul_rn(a.gamma, gu_q_max(gu_q_load(qe + (int64_t)s1 * 4))));
                    tot = g0;
                    for (int32_t jj = 1; jj < M; ++jj) tot = __dadd_rn(tot, g0);
                } else {
                    break;
                }
                gu_q_put(sc, b, tot);
            }
            if (b < 4u) {
                j = 0;
                begin_rollout();
            }
        };

        while (i < a.T) {
            bool go = false;  // the action of the real step is decided: take it in this turn
            uint32_t ua = 0u;
            if (sim) {
                // ---- one simulated move
                const uint32_t wq = gu_search_word(pre6, epoch6, a.seed_prefix, L.env, c);
                const uint32_t u = UNI ? (wq & 3u) : gu_q_action(row, wq, a.eps_sim_q16);
                x = gu_move(x, fx, u, gu_delta<LDS>(u, a.lut, a.W));
                fx = L.m.f[x];
                const int32_t rr = L.m.r[x];
                const bool dn = ((fx >> GU_CELL_TERM_BIT) & 1u) != 0u;
                G = __dadd_rn(G, __dmul_rn(disc, (double)rr));
                disc = __dmul_rn(disc, a.gamma);
                ++c;
                ++k;
                ++nsim;
                const bool leaf = !dn && k == D;
                if (!dn && (!UNI || leaf)) row = gu_q_load(qe + (int64_t)x * 4);
                if (dn || leaf) {
                    // ---- the rollout's end: its return into the action's sum, then the next rollout, action, or the real step
                    if (leaf) G = __dadd_rn(G, __dmul_rn(disc, gu_q_max(row)));
                    acc = j == 0 ? G : __dadd_rn(acc, G);
                    ++j;
                    if (j == M) {
                        gu_q_put(sc, b, acc);
                        ++b;
                        open();
                    } else {
                        begin_rollout();
                    }
                    go = b == 4u;
                }
            } else {
                // ---- the head of a real step: rules 1-3
                L.reset(a);
                w = L.word();
                if (M == 0 || (w >> 16) < a.eps_q16) {
                    ua = gu_q_action(L.q, w, a.eps_q16);
                    go = true;
                } else {
                    b = 0u;
                    open();
                    sim = true;
                    go = b == 4u;
                }
            }
            if (go) {
                if (sim) {  // (a searched iteration: the tie rule on the score row; w is past the epsilon test)
                    ua = gu_q_action(sc, w, a.eps_q16);
                    searched = true;
                    sim = false;
                }
                // ---- rules 4-5: gu_td_kernel's Q-learning step
                const int32_t s2 = L.move(a, ua);
                QRow n = L.next_row(s2);
                const double target = L.d ? (double)L.r : __dadd_rn((double)L.r, __dmul_rn(a.gamma, gu_q_max(n)));
                L.update(a, (int64_t)L.s * 4 + ua, ua, s2, n, target);
                L.step(a, i, s2, n);
                ++i;
            }
        }
        L.end(a);
        if (searched) {
            double2 *out = reinterpret_cast<double2 *>(a.score + L.e * 4);
            out[0] = make_double2(sc.v0, sc.v1);
            out[1] = make_double2(sc.v2, sc.v3);
        }
        a.sim_steps[L.e] = nsim;
    }
    L.ballot(a);
}

static int gu_launch_search(gu_engine *h, int64_t T, int32_t M, int32_t D, double alpha, double gamma, uint32_t eps_q16, uint32_t eps_sim_q16,
                     uint32_t flags)
{
    SearchArgs a{};
    gu_tabular_args(h, a, T, alpha, gamma, eps_q16, flags);
    a.M = M;
    a.D = D;
    a.eps_sim_q16 = eps_sim_q16;
    a.score = h->d_search_score;
    a.sim_steps = h->d_search_steps;
    const int rc = eps_sim_q16 == 65536u ? gu_tabular_launch(h, gu_search_kernel<true, true>, gu_search_kernel<true, false>, a)
                                         : gu_tabular_launch(h, gu_search_kernel<false, true>, gu_search_kernel<false, false>, a);
    return rc != GU_OK ? rc : gu_tabular_after(h, T, flags);
}

void gu_search_free(gu_engine *h) { gu_release(h->d_search_score, h->d_search_steps); }

extern "C" {

int gu_search_run(gu_handle h, int64_t T, int32_t M, int32_t D, double alpha, double gamma, uint32_t eps_q16, uint32_t eps_sim_q16,
                  uint32_t flags)
{
    GU_ENTER(h);
    GU_NO_OVERLAY(h, "gu_search_run");
    GU_NEED_GRID(h);
    GU_NEED_Q(h);
    GU_REQUIRE(M >= 0 && M <= GU_SEARCH_MAX_M, GU_ERR_INVALID, "simulations %d out of range (0 .. %d)", M, GU_SEARCH_MAX_M);
    GU_REQUIRE(D >= 0 && D <= GU_SEARCH_MAX_D, GU_ERR_INVALID, "depth %d out of range (0 .. %d)", D, GU_SEARCH_MAX_D);
    GU_REQUIRE(eps_sim_q16 <= 65536u, GU_ERR_INVALID, "eps_sim_q16 %u above 65536", eps_sim_q16);
    GU_TRY(gu_tabular_check(h, "gu_search_run", T, -1, eps_q16, alpha, gamma, flags));
    GU_TRY(gu_move_budget(T, 1 + 4 * (int64_t)M * D, "1 + 4 M D"));  // per real step, at most
    if (T == 0) return GU_OK;
    if (!h->d_search_score) {
        GU_HIP(hipStreamSynchronize(h->stream));
        GU_TRY(gu_tabular_fits(h, (size_t)h->N * (4 * sizeof(double) + sizeof(int64_t)), "search scores"));
        GU_HIP(hipMalloc(&h->d_search_score, (size_t)h->N * 4 * sizeof(double)));
        GU_HIP(hipMalloc(&h->d_search_steps, (size_t)h->N * sizeof(int64_t)));
        GU_HIP(hipMemsetAsync(h->d_search_score, 0, (size_t)h->N * 4 * sizeof(double), h->stream));
        GU_HIP(hipMemsetAsync(h->d_search_steps, 0, (size_t)h->N * sizeof(int64_t), h->stream));
    }
    return gu_launch_search(h, T, M, D, alpha, gamma, eps_q16, eps_sim_q16, flags);
}

int gu_search_get(gu_handle h, int64_t env0, int64_t n, double *score, int64_t *sim_steps)
{
    GU_ENTER(h);
    GU_NEED_GRID(h);
    GU_NEED_Q(h);
    GU_TRY(gu_env_range(h, env0, n));
    GU_HIP(hipStreamSynchronize(h->stream));
    if (!n) return GU_OK;
    if (!h->d_search_score) {  // (nothing searched yet: what the storage holds right after its allocation)
        if (score) std::fill(score, score + (size_t)n * 4, 0.0);
        if (sim_steps) std::fill(sim_steps, sim_steps + (size_t)n, (int64_t)0);
        return GU_OK;
    }
    GU_TRY(gu_env_copy(h, hipMemcpyDeviceToHost, score, h->d_search_score, env0, n, 4, false));
    return gu_env_copy(h, hipMemcpyDeviceToHost, sim_steps, h->d_search_steps, env0, n, 1, false);
}

}  // extern "C"
