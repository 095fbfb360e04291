// gu_mcts.hip -- batched Monte-Carlo tree search (UCT) at decision time for gfx950 (Kocsis & Szepesvari 2006; Sutton & Barto 8.11;
// include/gu.h: gu_mcts_run; restated on the CPU by tests/_mcts_oracle.py).  Learner e owns env e, its gu_td_* table and a pool of
// tree nodes in HBM; before each non-exploring real move it rebuilds a search tree at the state it stands in by M simulations with
// the TRUE model -- selection by UCB1 on the tree's own statistics, one new node, gu_search.hip's rollout with its leaf bootstrap on
// max Q, backup along the parent links --, takes the root action with the largest mean return and learns from the real transition
// by gu_td_kernel's Q-learning step.  The lane, the Q-row rules and the rounding are gu_tabular.hpp's.
//
// ONE LOOP, FOUR LANE MODES (gu_search.hip's act / sim structure, sim split in three).  Every turn of the loop a lane does one unit:
//   act  : the head of a real step (rules 1-3: reset, word, epsilon test); an exploring lane, or any lane with M = 0, takes its real
//          step in the same turn; a searching lane writes its root node and opens simulation 0;
//   sel  : one level of the tree: the score row of node v from its rows, the tie rule, the simulated move.  It ends in the child
//          (the next turn's node), in a new node and the rollout behind it, or -- terminal cell -- in the backup;
//   roll : one simulated move of the rollout (gu_search.hip's, D = 0 bootstraps in the sel turn);
//   back : one edge of the backup.  The root edge ends the simulation: the next one opens, or, behind simulation M - 1, the lane
//          forms the final row and takes its real step in the same turn.
// A lane deep in its tree or in a long rollout never holds back the other lanes of its wave beyond the turn they share.
//
// THE POOL.  Node v of learner e is ONE aligned 64-byte piece at pool + (e * P + v) * 64: w[4] float64 (32 bytes) | visits[4]
// uint32 (16) | child[4] int32 (16) -- the three rows selection needs come out of the node index alone, four 16-byte loads that
// leave together: one memory round trip per tree level (the move itself is an LDS lookup).  What only the backup needs sits apart,
// meta[e * P + v] = (state, parent * 4 + action): 8 bytes, so that selection never drags it through the cache.  Learner-major like
// the Q tables: no two lanes share a node, so nothing coalesces across lanes anyway, and the host copies a learner's tree as one piece.
// THE PATH needs no stack: the backup follows the parent links; the reward of the edge into node v is the reward plane at v's
// state (a reward depends on the arrival cell alone); the reward of the last edge -- whose target may be no node at all -- waits
// in a register.  A back turn loads meta[v] beside the two entries it updates, all three addresses from v: one round trip per edge.
// A lane reads back only what it wrote itself, in program order; nothing in the pool is shared between lanes.
//
// THE SCHEDULE IS DATA (gu_explore.hip): U | B | I, float64, shared by all learners, staged into LDS behind the planes under
// gu_explore.hip's budget rule (planes + tables within the share of a CU's LDS that leaves room for 2048 lanes), read through L2
// otherwise.  The kernel has no log, sqrt or division.
#include "gu_tabular.hpp"

struct MctsArgs : TabArgs {
    int32_t M, H, D;       // simulations per decision (0 .. P - 1), the tree's depth cap, the rollout depth
    uint32_t eps_sim_q16;  // the rollout policy's epsilon
    uint8_t *pool;         // [N][P] nodes of 64 bytes: w[4] | visits[4] | child[4]
    int2 *meta;            // [N][P] (state, parent * 4 + action; -1 for the root)
    int32_t P;             // nodes per learner
    int32_t *nodes;        // [N] nodes of the env's most recent searched iteration
    int64_t *sim_steps;    // [N] simulated moves of this launch
    const double *tab;     // U[C] | B[C] | I[C]
    int32_t C;
    int32_t tab_lds;       // bytes of tab the LDS kernels stage behind the planes (0: read it through L2)
};

// the stream-8 word of draw c, gu_search_word's epoch cache: the prefix of c's epoch in (pre, epoch), recomputed where c enters
// another epoch -- a wave-uniform test, the block out of line
__device__ __forceinline__ uint32_t gu_mcts_word(uint32_t &pre, uint32_t &epoch, uint32_t seed_prefix, uint32_t env, uint64_t c)
{
    const uint32_t hi = (uint32_t)(c >> 32);
    if (__builtin_expect(__builtin_amdgcn_ballot_w64(hi != epoch) != 0ull, 0)) {
        const uint32_t p = gu_rng_prefix(gu_rng_seed_prefix_epoch(seed_prefix, hi), env);
        pre = hi != epoch ? p : pre;
        epoch = hi;
    }
    return gu_rng_word(pre, GU_RNG_STREAM_MCTS, (uint32_t)c);
}

__device__ __forceinline__ int32_t gu_mcts_child(const int4 &c, uint32_t a) { return a == 0u ? c.x : a == 1u ? c.y : a == 2u ? c.z : c.w; }

// the three rows of one node
struct MctsNode {
    QRow w;
    uint4 n;
    int4 ch;
};

__device__ __forceinline__ MctsNode gu_mcts_load(const uint8_t *node)
{
    return MctsNode{gu_q_load(reinterpret_cast<const double *>(node)), *reinterpret_cast<const uint4 *>(node + 32),
                    *reinterpret_cast<const int4 *>(node + 48)};
}

// a node without statistics or children
__device__ __forceinline__ void gu_mcts_clear(uint8_t *node)
{
    reinterpret_cast<double2 *>(node)[0] = make_double2(0.0, 0.0);
    reinterpret_cast<double2 *>(node)[1] = make_double2(0.0, 0.0);
    *reinterpret_cast<uint4 *>(node + 32) = make_uint4(0u, 0u, 0u, 0u);
    *reinterpret_cast<int4 *>(node + 48) = make_int4(-1, -1, -1, -1);
}

// w_b * I[n_b] of the four actions, `none` where n_b == 0 (t: U | B | I, indices clamped to C - 1)
__device__ __forceinline__ QRow gu_mcts_means(const double *t, uint32_t C, const MctsNode &nd, double none)
{
    const uint32_t top = C - 1u;
    const double *I = t + 2 * C;
    return QRow{nd.n.x ? __dmul_rn(nd.w.v0, I[min(nd.n.x, top)]) : none, nd.n.y ? __dmul_rn(nd.w.v1, I[min(nd.n.y, top)]) : none,
                nd.n.z ? __dmul_rn(nd.w.v2, I[min(nd.n.z, top)]) : none, nd.n.w ? __dmul_rn(nd.w.v3, I[min(nd.n.w, top)]) : none};
}

// the UCB1 score row of a node: mean + U[n_s] * B[n_b], +infinity for an untried action
__device__ __forceinline__ QRow gu_mcts_scores(const double *t, uint32_t C, const MctsNode &nd)
{
    const uint32_t top = C - 1u;
    const double inf = __builtin_huge_val();
    const double u = t[min(nd.n.x + nd.n.y + nd.n.z + nd.n.w, top)];  // (a node's visits sum to at most GU_MCTS_MAX_SIMS)
    const double *B = t + C;
    const QRow mean = gu_mcts_means(t, C, nd, inf);
    return QRow{nd.n.x ? __dadd_rn(mean.v0, __dmul_rn(u, B[min(nd.n.x, top)])) : inf, nd.n.y ? __dadd_rn(mean.v1, __dmul_rn(u, B[min(nd.n.y, top)])) : inf,
                nd.n.z ? __dadd_rn(mean.v2, __dmul_rn(u, B[min(nd.n.z, top)])) : inf, nd.n.w ? __dadd_rn(mean.v3, __dmul_rn(u, B[min(nd.n.w, top)])) : inf};
}

enum { GU_MCTS_ACT = 0, GU_MCTS_SEL = 1, GU_MCTS_ROLL = 2, GU_MCTS_BACK = 3 };

template <bool UNI, bool LDS>
__global__ void __launch_bounds__(GU_BLOCK) gu_mcts_kernel(const MctsArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const bool ltab = LDS && a.tab_lds;
    if (ltab)  // (the barrier behind the planes, in TabLane's constructor, covers these stores too)
        for (int32_t i = threadIdx.x * 16; i < a.tab_lds; i += blockDim.x * 16)
            *reinterpret_cast<uint4 *>(smem + 2 * a.cell_bytes + i) = *reinterpret_cast<const uint4 *>(reinterpret_cast<const uint8_t *>(a.tab) + i);
    TabLane<LDS> L(a, smem);
    if (L.e < a.N) {
        L.begin(a);
        const int32_t M = a.M, H = a.H, D = a.D;
        const uint32_t C = (uint32_t)a.C;
        const double *tab = ltab ? reinterpret_cast<const double *>(smem + 2 * a.cell_bytes) : a.tab;
        const double *qe = L.qe;  // (not __restrict__: the real step's update writes the table the rollouts read)
        uint8_t *pool = a.pool + L.e * (int64_t)a.P * 64;
        int2 *meta = a.meta + L.e * (int64_t)a.P;
        const uint64_t span = (uint64_t)(uint32_t)(H + D);  // stream-8 draws set aside for one simulation
        int32_t i = 0;            // real steps done
        int32_t mode = GU_MCTS_ACT;
        bool searched = false;    // the pool holds the tree of a searched iteration of this launch
        uint32_t w = 0u;          // the stream-4 word of the real step being decided
        int32_t j = 0;            // the simulation
        int32_t cnt = 0;          // nodes of the tree
        int32_t v = 0, depth = 0; // sel: the node, its depth
        MctsNode nd{QRow{0.0, 0.0, 0.0, 0.0}, make_uint4(0u, 0u, 0u, 0u), make_int4(-1, -1, -1, -1)};  // ... and its rows
        int32_t x = 0;            // the simulated state (sel: node v's), its cell flags
        uint32_t fx = 0u;
        int32_t k = 0;            // roll: moves of the rollout done
        int32_t bv = 0, br = 0;   // back: the edge (bv, bu) and its reward
        uint32_t bu = 0u;
        uint64_t c = 0ull;        // the counter of the next stream-8 draw
        double G = 0.0, disc = 0.0;
        QRow row{0.0, 0.0, 0.0, 0.0};
        int64_t nsim = 0;
        uint32_t epoch8 = (uint32_t)((L.t * (uint64_t)M * span) >> 32);
        uint32_t pre8 = gu_rng_prefix(gu_rng_seed_prefix_epoch(a.seed_prefix, epoch8), L.env);

        // simulation j opens at the root, whose rows are in nd
        auto open = [&]() {
            v = 0;
            depth = 0;
            x = L.s;
            fx = L.m.f[L.s];
            c = (L.t * (uint64_t)M + (uint64_t)(uint32_t)j) * span;
            mode = GU_MCTS_SEL;
        };

        while (i < a.T) {
            bool go = false;  // the action of the real step is decided: take it in this turn
            uint32_t ua = 0u;
            if (mode == GU_MCTS_SEL) {
                // ---- one level of the tree
                const uint32_t wq = gu_mcts_word(pre8, epoch8, a.seed_prefix, L.env, c);
                const uint32_t u = gu_q_action(gu_mcts_scores(tab, C, nd), wq, 0u);
                const int32_t x2 = gu_move(x, fx, u, gu_delta<LDS>(u, a.lut, a.W));
                const uint32_t f2 = L.m.f[x2];
                const int32_t r2 = L.m.r[x2];
                int32_t ch = gu_mcts_child(nd.ch, u);
                ++c;
                ++depth;
                ++nsim;
                bv = v;  // (where this is the simulation's last level, the backup begins at this edge)
                bu = u;
                br = r2;
                if ((f2 >> GU_CELL_TERM_BIT) & 1u) {
                    G = 0.0;
                    mode = GU_MCTS_BACK;
                } else if (ch >= 0 && depth < H) {
                    v = ch;
                    x = x2;
                    fx = f2;
                    nd = gu_mcts_load(pool + (int64_t)v * 64);
                } else {
                    if (ch < 0 && cnt < a.P) {  // (cnt <= j + 1 < P by construction)
                        gu_mcts_clear(pool + (int64_t)cnt * 64);
                        meta[cnt] = make_int2(x2, v * 4 + (int32_t)u);
                        reinterpret_cast<int32_t *>(pool + (int64_t)v * 64 + 48)[u] = cnt;
                        ++cnt;
                    }
                    x = x2;
                    fx = f2;
                    G = 0.0;
                    disc = 1.0;
                    k = 0;
                    if (!UNI || D == 0) row = gu_q_load(qe + (int64_t)x * 4);
                    if (D == 0) {
                        G = __dadd_rn(G, __dmul_rn(disc, gu_q_max(row)));
                        mode = GU_MCTS_BACK;
                    } else {
                        mode = GU_MCTS_ROLL;
                    }
                }
            } else if (mode == GU_MCTS_ROLL) {
                // ---- one simulated move of the rollout
                const uint32_t wq = gu_mcts_word(pre8, epoch8, a.seed_prefix, L.env, c);
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
                if (leaf) G = __dadd_rn(G, __dmul_rn(disc, gu_q_max(row)));
                if (dn || leaf) mode = GU_MCTS_BACK;
            } else if (mode == GU_MCTS_BACK) {
                // ---- one edge of the backup
                uint8_t *node = pool + (int64_t)bv * 64;
                double *pw = reinterpret_cast<double *>(node) + bu;
                uint32_t *pn = reinterpret_cast<uint32_t *>(node + 32) + bu;
                const double wv = *pw;
                const uint32_t nv = *pn;
                const int2 up = meta[bv];
                G = __dadd_rn((double)br, __dmul_rn(a.gamma, G));
                *pw = __dadd_rn(wv, G);
                *pn = nv + 1u;
                if (bv != 0) {
                    br = L.m.r[up.x];
                    bu = (uint32_t)up.y & 3u;
                    bv = up.y >> 2;
                } else {
                    // ---- the simulation's end: the next one, or the real step
                    ++j;
                    nd = gu_mcts_load(pool);
                    if (j == M) {
                        row = gu_mcts_means(tab, C, nd, -__builtin_huge_val());
                        go = true;
                    } else {
                        open();
                    }
                }
            } else {
                // ---- the head of a real step: rules 1-3
                L.reset(a);
                w = L.word();
                if (M == 0 || (w >> 16) < a.eps_q16) {
                    ua = gu_q_action(L.q, w, a.eps_q16);
                    go = true;
                } else {
                    nd = MctsNode{QRow{0.0, 0.0, 0.0, 0.0}, make_uint4(0u, 0u, 0u, 0u), make_int4(-1, -1, -1, -1)};
                    gu_mcts_clear(pool);
                    meta[0] = make_int2(L.s, -1);
                    cnt = 1;
                    j = 0;
                    open();
                }
            }
            if (go) {
                if (mode != GU_MCTS_ACT) {  // (a searched iteration: the tie rule on the final row; w is past the epsilon test)
                    ua = gu_q_action(row, w, a.eps_q16);
                    searched = true;
                    mode = GU_MCTS_ACT;
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
        if (searched) a.nodes[L.e] = cnt;
        a.sim_steps[L.e] = nsim;
    }
    L.ballot(a);
}

template <bool UNI>
static int gu_mcts_launch(gu_engine *h, MctsArgs &a)
{
    const int lds_bs = gu_lds_block(h, GU_BLOCK, 2);
    if (lds_bs) {
        // the tables go into LDS only where LDS then still admits 2048 lanes per CU (the wave limit): lds_per_cu / 2048 bytes per lane
        // (staged in 16-byte pieces: the bytes rounded up, which gu_mcts_set_tables allocated)
        const size_t planes = 2 * (size_t)h->cell_bytes, tab = ((size_t)a.C * 3 * sizeof(double) + 15) & ~(size_t)15;
        const size_t budget = (size_t)h->lds_per_cu / 2048 * (size_t)lds_bs;
        a.tab_lds = a.M > 0 && planes + tab <= budget ? (int32_t)tab : 0;
        hipLaunchKernelGGL((gu_mcts_kernel<UNI, true>), dim3(gu_blocks(h->N, lds_bs)), dim3(lds_bs), planes + (size_t)a.tab_lds, h->stream, a);
    } else {
        a.tab_lds = 0;
        hipLaunchKernelGGL((gu_mcts_kernel<UNI, false>), dim3(gu_blocks(h->N, GU_BLOCK)), dim3(GU_BLOCK), 0, h->stream, a);
    }
    GU_HIP(hipGetLastError());
    return GU_OK;
}

static int gu_launch_mcts(gu_engine *h, int64_t T, int32_t M, int32_t H, int32_t D, double alpha, double gamma, uint32_t eps_q16, uint32_t eps_sim_q16,
                   uint32_t flags)
{
    MctsArgs a{};
    gu_tabular_args(h, a, T, alpha, gamma, eps_q16, flags);
    a.M = M;
    a.H = H;
    a.D = D;
    a.eps_sim_q16 = eps_sim_q16;
    a.pool = h->d_mcts_pool;
    a.meta = reinterpret_cast<int2 *>(h->d_mcts_meta);
    a.P = h->mcts_P;
    a.nodes = h->d_mcts_nodes;
    a.sim_steps = h->d_mcts_steps;
    a.tab = h->d_mcts_tab;  // (nullptr while M == 0 needs none: never read then)
    a.C = h->mcts_C;
    const int rc = eps_sim_q16 == 65536u ? gu_mcts_launch<true>(h, a) : gu_mcts_launch<false>(h, a);
    return rc != GU_OK ? rc : gu_tabular_after(h, T, flags);
}

void gu_mcts_free(gu_engine *h)
{
    gu_release(h->d_mcts_pool, h->d_mcts_meta, h->d_mcts_nodes, h->d_mcts_steps);
    h->mcts_P = 0;
}

#define GU_NEED_POOLS(h) GU_REQUIRE(GU_HAS_POOLS(h), GU_ERR_STATE, "no node pools: call gu_mcts_init first")

extern "C" {

int gu_mcts_init(gu_handle h, int32_t max_sims)
{
    GU_ENTER(h);
    GU_NEED_GRID(h);
    GU_NEED_Q(h);
    GU_REQUIRE(max_sims >= 1 && max_sims <= GU_MCTS_MAX_SIMS, GU_ERR_INVALID, "max_sims %d out of range (1 .. %d)", max_sims, GU_MCTS_MAX_SIMS);
    const int32_t P = max_sims + 1;
    const size_t nodes = (size_t)h->N * (size_t)P;
    GU_HIP(hipStreamSynchronize(h->stream));
    if (!h->d_mcts_pool || h->mcts_P != P) {
        gu_mcts_free(h);
        GU_TRY(gu_tabular_fits(h, nodes * 72 + (size_t)h->N * 12, "tree-search node pools"));
        GU_HIP(hipMalloc(&h->d_mcts_pool, nodes * 64));
        GU_HIP(hipMalloc(&h->d_mcts_meta, nodes * 8));
        GU_HIP(hipMalloc(&h->d_mcts_nodes, (size_t)h->N * sizeof(int32_t)));
        GU_HIP(hipMalloc(&h->d_mcts_steps, (size_t)h->N * sizeof(int64_t)));
        h->mcts_P = P;
    }
    GU_HIP(hipMemsetAsync(h->d_mcts_pool, 0, nodes * 64, h->stream));  // (root rows of zeros until an iteration has been searched)
    GU_HIP(hipMemsetAsync(h->d_mcts_meta, 0xFF, nodes * 8, h->stream));
    GU_HIP(hipMemsetAsync(h->d_mcts_nodes, 0, (size_t)h->N * sizeof(int32_t), h->stream));
    GU_HIP(hipMemsetAsync(h->d_mcts_steps, 0, (size_t)h->N * sizeof(int64_t), h->stream));
    GU_HIP(hipStreamSynchronize(h->stream));
    return GU_OK;
}

int gu_mcts_set_tables(gu_handle h, int32_t C, const double *U, const double *B, const double *I)
{
    GU_ENTER(h);
    const double *v[] = {U, B, I};
    return gu_schedule_upload(h, h->d_mcts_tab, h->mcts_C, C, v, 3);
}

int gu_mcts_run(gu_handle h, int64_t T, int32_t M, int32_t H, int32_t D, double alpha, double gamma, uint32_t eps_q16, uint32_t eps_sim_q16,
                uint32_t flags)
{
    GU_ENTER(h);
    GU_NO_OVERLAY(h, "gu_mcts_run");
    GU_NEED_GRID(h);
    GU_NEED_Q(h);
    GU_NEED_POOLS(h);
    GU_REQUIRE(M >= 0 && M <= h->mcts_P - 1, GU_ERR_INVALID, "simulations %d out of range (0 .. %d, gu_mcts_init's max_sims)", M, h->mcts_P - 1);
    GU_REQUIRE(H >= 1 && H <= GU_MCTS_MAX_DEPTH, GU_ERR_INVALID, "tree depth %d out of range (1 .. %d)", H, GU_MCTS_MAX_DEPTH);
    GU_REQUIRE(D >= 0 && D <= GU_SEARCH_MAX_D, GU_ERR_INVALID, "depth %d out of range (0 .. %d)", D, GU_SEARCH_MAX_D);
    GU_REQUIRE(eps_sim_q16 <= 65536u, GU_ERR_INVALID, "eps_sim_q16 %u above 65536", eps_sim_q16);
    GU_REQUIRE(M == 0 || GU_HAS_MCTS_TABLES(h), GU_ERR_STATE, "no tree-search tables: call gu_mcts_set_tables first");
    GU_TRY(gu_tabular_check(h, "gu_mcts_run", T, -1, eps_q16, alpha, gamma, flags));
    GU_TRY(gu_move_budget(T, 1 + (int64_t)M * (H + D), "1 + M (H + D)"));  // per real step, at most
    if (T == 0) return GU_OK;
    return gu_launch_mcts(h, T, M, H, D, alpha, gamma, eps_q16, eps_sim_q16, flags);
}

static int gu_mcts_range(gu_engine *h, int64_t env0, int64_t n)
{
    GU_NEED_GRID(h);
    GU_NEED_Q(h);
    GU_NEED_POOLS(h);
    return gu_env_range(h, env0, n);
}

int gu_mcts_get(gu_handle h, int64_t env0, int64_t n, double *w, uint32_t *visits, int32_t *nodes, int64_t *sim_steps)
{
    GU_ENTER(h);
    GU_TRY(gu_mcts_range(h, env0, n));
    GU_HIP(hipStreamSynchronize(h->stream));
    if (!n) return GU_OK;
    // the root is node 0 of each env's pool: its w row at byte 0, its visits row at byte 32
    const size_t pitch = (size_t)h->mcts_P * 64;
    const uint8_t *root = h->d_mcts_pool + (size_t)env0 * pitch;
    if (w) GU_HIP(hipMemcpy2D(w, 32, root, pitch, 32, (size_t)n, hipMemcpyDeviceToHost));
    if (visits) GU_HIP(hipMemcpy2D(visits, 16, root + 32, pitch, 16, (size_t)n, hipMemcpyDeviceToHost));
    GU_TRY(gu_env_copy(h, hipMemcpyDeviceToHost, nodes, h->d_mcts_nodes, env0, n, 1, false));
    return gu_env_copy(h, hipMemcpyDeviceToHost, sim_steps, h->d_mcts_steps, env0, n, 1, false);
}

int gu_mcts_get_tree(gu_handle h, int64_t env0, int64_t n, int32_t *state, int32_t *parent, int32_t *child, uint32_t *visits, double *w,
                     int32_t *count)
{
    GU_ENTER(h);
    GU_TRY(gu_mcts_range(h, env0, n));
    GU_HIP(hipStreamSynchronize(h->stream));
    if (!n) return GU_OK;
    const size_t P = (size_t)h->mcts_P, k = (size_t)n * P;
    std::vector<uint8_t> pool(k * 64);
    std::vector<int32_t> meta(k * 2), cnt((size_t)n);
    GU_TRY(gu_env_copy(h, hipMemcpyDeviceToHost, pool.data(), h->d_mcts_pool, env0, n, P * 64, false));
    GU_TRY(gu_env_copy(h, hipMemcpyDeviceToHost, meta.data(), h->d_mcts_meta, env0, n, P * 2, false));
    GU_TRY(gu_env_copy(h, hipMemcpyDeviceToHost, cnt.data(), h->d_mcts_nodes, env0, n, 1, false));
    for (size_t e = 0; e < (size_t)n; ++e) {
        if (count) count[e] = cnt[e];
        for (size_t v = 0; v < P; ++v) {
            const size_t i = e * P + v;
            const bool live = (int64_t)v < (int64_t)cnt[e];
            const uint8_t *node = pool.data() + i * 64;
            if (state) state[i] = live ? meta[i * 2] : -1;
            if (parent) parent[i] = live ? meta[i * 2 + 1] : -1;
            for (size_t b = 0; b < 4; ++b) {
                if (w) w[i * 4 + b] = live ? reinterpret_cast<const double *>(node)[b] : 0.0;
                if (visits) visits[i * 4 + b] = live ? reinterpret_cast<const uint32_t *>(node + 32)[b] : 0u;
                if (child) child[i * 4 + b] = live ? reinterpret_cast<const int32_t *>(node + 48)[b] : -1;
            }
        }
    }
    return GU_OK;
}

}  // extern "C"
