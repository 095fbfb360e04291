// gu_fruit.hip -- fruit for gfx950: collectable rewards, each eaten once per episode (include/gu.h: gu_set_fruit; restated on the
// CPU by tests/_fruit_oracle.py).  The fruit is a third byte plane behind the engine's two cell planes (gu_engine::d_fruit_cell
// holds all three in one piece), three engine-wide values and one uint32 "eaten" mask per env (gu_engine::d_eaten).  Here are the
// entry points, the fruit step kernel (gu_step, gu_step_device), the fruit rollout kernel (gu_rollout) and the launch that clears
// the masks in front of a reset; the fruit learners are instantiations of gu_td_kernel (gu_td.hip, through TabLane's FRUIT parameter).
//
// One lane per env, like the calm kernels.  The three planes are staged in LDS where they fit 64 KiB (gu_lds_block(h, bs, 3)),
// else all three are read from L2.  Fruit never changes a move: the fruit byte of s' is read BESIDE the flags and the reward byte of
// s' (three independent reads behind one address), so the dependent chain of a step is as long as the calm kernel's.  The mask
// stays in a VGPR for the whole launch: one load at the start, one store at the end.  Plain stores, no schedule (GuPacer).
#include "gu_tabular.hpp"

#include <algorithm>
#include <vector>

// ------------------------------------------------------------------------------------
// single step: gu_step_kernel's rules (rejected actions, lazy auto-reset, done ballot, host copies) with the fruit of s'
// ------------------------------------------------------------------------------------
struct FruitStepArgs {
    const uint8_t *cell;  // [flags | reward | fruit]
    int32_t cell_bytes, W;
    uint64_t lut;
    const int32_t *actions;
    int32_t *pos, *reward, *done;
    uint32_t *episode;
    uint32_t *tcount;
    uint32_t *eaten;
    const int32_t *starts;
    uint32_t n_starts, seed_prefix, env_id0, values;
    int64_t N;
    uint32_t flags;
    GridSel gs;
    int32_t *host_obs, *host_reward, *host_done;
    uint32_t *host_seq;
    uint32_t seq;
    uint32_t *blocks_done;
    uint32_t *host_err;
    uint64_t *done_bits;
};

template <bool LDS>
__global__ void __launch_bounds__(GU_BLOCK) gu_fruit_step_kernel(const FruitStepArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const CellMap m = gu_stage_map<LDS>(a.cell, a.cell_bytes, smem, a.gs, 3);
    const uint8_t *fr = m.f + 2 * a.cell_bytes;
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int32_t d = 0;
    if (e < a.N) {
        const uint32_t raw = (uint32_t)a.actions[e];
        const uint32_t act = raw & 3u;
        int32_t s = a.pos[e], r;
        if (a.host_err && !GU_ACTION_OK(raw)) {  // (gu_step_kernel: this env does not step, eats nothing, and the host is told)
            __hip_atomic_store(a.host_err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            a.tcount[e] -= 1u;
            r = a.reward[e];
            d = a.done[e];
        } else {
            uint32_t eaten = a.eaten[e];
            if ((a.flags & GU_F_AUTO_RESET) && a.done[e]) {  // lazy `if done: env.reset()`: the fruit grows back
                const uint32_t ep = a.episode[e];
                s = a.starts[gu_rng_start_index(gu_rng_prefix(a.seed_prefix, a.env_id0 + (uint32_t)e), ep, a.n_starts)];
                a.episode[e] = ep + 1;
                eaten = 0u;
            }
            s = gu_move(s, m.f[s], act, gu_delta<LDS>(act, a.lut, a.W));
            r = m.r[s] + gu_fruit_eat(fr[s], a.values, eaten);
            d = (m.f[s] >> GU_CELL_TERM_BIT) & 1;
            a.pos[e] = s;
            a.reward[e] = r;
            a.done[e] = d;
            a.eaten[e] = eaten;
        }
        if (a.host_obs) a.host_obs[e] = s;
        if (a.host_reward) a.host_reward[e] = r;
        if (a.host_done) a.host_done[e] = d;
    }
    const uint64_t bits = __ballot(d != 0);
    if ((threadIdx.x & 63) == 0 && e < a.N) a.done_bits[e >> 6] = bits;
    if (a.host_seq) {  // the completion word, as gu_step_kernel publishes it
        __threadfence_system();
        __syncthreads();
        if (threadIdx.x == 0) {
            const uint32_t arrived = atomicAdd(a.blocks_done, 1u);
            if (arrived == gridDim.x - 1) {
                *a.blocks_done = 0u;
                __threadfence_system();
                __hip_atomic_store(a.host_seq, a.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
    }
}

int gu_fruit_launch_step(gu_engine *h, const int32_t *d_actions_row, uint32_t flags, int32_t *host_obs, int32_t *host_reward, int32_t *host_done,
                         uint32_t *host_seq, uint32_t seq, uint32_t *host_err)
{
    h->entry_table_ok = false;
    FruitStepArgs a{h->d_fruit_cell, h->cell_bytes, h->W, h->delta_lut, d_actions_row, h->pos(), h->reward(), h->done(), h->d_episode, h->d_tcount,
                    h->d_eaten, h->d_starts, (uint32_t)h->n_starts, h->seed_prefix, (uint32_t)h->env_id0, h->fruit_values, h->N, flags, gu_grid_sel(h),
                    host_obs, host_reward, host_done, host_seq, seq, h->d_blocks_done, host_err, h->d_done_bits};
    const int lds_bs = gu_lds_block(h, GU_BLOCK, 3);
    const dim3 grid(gu_blocks(h->N, GU_BLOCK)), block(GU_BLOCK);
    if (lds_bs) hipLaunchKernelGGL(gu_fruit_step_kernel<true>, grid, block, 3 * (size_t)h->cell_bytes, h->stream, a);
    else hipLaunchKernelGGL(gu_fruit_step_kernel<false>, grid, block, 0, h->stream, a);
    GU_HIP(hipGetLastError());
    h->steps_taken += 1;
    gu_tabular_drop_carry(h);
    return gu_trail_after_step(h, flags);
}

// ------------------------------------------------------------------------------------
// rollout: T steps per lane in one launch; the four policies with the calm kernels' action and sampling streams (0 and 2)
// ------------------------------------------------------------------------------------
struct FruitRolloutArgs {
    const uint8_t *cell;  // [flags | reward | fruit]
    const uint8_t *greedy;
    const uint4 *pi_thr;
    int32_t cell_bytes, W;
    uint64_t lut;
    int32_t *pos, *reward, *done;
    uint32_t *episode;
    const uint32_t *tcount;
    uint32_t *eaten;
    const int32_t *starts;
    const uint32_t *actions;  // GU_POLICY_STREAM: the packed stream, [ceil(T / 16)][N]
    int32_t *tr_obs, *tr_reward, *tr_done;  // GU_F_TRAJECTORY: [T][N] planes (else nullptr)
    int32_t *ret, *episodes_fin;            // GU_F_STATS (else nullptr)
    uint64_t *done_bits;
    uint32_t n_starts, seed_prefix, env_id0, values;
    uint64_t steps_taken;
    int64_t N, T;
    int32_t auto_reset;
    GridSel gs;
};

// Auto-reset, rows and statistics are launch-uniform tests on the arguments.  The step count is 64 bits wide and streams 0 and 2 are
// re-keyed in the step that crosses a multiple of 2^32, so no launch needs another form.
template <int POLICY, bool LDS>
__global__ void __launch_bounds__(GU_BLOCK) gu_fruit_rollout_kernel(const FruitRolloutArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const CellMap m = gu_stage_map<LDS>(a.cell, a.cell_bytes, smem, a.gs, 3);
    const uint8_t *fr = m.f + 2 * a.cell_bytes;
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int32_t d = 0;
    if (e < a.N) {
        const uint32_t env = a.env_id0 + (uint32_t)e;
        int32_t s = a.pos[e], r = a.reward[e];
        d = a.done[e];
        uint32_t ep = a.episode[e], eaten = a.eaten[e];
        uint64_t t = a.steps_taken + (uint64_t)(int64_t)(int32_t)a.tcount[e];
        const uint32_t start_prefix = gu_rng_prefix(a.seed_prefix, env);  // stream 1: no epoch
        // streams 0 and 2 share the prefix of the step count's epoch: re-keyed in the step that crosses a multiple of 2^32
        uint32_t prefix = gu_rng_prefix(gu_rng_seed_prefix_epoch(a.seed_prefix, (uint32_t)(t >> 32)), env);
        uint32_t word = 0;  // uniform: the stream-0 word of steps t & ~15 ..; stream: the packed word; sample: the stream-2 word of step t
        if (POLICY == GU_POLICY_UNIFORM) word = gu_rng_word(prefix, GU_RNG_STREAM_ACTION, (uint32_t)t >> 4);
        if (POLICY == GU_POLICY_SAMPLE) word = gu_rng_sample_word(prefix, (uint32_t)t);
        int32_t ret = 0, fin = 0;
        for (int64_t i = 0; i < a.T; ++i) {
            if (a.auto_reset && d) {  // lazy `if done: env.reset()`: the fruit grows back
                s = a.starts[gu_rng_start_index(start_prefix, ep, a.n_starts)];
                ++ep;
                d = 0;
                eaten = 0u;
            }
            uint32_t act;
            if (POLICY == GU_POLICY_UNIFORM) {
                act = (word >> (2u * ((uint32_t)t & 15u))) & 3u;
            } else if (POLICY == GU_POLICY_STREAM) {
                if ((i & 15) == 0) word = a.actions[(i >> 4) * a.N + e];
                act = (word >> (2u * (uint32_t)(i & 15))) & 3u;
            } else if (POLICY == GU_POLICY_GREEDY) {
                act = a.greedy[s];
            } else {
                act = gu_sample_action(word, a.pi_thr[s]);
            }
            s = gu_move(s, m.f[s], act, gu_delta<LDS>(act, a.lut, a.W));
            // three reads behind the one address s': flags, reward byte, fruit byte
            r = m.r[s] + gu_fruit_eat(fr[s], a.values, eaten);
            d = (m.f[s] >> GU_CELL_TERM_BIT) & 1;
            ++t;
            if (((uint32_t)t & 15u) == 0u) {  // the next sixteen steps' words (and, once in 2^32 steps, the next epoch's prefix)
                if ((uint32_t)t == 0u) prefix = gu_rng_prefix(gu_rng_seed_prefix_epoch(a.seed_prefix, (uint32_t)(t >> 32)), env);
                if (POLICY == GU_POLICY_UNIFORM) word = gu_rng_word(prefix, GU_RNG_STREAM_ACTION, (uint32_t)t >> 4);
                if (POLICY == GU_POLICY_SAMPLE) word = gu_rng_word(prefix, GU_RNG_STREAM_SAMPLE, (uint32_t)t >> 4);
            } else if (POLICY == GU_POLICY_SAMPLE) {
                word = gu_rng_sample_next(word);
            }
            if (a.tr_obs) {
                const int64_t row = i * a.N + e;
                a.tr_obs[row] = s;
                a.tr_reward[row] = r;
                a.tr_done[row] = d;
            }
            ret += r;
            fin += d;
        }
        a.pos[e] = s;
        a.reward[e] = r;
        a.done[e] = d;
        a.episode[e] = ep;
        a.eaten[e] = eaten;
        if (a.ret) {
            a.ret[e] = ret;
            a.episodes_fin[e] = fin;
        }
    }
    const uint64_t bits = __ballot(d != 0);
    if ((threadIdx.x & 63) == 0 && e < a.N) a.done_bits[e >> 6] = bits;
}

// gu_launch_rollout hands a launch over here while fruit is set: `r` is what it has filled in (state, tables, rows, streams)
void gu_fruit_launch_rollout(gu_engine *h, const GuRolloutPlan &p, const RolloutArgs &r)
{
    FruitRolloutArgs a{};
    a.cell = h->d_fruit_cell, a.cell_bytes = h->cell_bytes, a.W = h->W, a.lut = h->delta_lut, a.gs = r.gs, a.values = h->fruit_values;
    a.greedy = r.greedy, a.pi_thr = r.pi_thr, a.actions = r.actions;
    a.pos = r.pos, a.reward = r.reward, a.done = r.done, a.episode = r.episode, a.tcount = r.tcount, a.done_bits = r.done_bits, a.eaten = h->d_eaten;
    a.starts = r.starts, a.n_starts = r.n_starts, a.env_id0 = r.env_id0, a.seed_prefix = h->seed_prefix;
    a.tr_obs = p.traj ? r.tr_obs : nullptr, a.tr_reward = p.traj ? r.tr_reward : nullptr, a.tr_done = p.traj ? r.tr_done : nullptr;
    a.ret = p.stats ? r.ret : nullptr, a.episodes_fin = p.stats ? r.episodes_fin : nullptr;
    a.N = h->N, a.T = r.T, a.steps_taken = h->steps_taken, a.auto_reset = p.auto_mode ? 1 : 0;
    gu_pick<3, 2, 1, 0>(p.policy, [&](auto policy_c) {
        gu_pick<0, 1>(p.lds != 0, [&](auto lds_c) {
            constexpr int POLICY = decltype(policy_c)::value;
            constexpr bool LDS = decltype(lds_c)::value != 0;
            gu_lds_launch<gu_fruit_rollout_kernel<POLICY, LDS>, false>(h, p.blocks, p.block, p.lds, a);
        });
    });
}

// ------------------------------------------------------------------------------------
// resets: gu_reset and gu_reset_done clear the masks of the envs they reset, in a launch of its own IN FRONT of gu_reset_kernel (it
// reads the done flags that the reset is about to clear); that kernel is untouched and engines without fruit never get here
// ------------------------------------------------------------------------------------
__global__ void __launch_bounds__(GU_BLOCK) gu_fruit_reset_kernel(uint32_t *__restrict__ eaten, const uint8_t *__restrict__ mask, const int32_t *__restrict__ done,
                                                                   int32_t only_done, int64_t N)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= N) return;
    bool take = !mask || mask[e];
    if (only_done && !done[e]) take = false;
    if (take) eaten[e] = 0u;
}

int gu_fruit_before_reset(gu_engine *h, const uint8_t *d_mask, bool only_done)
{
    if (!h->n_fruit) return GU_OK;
    hipLaunchKernelGGL(gu_fruit_reset_kernel, dim3(gu_blocks(h->N, GU_BLOCK)), dim3(GU_BLOCK), 0, h->stream, h->d_eaten, d_mask, h->done(), only_done ? 1 : 0, h->N);
    GU_HIP(hipGetLastError());
    return GU_OK;
}

void gu_fruit_free(gu_engine *h)
{
    gu_release(h->d_fruit_cell, h->d_eaten);
    h->n_fruit = 0;
    h->fruit_values = 0;
    std::fill(h->fruit_value, h->fruit_value + 3, 0);
}

// ------------------------------------------------------------------------------------
// entry points
// ------------------------------------------------------------------------------------
extern "C" {

int gu_set_fruit(gu_handle h, const uint8_t *fruit, const int32_t value[3])
{
    GU_ENTER(h);
    GU_NEED_GRID(h);
    GU_REQUIRE(h->n_grids == 1, GU_ERR_UNSUPPORTED, "fruit is a property of a single-grid engine (this one holds %d grids)", h->n_grids);
    GU_REQUIRE(!h->d_wind_cell, GU_ERR_UNSUPPORTED, "fruit and wind exclude each other: the engine has wind set (gu_set_wind; NULL calms it again)");
    GU_REQUIRE(!h->n_doors, GU_ERR_UNSUPPORTED, "fruit and doors exclude each other: the engine has doors set (gu_set_doors; NULL takes them away again)");
    GU_REQUIRE(!h->trail_cap, GU_ERR_UNSUPPORTED, "fruit and the agent trail exclude each other: the trail is on (gu_trail_enable(h, 0) turns it off)");
    int32_t F = 0;
    std::vector<uint8_t> flags;
    if (fruit) {
        GU_REQUIRE(value != nullptr, GU_ERR_INVALID, "value is NULL");
        // Each value in -16 .. 16 keeps a launch's int32 reward sum in range at T <= 1e8.  A step ends on ONE cell, so it eats at most
        // one fruit; a fruit is eaten at most once per episode and cannot lie on a terminal cell, so the step that eats it pays the
        // cell's -1 beside it (|r| <= 17) and an episode that eats k fruits has at least k + 1 steps, the last one a terminal step
        // of |r| <= 10.  No step pays more than 17 in absolute value, and 1e8 * 17 = 1.7e9 < 2^31.  (Reward planes that put +-10 on a
        // cell that is not terminal could take a step to 26: 2^31 / 26 = 8.2e7 steps are safe for those.)
        for (int k = 0; k < 3; ++k) GU_REQUIRE(value[k] >= -16 && value[k] <= 16, GU_ERR_INVALID, "value[%d] = %d outside -16 .. 16", k, value[k]);
        flags.resize((size_t)h->S);
        GU_HIP(hipStreamSynchronize(h->stream));
        GU_HIP(hipMemcpy(flags.data(), h->d_cell, (size_t)h->S, hipMemcpyDeviceToHost));
        uint32_t slots = 0;
        for (int32_t s = 0; s < h->S; ++s) {
            const uint32_t c = fruit[s], kind = (c >> 5) & 3u, slot = c & 31u;
            if (!c) continue;
            GU_REQUIRE(!(c & 0x80u) && kind != 0u, GU_ERR_INVALID, "fruit byte 0x%02x of cell %d: bit 7 must be zero, and kind 0 means the whole byte is zero", c, s);
            GU_REQUIRE(F < 32, GU_ERR_INVALID, "more than 32 fruits");
            GU_REQUIRE(!(flags[s] & (GU_CELL_WALL | GU_CELL_TERM)), GU_ERR_INVALID, "fruit on cell %d, which is a wall or a goal or lava cell", s);
            GU_REQUIRE(!((slots >> slot) & 1u), GU_ERR_INVALID, "slot %u is used twice (second at cell %d)", slot, s);
            slots |= 1u << slot;
            ++F;
        }
        GU_REQUIRE(F >= 1, GU_ERR_INVALID, "no fruit in the plane (NULL takes the fruit away)");
        GU_REQUIRE(slots == (F == 32 ? ~0u : (1u << F) - 1u), GU_ERR_INVALID, "the %d fruits must use the slots 0 .. %d, each once (slot mask 0x%08x)", F, F - 1, slots);
    }
    GU_HIP(hipStreamSynchronize(h->stream));
    const size_t cb = (size_t)h->cell_bytes;
    if (fruit) {  // what can fail comes first: a refused call leaves the engine as it was
        if (!h->d_eaten) GU_HIP(hipMalloc(&h->d_eaten, (size_t)h->N * sizeof(uint32_t)));
        if (!h->d_fruit_cell) {
            GU_HIP(hipMalloc(&h->d_fruit_cell, 3 * cb));
            GU_HIP(hipMemcpy(h->d_fruit_cell, h->d_cell, 2 * cb, hipMemcpyDeviceToDevice));
        }
    }
    gu_tabular_drop_carry(h);  // another reward rule: what the learners carry belongs to the old one
    h->entry_table_ok = false;
    if (h->graph_exec) {  // (a captured step graph holds the launches without fruit)
        (void)hipGraphExecDestroy(h->graph_exec);
        h->graph_exec = nullptr;
    }
    gu_td_rows_changed(h, F);  // Q tables of another row count go (S << F rows: gu_td_run)
    if (!fruit) {
        gu_fruit_free(h);
        return GU_OK;
    }
    std::vector<uint8_t> plane(cb, 0);  // (the padding behind cell S - 1 bears nothing)
    std::copy(fruit, fruit + h->S, plane.begin());
    GU_HIP(hipMemcpy(h->d_fruit_cell + 2 * cb, plane.data(), cb, hipMemcpyHostToDevice));
    GU_HIP(hipMemset(h->d_eaten, 0, (size_t)h->N * sizeof(uint32_t)));
    h->n_fruit = F;
    h->fruit_values = 0;
    for (int k = 0; k < 3; ++k) {  // four int8 bytes, byte 0 (kind 0: no fruit) zero
        h->fruit_value[k] = value[k];
        h->fruit_values |= (uint32_t)(uint8_t)(int8_t)value[k] << (8 * (k + 1));
    }
    return GU_OK;
}

int gu_get_fruit(gu_handle h, uint8_t *fruit, int32_t value[3], int32_t *n_fruit)
{
    GU_ENTER(h);
    GU_NEED_GRID(h);
    if (n_fruit) *n_fruit = h->n_fruit;
    if (value) std::copy(h->fruit_value, h->fruit_value + 3, value);
    if (fruit) {
        if (h->n_fruit) {
            GU_HIP(hipStreamSynchronize(h->stream));
            GU_HIP(hipMemcpy(fruit, h->d_fruit_cell + 2 * (size_t)h->cell_bytes, (size_t)h->S, hipMemcpyDeviceToHost));
        } else {
            std::fill(fruit, fruit + h->S, (uint8_t)0);
        }
    }
    return GU_OK;
}

static int gu_fruit_range(gu_engine *h, int64_t env0, int64_t n, const void *eaten)
{
    GU_NEED_GRID(h);
    GU_REQUIRE(h->n_fruit, GU_ERR_STATE, "no fruit set: call gu_set_fruit first");
    GU_REQUIRE(eaten != nullptr, GU_ERR_INVALID, "eaten is NULL");
    return gu_env_range(h, env0, n);
}

int gu_get_fruit_state(gu_handle h, int64_t env0, int64_t n, uint32_t *eaten)
{
    GU_ENTER(h);
    GU_TRY(gu_fruit_range(h, env0, n, eaten));
    return gu_env_copy(h, hipMemcpyDeviceToHost, eaten, h->d_eaten, env0, n, 1);
}

int gu_set_fruit_state(gu_handle h, int64_t env0, int64_t n, const uint32_t *eaten)
{
    GU_ENTER(h);
    GU_TRY(gu_fruit_range(h, env0, n, eaten));
    if (h->n_fruit < 32)
        for (int64_t i = 0; i < n; ++i)
            GU_REQUIRE((eaten[i] >> h->n_fruit) == 0u, GU_ERR_INVALID, "eaten[%lld] = 0x%08x has a bit at or above the %d fruits", (long long)i, eaten[i], h->n_fruit);
    gu_tabular_drop_carry(h);  // (a carried SARSA action was drawn on the row of the old mask)
    h->entry_table_ok = false;
    return gu_env_copy(h, hipMemcpyHostToDevice, eaten, h->d_eaten, env0, n, 1);
}

}  // extern "C"
