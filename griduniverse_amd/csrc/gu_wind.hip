// gu_wind.hip -- wind for gfx950: per-cell pushes with gusts (include/gu.h: gu_set_wind; restated on the CPU by tests/_wind_oracle.py).
// The wind is a third byte plane behind the engine's two cell planes (gu_engine::d_wind_cell holds all three in one piece), and a
// step is the engine's move followed by up to four more moves in the wind's direction (gu_map.hpp: gu_wind_push).  Here are the
// entry points, the windy step kernel (gu_step, gu_step_device) and the windy rollout kernel (gu_rollout); the windy learners are
// instantiations of gu_td_kernel (gu_td.hip, through TabLane's WIND parameter).
//
// One lane per env, like the calm kernels.  The three planes are staged in LDS where they fit 64 KiB (gu_lds_block(h, bs, 3)),
// else all three are read from L2.  A windy step is a chain of 2 + k dependent plane reads (the wind byte and the flags of the
// cell left, the flags behind every push) instead of one, so these kernels are bound by that latency, not by the store stream:
// they keep no schedule (GuPacer) and do not depend on where the trajectory buffer lies.
#include "gu_tabular.hpp"

#include <algorithm>
#include <vector>

// ------------------------------------------------------------------------------------
// one windy move: the wind of the cell left, the gust on the stream-9 word of step t, the action, the pushes
// ------------------------------------------------------------------------------------
template <bool LDS, bool GUST>
__device__ __forceinline__ int32_t gu_wind_move(const CellMap &m, const uint8_t *wd, int32_t s, uint32_t act, uint32_t prefix, uint64_t t, uint32_t gust_q16,
                                                uint64_t lut, int32_t W)
{
    const uint32_t c = wd[s];
    uint32_t k = GU_WIND_STRENGTH(c);
    // (hashed only where some lane of the wave stands in wind: one ballot and a scalar branch)
    if (GUST && __builtin_amdgcn_ballot_w64(k > 0u) != 0ull) k = gu_wind_gust(k, gu_rng_word(prefix, GU_RNG_STREAM_WIND, (uint32_t)t), gust_q16);
    s = gu_move(s, m.f[s], act, gu_delta<LDS>(act, lut, W));
    return gu_wind_push<LDS>(m.f, s, c, k, lut, W);
}

// ------------------------------------------------------------------------------------
// single step: gu_step_kernel's rules (rejected actions, lazy auto-reset, done ballot, host copies) around the windy move
// ------------------------------------------------------------------------------------
struct WindStepArgs {
    const uint8_t *cell;  // [flags | reward | wind]
    int32_t cell_bytes, W;
    uint64_t lut;
    const int32_t *actions;
    int32_t *pos, *reward, *done;
    uint32_t *episode;
    uint32_t *tcount;
    const int32_t *starts;
    uint32_t n_starts, seed_prefix, env_id0, gust_q16;
    uint64_t steps_taken;
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

template <bool LDS, bool GUST>
__global__ void __launch_bounds__(GU_BLOCK) gu_wind_step_kernel(const WindStepArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const CellMap m = gu_stage_map<LDS>(a.cell, a.cell_bytes, smem, a.gs, 3);
    const uint8_t *wd = m.f + 2 * a.cell_bytes;
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = e < a.N;
    // the windy move runs on every lane of the wave (its loops are wave-uniform): lanes past the batch stand on cell 0 with an
    // action that is skipped below
    int32_t s = 0, r = 0, d = 0;
    uint32_t raw = 0;
    bool ok = false;
    uint32_t prefix = 0;
    uint64_t t = 0;
    if (live) {
        raw = (uint32_t)a.actions[e];
        s = a.pos[e];
        ok = !a.host_err || GU_ACTION_OK(raw);
        if (!ok) {  // (gu_step_kernel: this env does not step, draws nothing, and the host is told)
            __hip_atomic_store(a.host_err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            a.tcount[e] -= 1u;
            r = a.reward[e];
            d = a.done[e];
        } else {
            const uint32_t env = a.env_id0 + (uint32_t)e;
            t = a.steps_taken + (uint64_t)(int64_t)(int32_t)a.tcount[e];
            if (GUST) prefix = gu_rng_prefix(gu_rng_seed_prefix_epoch(a.seed_prefix, (uint32_t)(t >> 32)), env);
            if ((a.flags & GU_F_AUTO_RESET) && a.done[e]) {
                const uint32_t ep = a.episode[e];
                s = a.starts[gu_rng_start_index(gu_rng_prefix(a.seed_prefix, env), ep, a.n_starts)];
                a.episode[e] = ep + 1;
            }
        }
    }
    {
        // (a lane that does not step goes through the move on cell 0 and throws the result away)
        const int32_t s2 = gu_wind_move<LDS, GUST>(m, wd, (live && ok) ? s : 0, raw & 3u, prefix, t, a.gust_q16, a.lut, a.W);
        if (live && ok) {
            s = s2;
            r = m.r[s];
            d = (m.f[s] >> GU_CELL_TERM_BIT) & 1;
            a.pos[e] = s;
            a.reward[e] = r;
            a.done[e] = d;
        }
    }
    if (live) {
        if (a.host_obs) a.host_obs[e] = s;
        if (a.host_reward) a.host_reward[e] = r;
        if (a.host_done) a.host_done[e] = d;
    }
    const uint64_t bits = __ballot(d != 0);
    if ((threadIdx.x & 63) == 0 && live) a.done_bits[e >> 6] = bits;
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

int gu_wind_launch_step(gu_engine *h, const int32_t *d_actions_row, uint32_t flags, int32_t *host_obs, int32_t *host_reward, int32_t *host_done,
                        uint32_t *host_seq, uint32_t seq, uint32_t *host_err)
{
    h->entry_table_ok = false;
    WindStepArgs a{h->d_wind_cell, h->cell_bytes, h->W, h->delta_lut, d_actions_row, h->pos(), h->reward(), h->done(), h->d_episode, h->d_tcount,
                   h->d_starts, (uint32_t)h->n_starts, h->seed_prefix, (uint32_t)h->env_id0, h->gust_q16, h->steps_taken, h->N, flags, gu_grid_sel(h),
                   host_obs, host_reward, host_done, host_seq, seq, h->d_blocks_done, host_err, h->d_done_bits};
    const int lds_bs = gu_lds_block(h, GU_BLOCK, 3);
    const dim3 grid(gu_blocks(h->N, GU_BLOCK)), block(GU_BLOCK);
    const size_t lds = lds_bs ? 3 * (size_t)h->cell_bytes : 0;
    if (lds_bs && h->gust_q16) hipLaunchKernelGGL((gu_wind_step_kernel<true, true>), grid, block, lds, h->stream, a);
    else if (lds_bs) hipLaunchKernelGGL((gu_wind_step_kernel<true, false>), grid, block, lds, h->stream, a);
    else if (h->gust_q16) hipLaunchKernelGGL((gu_wind_step_kernel<false, true>), grid, block, 0, h->stream, a);
    else hipLaunchKernelGGL((gu_wind_step_kernel<false, false>), grid, block, 0, h->stream, a);
    GU_HIP(hipGetLastError());
    h->steps_taken += 1;
    gu_tabular_drop_carry(h);
    return gu_trail_after_step(h, flags);
}

// ------------------------------------------------------------------------------------
// rollout: T windy steps per lane in one launch; the four policies with the calm kernels' action and sampling streams (0 and 2)
// ------------------------------------------------------------------------------------
struct WindRolloutArgs {
    const uint8_t *cell;  // [flags | reward | wind]
    const uint8_t *greedy;
    const uint4 *pi_thr;
    int32_t cell_bytes, W;
    uint64_t lut;
    int32_t *pos, *reward, *done;
    uint32_t *episode;
    const uint32_t *tcount;
    const int32_t *starts;
    const uint32_t *actions;  // GU_POLICY_STREAM: the packed stream, [ceil(T / 16)][N]
    int32_t *tr_obs, *tr_reward, *tr_done;  // GU_F_TRAJECTORY: [T][N] planes (else nullptr)
    int32_t *ret, *episodes_fin;            // GU_F_STATS (else nullptr)
    uint64_t *done_bits;
    uint32_t n_starts, seed_prefix, env_id0, gust_q16;
    uint64_t steps_taken;
    int64_t N, T;
    int32_t auto_reset;
    GridSel gs;
};

// GUST is a template parameter: the calm-gust instantiations carry no stream-9 hash.  Auto-reset, rows and statistics are
// launch-uniform tests on the arguments (a windy step is a chain of dependent plane reads: the tests hide behind it).
template <int POLICY, bool LDS, bool GUST>
__global__ void __launch_bounds__(GU_BLOCK) gu_wind_rollout_kernel(const WindRolloutArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const CellMap m = gu_stage_map<LDS>(a.cell, a.cell_bytes, smem, a.gs, 3);
    const uint8_t *wd = m.f + 2 * a.cell_bytes;
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = e < a.N;
    // lanes past the batch run the loop too (the pushes and the gust hash are wave-uniform), on cell 0, and store nothing
    const int64_t el = live ? e : 0;
    const uint32_t env = a.env_id0 + (uint32_t)el;
    int32_t s = a.pos[el], r = a.reward[el], d = a.done[el];
    uint32_t ep = a.episode[el];
    uint64_t t = a.steps_taken + (uint64_t)(int64_t)(int32_t)a.tcount[el];
    const uint32_t start_prefix = gu_rng_prefix(a.seed_prefix, env);  // stream 1: no epoch
    // streams 0, 2 and 9 share the prefix of the step count's epoch: re-keyed in the step that crosses a multiple of 2^32
    uint32_t prefix = gu_rng_prefix(gu_rng_seed_prefix_epoch(a.seed_prefix, (uint32_t)(t >> 32)), env);
    uint32_t word = 0;  // uniform: the stream-0 word of steps t & ~15 ..; stream: the packed word; sample: the stream-2 word of step t
    if (POLICY == GU_POLICY_UNIFORM) word = gu_rng_word(prefix, GU_RNG_STREAM_ACTION, (uint32_t)t >> 4);
    if (POLICY == GU_POLICY_SAMPLE) word = gu_rng_sample_word(prefix, (uint32_t)t);
    int32_t ret = 0, fin = 0;
    for (int64_t i = 0; i < a.T; ++i) {
        if (a.auto_reset && d) {  // lazy `if done: env.reset()`
            s = a.starts[gu_rng_start_index(start_prefix, ep, a.n_starts)];
            ++ep;
            d = 0;
        }
        uint32_t act;
        if (POLICY == GU_POLICY_UNIFORM) {
            act = (word >> (2u * ((uint32_t)t & 15u))) & 3u;
        } else if (POLICY == GU_POLICY_STREAM) {
            if ((i & 15) == 0) word = a.actions[(i >> 4) * a.N + el];
            act = (word >> (2u * (uint32_t)(i & 15))) & 3u;
        } else if (POLICY == GU_POLICY_GREEDY) {
            act = a.greedy[s];
        } else {
            act = gu_sample_action(word, a.pi_thr[s]);
        }
        s = gu_wind_move<LDS, GUST>(m, wd, s, act, prefix, t, a.gust_q16, a.lut, a.W);
        r = m.r[s];
        d = (m.f[s] >> GU_CELL_TERM_BIT) & 1;
        ++t;
        if (((uint32_t)t & 15u) == 0u) {  // the next sixteen steps' words (and, once in 2^32 steps, the next epoch's prefix)
            if ((uint32_t)t == 0u) prefix = gu_rng_prefix(gu_rng_seed_prefix_epoch(a.seed_prefix, (uint32_t)(t >> 32)), env);
            if (POLICY == GU_POLICY_UNIFORM) word = gu_rng_word(prefix, GU_RNG_STREAM_ACTION, (uint32_t)t >> 4);
            if (POLICY == GU_POLICY_SAMPLE) word = gu_rng_word(prefix, GU_RNG_STREAM_SAMPLE, (uint32_t)t >> 4);
        } else if (POLICY == GU_POLICY_SAMPLE) {
            word = gu_rng_sample_next(word);
        }
        if (a.tr_obs && live) {
            const int64_t row = i * a.N + e;
            a.tr_obs[row] = s;
            a.tr_reward[row] = r;
            a.tr_done[row] = d;
        }
        ret += r;
        fin += d;
    }
    if (live) {
        a.pos[e] = s;
        a.reward[e] = r;
        a.done[e] = d;
        a.episode[e] = ep;
        if (a.ret) {
            a.ret[e] = ret;
            a.episodes_fin[e] = fin;
        }
    }
    const uint64_t bits = __ballot(live && d != 0);
    if ((threadIdx.x & 63) == 0 && live) a.done_bits[e >> 6] = bits;
}

// gu_launch_rollout hands a launch over here while wind is set: `r` is what it has filled in (state, tables, rows, streams)
// (the lists run backwards so that the kernels keep their order in the code object: an unchanged binary is how a change here is checked)
void gu_wind_launch_rollout(gu_engine *h, const GuRolloutPlan &p, const RolloutArgs &r)
{
    WindRolloutArgs a{};
    a.cell = h->d_wind_cell, a.cell_bytes = h->cell_bytes, a.W = h->W, a.lut = h->delta_lut, a.gs = r.gs, a.gust_q16 = h->gust_q16;
    a.greedy = r.greedy, a.pi_thr = r.pi_thr, a.actions = r.actions;
    a.pos = r.pos, a.reward = r.reward, a.done = r.done, a.episode = r.episode, a.tcount = r.tcount, a.done_bits = r.done_bits;
    a.starts = r.starts, a.n_starts = r.n_starts, a.env_id0 = r.env_id0, a.seed_prefix = h->seed_prefix;
    a.tr_obs = p.traj ? r.tr_obs : nullptr, a.tr_reward = p.traj ? r.tr_reward : nullptr, a.tr_done = p.traj ? r.tr_done : nullptr;
    a.ret = p.stats ? r.ret : nullptr, a.episodes_fin = p.stats ? r.episodes_fin : nullptr;
    a.N = h->N, a.T = r.T, a.steps_taken = h->steps_taken, a.auto_reset = p.auto_mode ? 1 : 0;
    gu_pick<3, 2, 1, 0>(p.policy, [&](auto policy_c) {
        gu_pick<0, 1>(p.lds != 0, [&](auto lds_c) {
            gu_pick<0, 1>(h->gust_q16 != 0, [&](auto gust_c) {
                constexpr int POLICY = decltype(policy_c)::value;
                constexpr bool LDS = decltype(lds_c)::value != 0, GUST = decltype(gust_c)::value != 0;
                gu_lds_launch<gu_wind_rollout_kernel<POLICY, LDS, GUST>, false>(h, p.blocks, p.block, p.lds, a);
            });
        });
    });
}

void gu_wind_free(gu_engine *h)
{
    gu_release(h->d_wind_cell);
    h->gust_q16 = 0;
}

// ------------------------------------------------------------------------------------
// entry points
// ------------------------------------------------------------------------------------
extern "C" {

int gu_set_wind(gu_handle h, const uint8_t *wind, uint32_t gust_q16)
{
    GU_ENTER(h);
    GU_NEED_GRID(h);
    GU_REQUIRE(h->n_grids == 1, GU_ERR_UNSUPPORTED, "wind is a property of a single-grid engine (this one holds %d grids)", h->n_grids);
    GU_REQUIRE(!h->trail_cap, GU_ERR_UNSUPPORTED, "wind and the agent trail exclude each other: the trail is on (gu_trail_enable(h, 0) turns it off)");
    GU_REQUIRE(!h->n_fruit, GU_ERR_UNSUPPORTED, "wind and fruit exclude each other: the engine has fruit set (gu_set_fruit; NULL takes it away again)");
    GU_REQUIRE(!h->n_doors, GU_ERR_UNSUPPORTED, "wind and doors exclude each other: the engine has doors set (gu_set_doors; NULL takes them away again)");
    GU_REQUIRE(gust_q16 <= 65536u, GU_ERR_INVALID, "gust_q16 %u above 65536", gust_q16);
    if (wind)
        for (int32_t s = 0; s < h->S; ++s)
            GU_REQUIRE((wind[s] & 0xF0u) == 0, GU_ERR_INVALID, "wind byte 0x%02x of cell %d: bits 4 .. 7 must be zero", wind[s], s);
    GU_HIP(hipStreamSynchronize(h->stream));
    gu_tabular_drop_carry(h);  // another move rule: what the learners carry belongs to the old one
    h->entry_table_ok = false;
    if (h->graph_exec) {  // (a captured step graph holds the calm launches)
        (void)hipGraphExecDestroy(h->graph_exec);
        h->graph_exec = nullptr;
    }
    if (!wind) {
        gu_wind_free(h);
        return GU_OK;
    }
    const size_t cb = (size_t)h->cell_bytes;
    if (!h->d_wind_cell) {
        GU_HIP(hipMalloc(&h->d_wind_cell, 3 * cb));
        GU_HIP(hipMemcpy(h->d_wind_cell, h->d_cell, 2 * cb, hipMemcpyDeviceToDevice));
    }
    std::vector<uint8_t> plane(cb, 0);  // (the padding behind cell S - 1 is calm)
    std::copy(wind, wind + h->S, plane.begin());
    GU_HIP(hipMemcpy(h->d_wind_cell + 2 * cb, plane.data(), cb, hipMemcpyHostToDevice));
    h->gust_q16 = gust_q16;
    return GU_OK;
}

int gu_get_wind(gu_handle h, uint8_t *wind, uint32_t *gust_q16, int32_t *present)
{
    GU_ENTER(h);
    GU_NEED_GRID(h);
    if (present) *present = h->d_wind_cell ? 1 : 0;
    if (gust_q16) *gust_q16 = h->d_wind_cell ? h->gust_q16 : 0u;
    if (wind) {
        if (h->d_wind_cell) {
            GU_HIP(hipStreamSynchronize(h->stream));
            GU_HIP(hipMemcpy(wind, h->d_wind_cell + 2 * (size_t)h->cell_bytes, (size_t)h->S, hipMemcpyDeviceToHost));
        } else {
            std::fill(wind, wind + h->S, (uint8_t)0);
        }
    }
    return GU_OK;
}

}  // extern "C"
