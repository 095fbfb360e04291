// gu_doors.hip -- doors, keys and levers for gfx950: the first feature whose move rule depends on the lane's own bits of state
// (include/gu.h: gu_set_doors; restated on the CPU by tests/_doors_oracle.py).  The doors are a third byte plane behind the engine's
// two cell planes (gu_engine::d_door_cell holds all three in one piece) and one uint32 mask of open slots per env (gu_engine::d_open).
// Here are the entry points, the door step kernel (gu_step, gu_step_device), the door rollout kernel (gu_rollout) and the launch that
// clears the masks in front of a reset; the door learners are instantiations of gu_td_kernel (gu_td.hip, through TabLane's DOORS
// parameter).
//
// THE GATE, decided on purpose.  The rule reads door[c] after flags[s] has produced the candidate c: taken literally that is a second
// dependent LDS read in front of the reads at s', in a loop whose speed is its dependent chain.  A derived 16-bit plane that names,
// at s, the slot guarding each direction would take the gate off the chain at five bytes per cell instead of three (grids between
// 64 KiB / 5 and 64 KiB / 3 cells would fall to L2).  The rollout kernel here does neither.  It CARRIES the flags and the reward
// byte of the cell it stands on in VGPRs and reads all three bytes of the CANDIDATE -- flags[c], reward[c], door[c], three
// independent reads behind one address, as fruit reads s'.  Open or no door: the candidate's bytes become the carried ones.  Closed:
// the carried ones stay (they are the bytes of s' = s, which is what a bump pays).  So a step has ONE round of LDS reads on its
// chain, the calm kernel's count, the plane stays the byte the interface takes, and the LDS limit stays fruit's (three planes).  The
// cost is two VGPRs and three selects per step, and one more round of reads behind a lazy reset (the start cell's bytes).  The
// derived-plane form was not built, so there is no measured difference between the two to quote; what was measured is this kernel
// beside the fruit kernel, which has no gate at all (tools/doors_rate.py, profiles/doors_rate.json: 0.98 .. 1.08 of its rate).  The
// learners' lane (TabLane::move, gu_tabular.hpp) gates the same way, with the bytes of s read beside each other instead of carried.
// The step kernel takes one step per launch and reads door[c] behind the candidate, as the rule is written.
//
// One lane per env.  The mask stays in a VGPR for the whole launch: one load at the start, one store at the end.  Plain stores, no
// schedule (GuPacer).
#include "gu_tabular.hpp"

#include <algorithm>
#include <vector>

// ------------------------------------------------------------------------------------
// single step: gu_step_kernel's rules (rejected actions, lazy auto-reset, done ballot, host copies) behind the gate of the candidate cell
// ------------------------------------------------------------------------------------
struct DoorStepArgs {
    const uint8_t *cell;  // [flags | reward | door]
    int32_t cell_bytes, W;
    uint64_t lut;
    const int32_t *actions;
    int32_t *pos, *reward, *done;
    uint32_t *episode;
    uint32_t *tcount;
    uint32_t *open;
    const int32_t *starts;
    uint32_t n_starts, seed_prefix, env_id0;
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
__global__ void __launch_bounds__(GU_BLOCK) gu_doors_step_kernel(const DoorStepArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const CellMap m = gu_stage_map<LDS>(a.cell, a.cell_bytes, smem, a.gs, 3);
    const uint8_t *dr = m.f + 2 * a.cell_bytes;
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int32_t d = 0;
    if (e < a.N) {
        const uint32_t raw = (uint32_t)a.actions[e];
        const uint32_t act = raw & 3u;
        int32_t s = a.pos[e], r;
        if (a.host_err && !GU_ACTION_OK(raw)) {  // (gu_step_kernel: this env does not step, its mask stays, and the host is told)
            __hip_atomic_store(a.host_err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            a.tcount[e] -= 1u;
            r = a.reward[e];
            d = a.done[e];
        } else {
            uint32_t open = a.open[e];
            if ((a.flags & GU_F_AUTO_RESET) && a.done[e]) {  // lazy `if done: env.reset()`: the doors are shut again, the keys are back
                const uint32_t ep = a.episode[e];
                s = a.starts[gu_rng_start_index(gu_rng_prefix(a.seed_prefix, a.env_id0 + (uint32_t)e), ep, a.n_starts)];
                a.episode[e] = ep + 1;
                open = 0u;
            }
            const int32_t from = s;  // (behind the reset: a reset onto a key or lever cell touches nothing)
            const int32_t c = gu_move(s, m.f[s], act, gu_delta<LDS>(act, a.lut, a.W));
            const uint32_t dc = dr[c];
            s = gu_door_closed(dc, open) ? from : c;
            open = gu_door_touch(dc, open, s != from);
            r = m.r[s];
            d = (m.f[s] >> GU_CELL_TERM_BIT) & 1;
            a.pos[e] = s;
            a.reward[e] = r;
            a.done[e] = d;
            a.open[e] = open;
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

int gu_doors_launch_step(gu_engine *h, const int32_t *d_actions_row, uint32_t flags, int32_t *host_obs, int32_t *host_reward, int32_t *host_done,
                         uint32_t *host_seq, uint32_t seq, uint32_t *host_err)
{
    h->entry_table_ok = false;
    DoorStepArgs a{h->d_door_cell, h->cell_bytes, h->W, h->delta_lut, d_actions_row, h->pos(), h->reward(), h->done(), h->d_episode, h->d_tcount,
                    h->d_open, h->d_starts, (uint32_t)h->n_starts, h->seed_prefix, (uint32_t)h->env_id0, h->N, flags, gu_grid_sel(h),
                    host_obs, host_reward, host_done, host_seq, seq, h->d_blocks_done, host_err, h->d_done_bits};
    const int lds_bs = gu_lds_block(h, GU_BLOCK, 3);
    const dim3 grid(gu_blocks(h->N, GU_BLOCK)), block(GU_BLOCK);
    if (lds_bs) hipLaunchKernelGGL(gu_doors_step_kernel<true>, grid, block, 3 * (size_t)h->cell_bytes, h->stream, a);
    else hipLaunchKernelGGL(gu_doors_step_kernel<false>, grid, block, 0, h->stream, a);
    GU_HIP(hipGetLastError());
    h->steps_taken += 1;
    gu_tabular_drop_carry(h);
    return gu_trail_after_step(h, flags);
}

// ------------------------------------------------------------------------------------
// rollout: T steps per lane in one launch; the four policies with the calm kernels' streams 0, 1 and 2
// ------------------------------------------------------------------------------------
struct DoorRolloutArgs {
    const uint8_t *cell;  // [flags | reward | door]
    const uint8_t *greedy;
    const uint4 *pi_thr;
    int32_t cell_bytes, W;
    uint64_t lut;
    int32_t *pos, *reward, *done;
    uint32_t *episode;
    const uint32_t *tcount;
    uint32_t *open;
    const int32_t *starts;
    const uint32_t *actions;  // GU_POLICY_STREAM: the packed stream, [ceil(T / 16)][N]
    int32_t *tr_obs, *tr_reward, *tr_done;  // GU_F_TRAJECTORY: [T][N] planes (else nullptr)
    int32_t *ret, *episodes_fin;            // GU_F_STATS (else nullptr)
    uint64_t *done_bits;
    uint32_t n_starts, seed_prefix, env_id0;
    uint64_t steps_taken;
    int64_t N, T;
    int32_t auto_reset;
    GridSel gs;
};

// Auto-reset, rows and statistics are launch-uniform tests on the arguments.  The step count is 64 bits wide and streams 0 and 2 are
// re-keyed in the step that crosses a multiple of 2^32, so no launch needs another form.
template <int POLICY, bool LDS>
__global__ void __launch_bounds__(GU_BLOCK) gu_doors_rollout_kernel(const DoorRolloutArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const CellMap m = gu_stage_map<LDS>(a.cell, a.cell_bytes, smem, a.gs, 3);
    const uint8_t *dr = m.f + 2 * a.cell_bytes;
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int32_t d = 0;
    if (e < a.N) {
        const uint32_t env = a.env_id0 + (uint32_t)e;
        int32_t s = a.pos[e], r = a.reward[e];
        d = a.done[e];
        uint32_t ep = a.episode[e], open = a.open[e];
        uint32_t fs = m.f[s];   // the flags and the reward byte of the cell stood on, carried from step to step (the head of this file)
        int32_t rs = m.r[s];
        uint64_t t = a.steps_taken + (uint64_t)(int64_t)(int32_t)a.tcount[e];
        const uint32_t start_prefix = gu_rng_prefix(a.seed_prefix, env);  // stream 1: no epoch
        // streams 0 and 2 share the prefix of the step count's epoch: re-keyed in the step that crosses a multiple of 2^32
        uint32_t prefix = gu_rng_prefix(gu_rng_seed_prefix_epoch(a.seed_prefix, (uint32_t)(t >> 32)), env);
        uint32_t word = 0;  // uniform: the stream-0 word of steps t & ~15 ..; stream: the packed word; sample: the stream-2 word of step t
        if (POLICY == GU_POLICY_UNIFORM) word = gu_rng_word(prefix, GU_RNG_STREAM_ACTION, (uint32_t)t >> 4);
        if (POLICY == GU_POLICY_SAMPLE) word = gu_rng_sample_word(prefix, (uint32_t)t);
        int32_t ret = 0, fin = 0;
        for (int64_t i = 0; i < a.T; ++i) {
            if (a.auto_reset && d) {  // lazy `if done: env.reset()`: the doors are shut again, the keys are back
                s = a.starts[gu_rng_start_index(start_prefix, ep, a.n_starts)];
                ++ep;
                d = 0;
                open = 0u;
                fs = m.f[s];
                rs = m.r[s];
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
            const int32_t c = gu_move(s, fs, act, gu_delta<LDS>(act, a.lut, a.W));
            // three reads behind the one address c: flags, reward byte, door byte -- and the gate picks between them and the carried ones
            const uint32_t fc = m.f[c], dc = dr[c];
            const int32_t rc = m.r[c];
            const bool shut = gu_door_closed(dc, open);
            open = gu_door_touch(dc, open, !shut && c != s);
            s = shut ? s : c;
            fs = shut ? fs : fc;
            rs = shut ? rs : rc;
            r = rs;
            d = (int32_t)(fs >> GU_CELL_TERM_BIT) & 1;
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
        a.open[e] = open;
        if (a.ret) {
            a.ret[e] = ret;
            a.episodes_fin[e] = fin;
        }
    }
    const uint64_t bits = __ballot(d != 0);
    if ((threadIdx.x & 63) == 0 && e < a.N) a.done_bits[e >> 6] = bits;
}

// gu_launch_rollout hands a launch over here while doors are set: `r` is what it has filled in (state, tables, rows, streams)
void gu_doors_launch_rollout(gu_engine *h, const GuRolloutPlan &p, const RolloutArgs &r)
{
    DoorRolloutArgs a{};
    a.cell = h->d_door_cell, a.cell_bytes = h->cell_bytes, a.W = h->W, a.lut = h->delta_lut, a.gs = r.gs;
    a.greedy = r.greedy, a.pi_thr = r.pi_thr, a.actions = r.actions;
    a.pos = r.pos, a.reward = r.reward, a.done = r.done, a.episode = r.episode, a.tcount = r.tcount, a.done_bits = r.done_bits, a.open = h->d_open;
    a.starts = r.starts, a.n_starts = r.n_starts, a.env_id0 = r.env_id0, a.seed_prefix = h->seed_prefix;
    a.tr_obs = p.traj ? r.tr_obs : nullptr, a.tr_reward = p.traj ? r.tr_reward : nullptr, a.tr_done = p.traj ? r.tr_done : nullptr;
    a.ret = p.stats ? r.ret : nullptr, a.episodes_fin = p.stats ? r.episodes_fin : nullptr;
    a.N = h->N, a.T = r.T, a.steps_taken = h->steps_taken, a.auto_reset = p.auto_mode ? 1 : 0;
    gu_pick<3, 2, 1, 0>(p.policy, [&](auto policy_c) {
        gu_pick<0, 1>(p.lds != 0, [&](auto lds_c) {
            constexpr int POLICY = decltype(policy_c)::value;
            constexpr bool LDS = decltype(lds_c)::value != 0;
            gu_lds_launch<gu_doors_rollout_kernel<POLICY, LDS>, false>(h, p.blocks, p.block, p.lds, a);
        });
    });
}

// ------------------------------------------------------------------------------------
// resets: gu_reset and gu_reset_done clear the masks of the envs they reset, in a launch of its own IN FRONT of gu_reset_kernel (it
// reads the done flags that the reset is about to clear); that kernel is untouched and engines without doors never get here
// ------------------------------------------------------------------------------------
__global__ void __launch_bounds__(GU_BLOCK) gu_doors_reset_kernel(uint32_t *__restrict__ open, const uint8_t *__restrict__ mask, const int32_t *__restrict__ done,
                                                                   int32_t only_done, int64_t N)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= N) return;
    bool take = !mask || mask[e];
    if (only_done && !done[e]) take = false;
    if (take) open[e] = 0u;
}

int gu_doors_before_reset(gu_engine *h, const uint8_t *d_mask, bool only_done)
{
    if (!h->n_doors) return GU_OK;
    hipLaunchKernelGGL(gu_doors_reset_kernel, dim3(gu_blocks(h->N, GU_BLOCK)), dim3(GU_BLOCK), 0, h->stream, h->d_open, d_mask, h->done(), only_done ? 1 : 0, h->N);
    GU_HIP(hipGetLastError());
    return GU_OK;
}

void gu_doors_free(gu_engine *h)
{
    gu_release(h->d_door_cell, h->d_open);
    h->n_doors = 0;
}

// ------------------------------------------------------------------------------------
// entry points
// ------------------------------------------------------------------------------------
extern "C" {

int gu_set_doors(gu_handle h, const uint8_t *door)
{
    GU_ENTER(h);
    GU_NEED_GRID(h);
    GU_REQUIRE(h->n_grids == 1, GU_ERR_UNSUPPORTED, "doors are a property of a single-grid engine (this one holds %d grids)", h->n_grids);
    GU_REQUIRE(!h->d_wind_cell, GU_ERR_UNSUPPORTED, "doors and wind exclude each other: the engine has wind set (gu_set_wind; NULL calms it again)");
    GU_REQUIRE(!h->n_fruit, GU_ERR_UNSUPPORTED, "doors and fruit exclude each other: the engine has fruit set (gu_set_fruit; NULL takes it away again)");
    GU_REQUIRE(!h->trail_cap, GU_ERR_UNSUPPORTED, "doors and the agent trail exclude each other: the trail is on (gu_trail_enable(h, 0) turns it off)");
    int32_t D = 0;
    if (door) {
        std::vector<uint8_t> flags((size_t)h->S);
        GU_HIP(hipStreamSynchronize(h->stream));
        GU_HIP(hipMemcpy(flags.data(), h->d_cell, (size_t)h->S, hipMemcpyDeviceToHost));
        uint32_t doors = 0, openers = 0;  // slots that have a door cell / a key or lever cell
        for (int32_t s = 0; s < h->S; ++s) {
            const uint32_t c = door[s], kind = (c >> 4) & 3u, slot = c & 7u;
            if (!c) continue;
            // (bit 3 would be a ninth slot: the mask has eight)
            GU_REQUIRE(!(c & 0xC8u) && kind != 0u, GU_ERR_INVALID, "door byte 0x%02x of cell %d: bits 3, 6 and 7 must be zero (slots 0 .. 7), and kind 0 means the whole byte is zero", c, s);
            GU_REQUIRE(!(flags[s] & (GU_CELL_WALL | GU_CELL_TERM)), GU_ERR_INVALID, "a door, key or lever on cell %d, which is a wall or a goal or lava cell", s);
            (kind == 1u ? doors : openers) |= 1u << slot;
        }
        const uint32_t used = doors | openers;
        GU_REQUIRE(used != 0u, GU_ERR_INVALID, "nothing in the plane (NULL takes the doors away)");
        D = __builtin_popcount(used);
        GU_REQUIRE(used == (1u << D) - 1u, GU_ERR_INVALID, "the %d slots in use must be 0 .. %d (slot mask 0x%02x)", D, D - 1, used);
        GU_REQUIRE(doors == used, GU_ERR_INVALID, "a slot without a door cell (slots with doors 0x%02x, in use 0x%02x)", doors, used);
        GU_REQUIRE(openers == used, GU_ERR_INVALID, "a slot without a key or lever cell (slots with keys or levers 0x%02x, in use 0x%02x)", openers, used);
    }
    GU_HIP(hipStreamSynchronize(h->stream));
    const size_t cb = (size_t)h->cell_bytes;
    uint8_t *cell = nullptr;
    uint32_t *open = h->d_open;
    if (door) {
        // What can fail comes first, on buffers the engine does not hold yet: a refused call leaves the engine as it was, a failed
        // allocation or copy included.  The planes are built in a fresh buffer and swapped in below.
        std::vector<uint8_t> plane(cb, 0);  // (the padding behind cell S - 1 bears nothing)
        std::copy(door, door + h->S, plane.begin());
        hipError_t e = hipMalloc(&cell, 3 * cb);
        if (e == hipSuccess && !open) e = hipMalloc(&open, (size_t)h->N * sizeof(uint32_t));
        if (e == hipSuccess) e = hipMemcpy(cell, h->d_cell, 2 * cb, hipMemcpyDeviceToDevice);
        if (e == hipSuccess) e = hipMemcpy(cell + 2 * cb, plane.data(), cb, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemset(open, 0, (size_t)h->N * sizeof(uint32_t));  // (the last step that can fail: behind it the call is not refused)
        if (e != hipSuccess) {
            (void)hipFree(cell);
            if (open != h->d_open) (void)hipFree(open);
            return gu_fail(e == hipErrorOutOfMemory ? GU_ERR_NOMEM : GU_ERR_HIP, "gu_set_doors: the door planes and masks: %s", hipGetErrorString(e));
        }
    }
    gu_tabular_drop_carry(h);  // another move rule: what the learners carry belongs to the old one
    h->entry_table_ok = false;
    if (h->graph_exec) {  // (a captured step graph holds the launches without doors)
        (void)hipGraphExecDestroy(h->graph_exec);
        h->graph_exec = nullptr;
    }
    gu_td_rows_changed(h, D);  // Q tables of another row count go (S << D rows: gu_td_run)
    if (!door) {
        gu_doors_free(h);
        return GU_OK;
    }
    gu_release(h->d_door_cell);
    h->d_door_cell = cell;
    h->d_open = open;
    h->n_doors = D;
    return GU_OK;
}

int gu_get_doors(gu_handle h, uint8_t *door, int32_t *n_slots)
{
    GU_ENTER(h);
    GU_NEED_GRID(h);
    if (n_slots) *n_slots = h->n_doors;
    if (door) {
        if (h->n_doors) {
            GU_HIP(hipStreamSynchronize(h->stream));
            GU_HIP(hipMemcpy(door, h->d_door_cell + 2 * (size_t)h->cell_bytes, (size_t)h->S, hipMemcpyDeviceToHost));
        } else {
            std::fill(door, door + h->S, (uint8_t)0);
        }
    }
    return GU_OK;
}

static int gu_doors_range(gu_engine *h, int64_t env0, int64_t n, const void *open)
{
    GU_NEED_GRID(h);
    GU_REQUIRE(h->n_doors, GU_ERR_STATE, "no doors set: call gu_set_doors first");
    GU_REQUIRE(open != nullptr, GU_ERR_INVALID, "open is NULL");
    return gu_env_range(h, env0, n);
}

int gu_get_doors_state(gu_handle h, int64_t env0, int64_t n, uint32_t *open)
{
    GU_ENTER(h);
    GU_TRY(gu_doors_range(h, env0, n, open));
    return gu_env_copy(h, hipMemcpyDeviceToHost, open, h->d_open, env0, n, 1);
}

int gu_set_doors_state(gu_handle h, int64_t env0, int64_t n, const uint32_t *open)
{
    GU_ENTER(h);
    GU_TRY(gu_doors_range(h, env0, n, open));
    for (int64_t i = 0; i < n; ++i)
        GU_REQUIRE((open[i] >> h->n_doors) == 0u, GU_ERR_INVALID, "open[%lld] = 0x%08x has a bit at or above the %d slots", (long long)i, open[i], h->n_doors);
    gu_tabular_drop_carry(h);  // (a carried SARSA action was drawn on the row of the old mask)
    h->entry_table_ok = false;
    return gu_env_copy(h, hipMemcpyHostToDevice, open, h->d_open, env0, n, 1);
}

}  // extern "C"
