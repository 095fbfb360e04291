// gu_overlay.hpp -- what the kernels of the overlays share (DESIGN.md "Overlays"; gu_wind.hip, gu_fruit.hip, gu_doors.hip, gu_boxes.hip, gu_errands.hip): the
// argument structs that gu_overlay.hip fills, the completion word of a step kernel, the per-lane policy of a rollout kernel, and, for the
// four kinds that keep a word per env, the step kernel and the rollout kernel themselves: two frames around a rule struct of the kind's
// own file, with the ladders from launch shape to instantiation.  The rule stays written out in that struct; wind keeps its own kernels.
#pragma once
#include "gu_rollout.hpp"  // (gu_map.hpp, gu_rng.hpp, gu_sample_action, RolloutArgs)

// ---- single step: gu_step_kernel's arguments with the overlay's plane behind the two cell planes.  A kernel ignores what it does
// not use: wind reads no mask, doors no param, only gusts ask for the step count and only errands read param2. ----
struct OverlayStepArgs {
    const uint8_t *cell;  // [flags | reward | overlay]
    int32_t cell_bytes, W;
    uint64_t lut;
    const int32_t *actions;
    int32_t *pos, *reward, *done;
    uint32_t *episode;
    uint32_t *tcount;
    uint32_t *mask;  // [N] fruit: eaten, doors: open, boxes: the boxes' cells, errands: eaten | progress | instruction (gu_engine::d_overlay_mask)
    const int32_t *starts;
    uint32_t n_starts, seed_prefix, env_id0, param;  // param: gu_engine::overlay_param
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
    uint32_t init;  // the mask of an env that has just been reset (gu_engine::overlay_init: 0 but for boxes)
    uint32_t param2;  // gu_engine::overlay_param2 (errands: the pay and the field widths)
};

// ---- rollout: T steps per lane in one launch; the four policies with the calm kernels' action and sampling streams (0 and 2) ----
struct OverlayRolloutArgs {
    const uint8_t *cell;  // [flags | reward | overlay]
    const uint8_t *greedy;
    const uint4 *pi_thr;
    int32_t cell_bytes, W;
    uint64_t lut;
    int32_t *pos, *reward, *done;
    uint32_t *episode;
    const uint32_t *tcount;
    uint32_t *mask;
    const int32_t *starts;
    const uint32_t *actions;  // GU_POLICY_STREAM: the packed stream, [ceil(T / 16)][N]
    int32_t *tr_obs, *tr_reward, *tr_done;  // GU_F_TRAJECTORY: [T][N] planes (else nullptr)
    int32_t *ret, *episodes_fin;            // GU_F_STATS (else nullptr)
    uint64_t *done_bits;
    uint32_t n_starts, seed_prefix, env_id0, param;
    uint64_t steps_taken;
    int64_t N, T;
    int32_t auto_reset;
    GridSel gs;
    uint32_t init;  // (as OverlayStepArgs::init)
    uint32_t param2;  // (as OverlayStepArgs::param2)
};

// The completion word of a step kernel (gu_step_kernel and the overlays'): the host spins on a sequence number in page-locked memory
// instead of going through the runtime's completion path (no interrupt, no runtime call).  Every block makes its mirror stores
// visible to the host, then counts itself; the block that completes the count publishes the number (and re-arms the counter).
__device__ __forceinline__ void gu_step_publish(uint32_t *host_seq, uint32_t seq, uint32_t *blocks_done)
{
    if (host_seq) {
        __threadfence_system();
        __syncthreads();
        if (threadIdx.x == 0) {
            const uint32_t arrived = atomicAdd(blocks_done, 1u);
            if (arrived == gridDim.x - 1) {
                *blocks_done = 0u;
                __threadfence_system();
                __hip_atomic_store(host_seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
    }
}

// One lane's policy in an overlay rollout kernel.  The step count is 64 bits wide and streams 0, 2 and 9 share the prefix of its
// epoch, re-keyed in the step that crosses a multiple of 2^32, so no launch needs another form.
template <int POLICY>
struct OverlayPolicy {
    uint32_t env, prefix;
    uint32_t word;  // uniform: the stream-0 word of steps t & ~15 ..; stream: the packed word; sample: the stream-2 word of step t
    uint64_t t;

    __device__ __forceinline__ void begin(const OverlayRolloutArgs &a, uint32_t env_, uint64_t t_)
    {
        env = env_, t = t_;
        prefix = gu_rng_prefix(gu_rng_seed_prefix_epoch(a.seed_prefix, (uint32_t)(t >> 32)), env);
        word = 0;
        if (POLICY == GU_POLICY_UNIFORM) word = gu_rng_word(prefix, GU_RNG_STREAM_ACTION, (uint32_t)t >> 4);
        if (POLICY == GU_POLICY_SAMPLE) word = gu_rng_sample_word(prefix, (uint32_t)t);
    }

    // the action of step i of the launch for env index e on cell s
    __device__ __forceinline__ uint32_t act(const OverlayRolloutArgs &a, int64_t i, int64_t e, int32_t s)
    {
        if (POLICY == GU_POLICY_UNIFORM) return (word >> (2u * ((uint32_t)t & 15u))) & 3u;
        if (POLICY == GU_POLICY_STREAM) {
            if ((i & 15) == 0) word = a.actions[(i >> 4) * a.N + e];
            return (word >> (2u * (uint32_t)(i & 15))) & 3u;
        }
        if (POLICY == GU_POLICY_GREEDY) return a.greedy[s];
        return gu_sample_action(word, a.pi_thr[s]);
    }

    __device__ __forceinline__ void next(const OverlayRolloutArgs &a)
    {
        ++t;
        if (((uint32_t)t & 15u) == 0u) {  // the next sixteen steps' words (and, once in 2^32 steps, the next epoch's prefix)
            if ((uint32_t)t == 0u) prefix = gu_rng_prefix(gu_rng_seed_prefix_epoch(a.seed_prefix, (uint32_t)(t >> 32)), env);
            if (POLICY == GU_POLICY_UNIFORM) word = gu_rng_word(prefix, GU_RNG_STREAM_ACTION, (uint32_t)t >> 4);
            if (POLICY == GU_POLICY_SAMPLE) word = gu_rng_word(prefix, GU_RNG_STREAM_SAMPLE, (uint32_t)t >> 4);
        } else if (POLICY == GU_POLICY_SAMPLE) {
            word = gu_rng_sample_next(word);
        }
    }
};

// ------------------------------------------------------------------------------------
// the two frames of fruit, doors, boxes and errands: everything of a step and of a rollout kernel that is contract and not rule
// ------------------------------------------------------------------------------------
// These four kinds keep a uint32 word per env and move one lane at a time, so their kernels differ in the rule alone.  Wind's do not
// fit and are not bent to: they run every lane of the wave, lanes past the batch included (the push loop and the gust ballot are
// wave-uniform), carry no word and take GUST as a template parameter -- another frame, gu_wind.hip's own.
//
// A kind's RULE is a struct that holds the lane's word and what the kind carries beside it, with four functions; `a` is the launch's
// OverlayStepArgs or OverlayRolloutArgs (a rule reads param, param2, init, lut and W of it), `m` the staged planes:
//   void load(const ARGS &a, const OverlayMap &m, uint32_t word, int32_t s)
//        the word as it came from mask[e], and the carried values derived from it and from the cell s stood on (once per launch);
//   void reset(const ARGS &a, const OverlayMap &m, uint32_t start_prefix, uint32_t ep, int32_t s)
//        what a lazy reset restores: start_prefix is stream 1's (seed and env, no epoch), ep the episode count BEFORE the reset
//        increments it, s the start cell;
//   template <bool LDS> void move(const ARGS &a, const OverlayMap &m, uint32_t act, int32_t &s, int32_t &r, int32_t &d)
//        one step of the rule: leaves the cell, the reward, the done flag and the lane's own state behind the step;
//   uint32_t word() const
//        the word to store in mask[e];
//   static constexpr bool DONE_IN_PLACE
//        for the compiler, not for the reader: true where the rollout frame hands its own `d` to move, false where move writes a copy
//        that the frame assigns.  The values are the same; what differs is when the compiler first sees `d` as a value (a variable
//        whose address goes to a force-inlined function stays in memory until that function is inlined), and with it whether the
//        done ballot is taken from a VGPR or from a carried SGPR pair and which registers the loop gets.  Each kind states the form
//        its kernel had before the frames, so every loop keeps its instruction sequence (docs/HISTORY.md "Overlay frames").
// The step/rollout rule is NOT the learners' (OV of gu_tabular_overlay.hpp): that one takes the lane by reference for reasons of code
// generation (docs/HISTORY.md "Learner lane"), and the two stay apart.
struct OverlayMap {
    const uint8_t *f;  // flags plane
    const int8_t *r;   // reward plane
    const uint8_t *o;  // the overlay's plane
};

template <bool LDS, class ARGS>
__device__ __forceinline__ OverlayMap gu_stage_overlay(const ARGS &a, uint8_t *smem)
{
    const CellMap m = gu_stage_map<LDS>(a.cell, a.cell_bytes, smem, a.gs, 3);
    return OverlayMap{m.f, m.r, m.f + 2 * a.cell_bytes};
}

// single step: gu_step_kernel's rules (rejected actions, lazy auto-reset, done ballot, host copies, completion word) around RULE::move
template <class RULE, bool LDS>
__global__ void __launch_bounds__(GU_BLOCK) gu_overlay_step_kernel(const OverlayStepArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const OverlayMap m = gu_stage_overlay<LDS>(a, smem);
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int32_t done = 0;  // (the ballot's; lanes past the batch vote 0)
    if (e < a.N) {
        const uint32_t raw = (uint32_t)a.actions[e];
        const uint32_t act = raw & 3u;
        int32_t s = a.pos[e], r, d;
        if (a.host_err && !GU_ACTION_OK(raw)) {  // (gu_step_kernel: this env does not step, its word stays, nothing is drawn, and the host is told)
            __hip_atomic_store(a.host_err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            a.tcount[e] -= 1u;
            r = a.reward[e];
            d = a.done[e];
        } else {
            RULE R;
            R.load(a, m, a.mask[e], s);
            if ((a.flags & GU_F_AUTO_RESET) && a.done[e]) {  // lazy `if done: env.reset()`
                const uint32_t ep = a.episode[e];
                const uint32_t start_prefix = gu_rng_prefix(a.seed_prefix, a.env_id0 + (uint32_t)e);
                s = a.starts[gu_rng_start_index(start_prefix, ep, a.n_starts)];
                a.episode[e] = ep + 1;
                R.reset(a, m, start_prefix, ep, s);
            }
            R.template move<LDS>(a, m, act, s, r, d);
            a.pos[e] = s;
            a.reward[e] = r;
            a.done[e] = d;
            a.mask[e] = R.word();
        }
        if (a.host_obs) a.host_obs[e] = s;
        if (a.host_reward) a.host_reward[e] = r;
        if (a.host_done) a.host_done[e] = d;
        done = d;
    }
    const uint64_t bits = __ballot(done != 0);
    if ((threadIdx.x & 63) == 0 && e < a.N) a.done_bits[e >> 6] = bits;
    gu_step_publish(a.host_seq, a.seq, a.blocks_done);
}

// rollout: T steps per lane in one launch.  Auto-reset, rows and statistics are launch-uniform tests on the arguments; the state and
// the word stay in VGPRs for the whole launch: one load at the start, one store at the end.  Plain stores, no schedule (GuPacer).
template <class RULE, int POLICY, bool LDS>
__global__ void __launch_bounds__(GU_BLOCK) gu_overlay_rollout_kernel(const OverlayRolloutArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const OverlayMap m = gu_stage_overlay<LDS>(a, smem);
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int32_t d = 0;
    if (e < a.N) {
        const uint32_t env = a.env_id0 + (uint32_t)e;
        int32_t s = a.pos[e], r = a.reward[e];
        d = a.done[e];
        uint32_t ep = a.episode[e];
        RULE R;
        R.load(a, m, a.mask[e], s);
        const uint64_t t0 = a.steps_taken + (uint64_t)(int64_t)(int32_t)a.tcount[e];
        const uint32_t start_prefix = gu_rng_prefix(a.seed_prefix, env);  // stream 1 (and the errands' 11): no epoch
        OverlayPolicy<POLICY> P;
        P.begin(a, env, t0);
        int32_t ret = 0, fin = 0;
        for (int64_t i = 0; i < a.T; ++i) {
            if (a.auto_reset && d) {  // lazy `if done: env.reset()`
                s = a.starts[gu_rng_start_index(start_prefix, ep, a.n_starts)];
                R.reset(a, m, start_prefix, ep, s);
                ++ep;
                d = 0;
            }
            const uint32_t act = P.act(a, i, e, s);
            if constexpr (RULE::DONE_IN_PLACE) {
                R.template move<LDS>(a, m, act, s, r, d);
            } else {  // (the same values through a copy: see DONE_IN_PLACE above)
                int32_t d1;
                R.template move<LDS>(a, m, act, s, r, d1);
                d = d1;
            }
            P.next(a);
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
        a.mask[e] = R.word();
        if (a.ret) {
            a.ret[e] = ret;
            a.episodes_fin[e] = fin;
        }
    }
    const uint64_t bits = __ballot(d != 0);
    if ((threadIdx.x & 63) == 0 && e < a.N) a.done_bits[e >> 6] = bits;
}

// the ladders from launch shape to instantiation; a kind's gu_<kind>_step and gu_<kind>_rollout call them from its own file, so each
// kind's ten instantiations compile in their own object
template <class RULE>
static void gu_overlay_step_launch(gu_engine *h, bool lds, const OverlayStepArgs &a)
{
    const dim3 grid(gu_blocks(h->N, GU_BLOCK)), block(GU_BLOCK);
    if (lds) hipLaunchKernelGGL((gu_overlay_step_kernel<RULE, true>), grid, block, 3 * (size_t)h->cell_bytes, h->stream, a);
    else hipLaunchKernelGGL((gu_overlay_step_kernel<RULE, false>), grid, block, 0, h->stream, a);
}

template <class RULE>
static void gu_overlay_rollout_launch(gu_engine *h, const GuRolloutPlan &p, const OverlayRolloutArgs &a)
{
    gu_pick<3, 2, 1, 0>(p.policy, [&](auto policy_c) {  // (the lists run backwards, as gu_rollout.hpp's do: the kernels keep their order in the code object)
        gu_pick<0, 1>(p.lds != 0, [&](auto lds_c) {
            constexpr int POLICY = decltype(policy_c)::value;
            constexpr bool LDS = decltype(lds_c)::value != 0;
            gu_lds_launch<gu_overlay_rollout_kernel<RULE, POLICY, LDS>, false>(h, p.blocks, p.block, p.lds, a);
        });
    });
}
