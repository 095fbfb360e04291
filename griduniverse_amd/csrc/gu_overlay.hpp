// gu_overlay.hpp -- what the kernels of the overlays share (DESIGN.md "Overlays"; gu_wind.hip, gu_fruit.hip, gu_doors.hip, gu_boxes.hip, gu_errands.hip): the
// argument structs that gu_overlay.hip fills, the completion word of a step kernel and the per-lane policy of a rollout kernel.
// Everything around a feature's move or reward rule; the rule itself stays written out in the feature's own kernels.
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
