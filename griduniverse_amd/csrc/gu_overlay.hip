// gu_overlay.hip -- the overlay slot of a single-grid engine (DESIGN.md "Overlays"): wind, fruit, doors, boxes or errands, at most one at a time.
// An overlay is a third byte plane behind the engine's two cell planes (gu_engine::d_overlay_cell holds all three in one piece, which
// its kernels stage in LDS where they fit 64 KiB) and, for fruit, doors and boxes, one uint32 mask per env with its value at reset
// (gu_engine::overlay_init: 0 but for boxes).  Here is everything around a feature's rule: the install path, the getters, the masks'
// copies, the masks' reset, the arguments of the step, rollout and learner launches, the readback of the grid's flags that a plane is
// validated against and the plane format that fruit and errands share.  The features keep their plane's validation and their rule:
// wind in kernels of its own (gu_wind.hip), fruit, doors, boxes and errands in a rule struct for the two frames of gu_overlay.hpp
// (gu_fruit.hip, gu_doors.hip, gu_boxes.hip, gu_errands.hip); errands keep their reset kernel too (it draws).
#include "gu_overlay.hpp"
#include "gu_tabular.hpp"  // (gu_env_range, gu_env_copy)

#include <algorithm>
#include <vector>

int gu_overlay_admits(gu_engine *h, int kind)
{
    const char *name = GU_OVERLAY_NAME[kind];
    GU_REQUIRE(h->n_grids == 1, GU_ERR_UNSUPPORTED, "gu_set_%s needs a single-grid engine (this one holds %d grids)", name, h->n_grids);
    GU_REQUIRE(!h->trail_cap, GU_ERR_UNSUPPORTED, "%s and the agent trail exclude each other: the trail is on (gu_trail_enable(h, 0) turns it off)", name);
    GU_REQUIRE(!h->overlay || h->overlay == kind, GU_ERR_UNSUPPORTED, "%s and %s exclude each other: %s", name, GU_OVERLAY_NAME[h->overlay],
               GU_OVERLAY_IS_SET[h->overlay]);
    return GU_OK;
}

void gu_overlay_free(gu_engine *h)
{
    gu_release(h->d_overlay_cell, h->d_overlay_mask);
    h->overlay = GU_OVERLAY_NONE;
    h->overlay_bits = 0;
    h->overlay_param = 0;
    h->overlay_param2 = 0;
    h->overlay_init = 0;
    h->box_flags.clear();
    std::fill(h->fruit_value, h->fruit_value + 3, 0);
}

int gu_overlay_install(gu_engine *h, int kind, const uint8_t *plane, int32_t bits, uint32_t param, uint32_t init, uint32_t param2)
{
    GU_TRY(gu_overlay_admits(h, kind));
    GU_HIP(hipStreamSynchronize(h->stream));
    const size_t cb = (size_t)h->cell_bytes, mask_bytes = (size_t)h->N * sizeof(uint32_t);
    uint8_t *cell = nullptr;
    uint32_t *mask = nullptr;
    if (plane) {
        // What can fail comes first, on buffers the engine does not hold yet: a refused call leaves the engine as it was, a failed
        // allocation or copy included.  The planes are built in a fresh buffer and swapped in below.
        std::vector<uint8_t> padded(cb, 0);  // (the padding behind cell S - 1 bears nothing)
        std::copy(plane, plane + h->S, padded.begin());
        hipError_t e = hipMalloc(&cell, 3 * cb);
        if (e == hipSuccess && bits) e = hipMalloc(&mask, mask_bytes);
        if (e == hipSuccess) e = hipMemcpy(cell, h->d_cell, 2 * cb, hipMemcpyDeviceToDevice);
        if (e == hipSuccess) e = hipMemcpy(cell + 2 * cb, padded.data(), cb, hipMemcpyHostToDevice);
        if (e == hipSuccess && bits) e = hipMemsetD32((hipDeviceptr_t)mask, (int)init, (size_t)h->N);  // (the last step that can fail: behind it the call is not refused)
        if (e != hipSuccess) {
            gu_release(cell, mask);
            return gu_fail(e == hipErrorOutOfMemory ? GU_ERR_NOMEM : GU_ERR_HIP, "gu_set_%s: the planes and masks: %s", GU_OVERLAY_NAME[kind], hipGetErrorString(e));
        }
    }
    gu_envs_touched(h);  // another move or reward rule: what the learners carry belongs to the old one
    gu_graph_drop(h);    // (a captured step graph holds the launches of the old rule)
    gu_td_rows_changed(h, plane ? bits : 0);  // Q tables of another row count go (S << bits rows: gu_td_run)
    gu_overlay_free(h);
    if (!plane) return GU_OK;
    h->overlay = kind;
    h->d_overlay_cell = cell;
    h->d_overlay_mask = mask;
    h->overlay_bits = bits;
    h->overlay_param = param;
    h->overlay_param2 = param2;
    h->overlay_init = init;
    return GU_OK;
}

// the flags plane of the engine's grid on the host (wall and terminal bits: what nothing of an overlay's plane may lie on)
int gu_overlay_grid_flags(gu_engine *h, std::vector<uint8_t> &flags)
{
    flags.resize((size_t)h->S);
    GU_HIP(hipStreamSynchronize(h->stream));
    GU_HIP(hipMemcpy(flags.data(), h->d_cell, (size_t)h->S, hipMemcpyDeviceToHost));
    return GU_OK;
}

// The plane format that fruit and errands share (bits 0..4 the slot, bits 5..6 the kind): bit 7 zero, kind 0 only in a zero byte, no
// fruit on a wall or terminal cell, at most `cap` fruits, which use the slots 0 .. F - 1 each once.  Each kind keeps its own words.
int gu_overlay_fruit_plane(gu_engine *h, int kind, const uint8_t *plane, int32_t cap, int32_t *n_fruit, int32_t *of_kind)
{
    const bool errands = kind == GU_OVERLAY_ERRANDS;
    std::vector<uint8_t> flags;
    GU_TRY(gu_overlay_grid_flags(h, flags));
    int32_t F = 0;
    uint32_t slots = 0;
    for (int32_t s = 0; s < h->S; ++s) {
        const uint32_t c = plane[s], k = (c >> 5) & 3u, slot = c & 31u;
        if (!c) continue;
        GU_REQUIRE(!(c & 0x80u) && k != 0u, GU_ERR_INVALID, "%s byte 0x%02x of cell %d: bit 7 must be zero, and kind 0 means the whole byte is zero", errands ? "errand" : "fruit",
                   c, s);
        GU_REQUIRE(F < cap, GU_ERR_INVALID, "more than %d fruits", cap);
        GU_REQUIRE(!(flags[s] & (GU_CELL_WALL | GU_CELL_TERM)), GU_ERR_INVALID, "fruit on cell %d, which is a wall or a goal or lava cell", s);
        GU_REQUIRE(slot < (uint32_t)cap && !((slots >> slot) & 1u), GU_ERR_INVALID,
                   errands ? "slot %u of cell %d is used twice or lies above 7" : "slot %u is used twice (second at cell %d)", slot, s);
        slots |= 1u << slot;
        if (of_kind) ++of_kind[k];
        ++F;
    }
    GU_REQUIRE(F >= 1, GU_ERR_INVALID, "no fruit in the plane (NULL takes the %s away)", GU_OVERLAY_NAME[kind]);
    GU_REQUIRE(slots == (F == 32 ? ~0u : (1u << F) - 1u), GU_ERR_INVALID,
               errands ? "the %d fruits must use the slots 0 .. %d, each once (slot mask 0x%02x)" : "the %d fruits must use the slots 0 .. %d, each once (slot mask 0x%08x)", F,
               F - 1, slots);
    *n_fruit = F;
    return GU_OK;
}

int gu_overlay_get_plane(gu_engine *h, int kind, uint8_t *plane)
{
    if (h->overlay != kind) {
        std::fill(plane, plane + h->S, (uint8_t)0);
        return GU_OK;
    }
    GU_HIP(hipStreamSynchronize(h->stream));
    GU_HIP(hipMemcpy(plane, h->d_overlay_cell + 2 * (size_t)h->cell_bytes, (size_t)h->S, hipMemcpyDeviceToHost));
    return GU_OK;
}

// ------------------------------------------------------------------------------------
// the masks: copies for envs env0 .. env0+n-1 (`what`: the caller's name of the array), and the resets
// ------------------------------------------------------------------------------------
static int gu_overlay_mask_range(gu_engine *h, int kind, int64_t env0, int64_t n, const void *masks, const char *what)
{
    GU_NEED_GRID(h);
    GU_REQUIRE(h->overlay == kind, GU_ERR_STATE, "no %s set: call gu_set_%s first", GU_OVERLAY_NAME[kind], GU_OVERLAY_NAME[kind]);
    GU_REQUIRE(masks != nullptr, GU_ERR_INVALID, "%s is NULL", what);
    return gu_env_range(h, env0, n);
}

int gu_overlay_get_masks(gu_engine *h, int kind, int64_t env0, int64_t n, uint32_t *masks, const char *what)
{
    GU_TRY(gu_overlay_mask_range(h, kind, env0, n, masks, what));
    return gu_env_copy(h, hipMemcpyDeviceToHost, masks, h->d_overlay_mask, env0, n, 1);
}

int gu_overlay_set_masks(gu_engine *h, int kind, int64_t env0, int64_t n, const uint32_t *masks, const char *what)
{
    GU_TRY(gu_overlay_mask_range(h, kind, env0, n, masks, what));
    if (h->overlay_bits < 32)  // (32 fruits use every bit)
        for (int64_t i = 0; i < n; ++i)
            GU_REQUIRE((masks[i] >> h->overlay_bits) == 0u, GU_ERR_INVALID, "%s[%lld] = 0x%08x has a bit at or above the %d bits in use", what, (long long)i,
                       masks[i], h->overlay_bits);
    gu_envs_touched(h);  // (a carried SARSA action was drawn on the row of the old mask)
    return gu_env_copy(h, hipMemcpyHostToDevice, masks, h->d_overlay_mask, env0, n, 1);
}

// gu_reset and gu_reset_done set the masks of the envs they reset to the slot's reset value (0 but for boxes), in a launch of its own IN FRONT of gu_reset_kernel (it reads the
// done flags that the reset is about to clear); that kernel is untouched and engines without masks never get here
__global__ void __launch_bounds__(GU_BLOCK) gu_overlay_reset_kernel(uint32_t *__restrict__ masks, const uint8_t *__restrict__ mask, const int32_t *__restrict__ done,
                                                                     int32_t only_done, int64_t N, uint32_t init)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= N) return;
    bool take = !mask || mask[e];
    if (only_done && !done[e]) take = false;
    if (take) masks[e] = init;
}

int gu_overlay_before_reset(gu_engine *h, const uint8_t *d_mask, bool only_done)
{
    if (!h->d_overlay_mask) return GU_OK;
    if (h->overlay == GU_OVERLAY_ERRANDS) return gu_errands_before_reset(h, d_mask, only_done);  // (draws the instruction: gu_errands.hip)
    hipLaunchKernelGGL(gu_overlay_reset_kernel, dim3(gu_blocks(h->N, GU_BLOCK)), dim3(GU_BLOCK), 0, h->stream, h->d_overlay_mask, d_mask, h->done(), only_done ? 1 : 0, h->N,
                       h->overlay_init);
    GU_HIP(hipGetLastError());
    return GU_OK;
}

// ------------------------------------------------------------------------------------
// the launches: the arguments are the same for every overlay; the feature picks its kernel's instantiation
// ------------------------------------------------------------------------------------
int gu_overlay_launch_step(gu_engine *h, const int32_t *d_actions_row, uint32_t flags, int32_t *host_obs, int32_t *host_reward, int32_t *host_done,
                           uint32_t *host_seq, uint32_t seq, uint32_t *host_err)
{
    static void (*const step[])(gu_engine *, bool, const OverlayStepArgs &) = {nullptr, gu_wind_step, gu_fruit_step, gu_doors_step, gu_boxes_step, gu_errands_step};
    const OverlayStepArgs a{h->d_overlay_cell, h->cell_bytes, h->W, h->delta_lut, d_actions_row, h->pos(), h->reward(), h->done(), h->d_episode, h->d_tcount,
                            h->d_overlay_mask, h->d_starts, (uint32_t)h->n_starts, h->seed_prefix, (uint32_t)h->env_id0, h->overlay_param, h->steps_taken, h->N, flags,
                            gu_grid_sel(h), host_obs, host_reward, host_done, host_seq, seq, h->d_blocks_done, host_err, h->d_done_bits, h->overlay_init, h->overlay_param2};
    step[h->overlay](h, gu_lds_block(h, GU_BLOCK, 3) != 0, a);
    GU_HIP(hipGetLastError());
    gu_envs_touched(h, 1);
    return gu_trail_after_step(h, flags);
}

// `r` is what gu_launch_rollout has filled in (state, tables, rows, streams)
void gu_overlay_launch_rollout(gu_engine *h, const GuRolloutPlan &p, const RolloutArgs &r)
{
    static void (*const rollout[])(gu_engine *, const GuRolloutPlan &, const OverlayRolloutArgs &) = {nullptr, gu_wind_rollout, gu_fruit_rollout, gu_doors_rollout,
                                                                                                      gu_boxes_rollout, gu_errands_rollout};
    OverlayRolloutArgs a{};
    a.cell = h->d_overlay_cell, a.cell_bytes = h->cell_bytes, a.W = h->W, a.lut = h->delta_lut, a.gs = r.gs, a.mask = h->d_overlay_mask, a.param = h->overlay_param,
    a.init = h->overlay_init, a.param2 = h->overlay_param2;
    a.greedy = r.greedy, a.pi_thr = r.pi_thr, a.actions = r.actions;
    a.pos = r.pos, a.reward = r.reward, a.done = r.done, a.episode = r.episode, a.tcount = r.tcount, a.done_bits = r.done_bits;
    a.starts = r.starts, a.n_starts = r.n_starts, a.env_id0 = r.env_id0, a.seed_prefix = h->seed_prefix;
    a.tr_obs = p.traj ? r.tr_obs : nullptr, a.tr_reward = p.traj ? r.tr_reward : nullptr, a.tr_done = p.traj ? r.tr_done : nullptr;
    a.ret = p.stats ? r.ret : nullptr, a.episodes_fin = p.stats ? r.episodes_fin : nullptr;
    a.N = h->N, a.T = r.T, a.steps_taken = h->steps_taken, a.auto_reset = p.auto_mode ? 1 : 0;
    rollout[h->overlay](h, p, a);
}

// the overlay block of a learner launch (gu_td.hip), and the three planes in the place of the engine's two
void gu_overlay_lane_args(gu_engine *h, TabArgs &a, OverlayLaneArgs &o)
{
    o.param = h->overlay_param, o.param2 = h->overlay_param2, o.init = h->overlay_init, o.rows = h->td_S, o.word = h->d_overlay_mask;
    if (h->overlay) a.cell = h->d_overlay_cell;
}
