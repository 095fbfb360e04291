// gu_fruit.hip -- fruit for gfx950: collectable rewards, each eaten once per episode (include/gu.h: gu_set_fruit; restated on the
// CPU by tests/_fruit_oracle.py).  The fruit is an overlay (DESIGN.md "Overlays"): a third byte plane behind the engine's two cell
// planes (gu_engine::d_overlay_cell holds all three in one piece), three engine-wide values and one uint32 "eaten" mask per env
// (gu_engine::d_overlay_mask).  Here are the plane's validation, the fruit step kernel (gu_step, gu_step_device) and the fruit rollout
// kernel (gu_rollout); the slot, the launches' arguments, the masks and everything else the overlays share is gu_overlay.hip's and
// gu_overlay.hpp's; the fruit learners are instantiations of gu_td_kernel (gu_td.hip, through FruitOverlay of gu_tabular_overlay.hpp).
//
// One lane per env, like the calm kernels.  The three planes are staged in LDS where they fit 64 KiB (gu_lds_block(h, bs, 3)),
// else all three are read from L2.  Fruit never changes a move: the fruit byte of s' is read BESIDE the flags and the reward byte of
// s' (three independent reads behind one address), so the dependent chain of a step is as long as the calm kernel's.  The mask
// stays in a VGPR for the whole launch: one load at the start, one store at the end.  Plain stores, no schedule (GuPacer).
#include "gu_overlay.hpp"

#include <algorithm>
#include <vector>

// ------------------------------------------------------------------------------------
// single step: gu_step_kernel's rules (rejected actions, lazy auto-reset, done ballot, host copies) with the fruit of s'
// ------------------------------------------------------------------------------------
template <bool LDS>
__global__ void __launch_bounds__(GU_BLOCK) gu_fruit_step_kernel(const OverlayStepArgs a)
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
            uint32_t eaten = a.mask[e];
            if ((a.flags & GU_F_AUTO_RESET) && a.done[e]) {  // lazy `if done: env.reset()`: the fruit grows back
                const uint32_t ep = a.episode[e];
                s = a.starts[gu_rng_start_index(gu_rng_prefix(a.seed_prefix, a.env_id0 + (uint32_t)e), ep, a.n_starts)];
                a.episode[e] = ep + 1;
                eaten = 0u;
            }
            s = gu_move(s, m.f[s], act, gu_delta<LDS>(act, a.lut, a.W));
            r = m.r[s] + gu_fruit_eat(fr[s], a.param, eaten);
            d = (m.f[s] >> GU_CELL_TERM_BIT) & 1;
            a.pos[e] = s;
            a.reward[e] = r;
            a.done[e] = d;
            a.mask[e] = eaten;
        }
        if (a.host_obs) a.host_obs[e] = s;
        if (a.host_reward) a.host_reward[e] = r;
        if (a.host_done) a.host_done[e] = d;
    }
    const uint64_t bits = __ballot(d != 0);
    if ((threadIdx.x & 63) == 0 && e < a.N) a.done_bits[e >> 6] = bits;
    gu_step_publish(a.host_seq, a.seq, a.blocks_done);
}

void gu_fruit_step(gu_engine *h, bool lds, const OverlayStepArgs &a)
{
    const dim3 grid(gu_blocks(h->N, GU_BLOCK)), block(GU_BLOCK);
    if (lds) hipLaunchKernelGGL(gu_fruit_step_kernel<true>, grid, block, 3 * (size_t)h->cell_bytes, h->stream, a);
    else hipLaunchKernelGGL(gu_fruit_step_kernel<false>, grid, block, 0, h->stream, a);
}

// ------------------------------------------------------------------------------------
// rollout: T steps per lane in one launch; the four policies with the calm kernels' action and sampling streams (0 and 2)
// ------------------------------------------------------------------------------------
// Auto-reset, rows and statistics are launch-uniform tests on the arguments.  The step count is 64 bits wide and streams 0 and 2 are
// re-keyed in the step that crosses a multiple of 2^32, so no launch needs another form.
template <int POLICY, bool LDS>
__global__ void __launch_bounds__(GU_BLOCK) gu_fruit_rollout_kernel(const OverlayRolloutArgs a)
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
        uint32_t ep = a.episode[e], eaten = a.mask[e];
        const uint64_t t0 = a.steps_taken + (uint64_t)(int64_t)(int32_t)a.tcount[e];
        const uint32_t start_prefix = gu_rng_prefix(a.seed_prefix, env);  // stream 1: no epoch
        OverlayPolicy<POLICY> P;
        P.begin(a, env, t0);
        int32_t ret = 0, fin = 0;
        for (int64_t i = 0; i < a.T; ++i) {
            if (a.auto_reset && d) {  // lazy `if done: env.reset()`: the fruit grows back
                s = a.starts[gu_rng_start_index(start_prefix, ep, a.n_starts)];
                ++ep;
                d = 0;
                eaten = 0u;
            }
            const uint32_t act = P.act(a, i, e, s);
            s = gu_move(s, m.f[s], act, gu_delta<LDS>(act, a.lut, a.W));
            // three reads behind the one address s': flags, reward byte, fruit byte
            r = m.r[s] + gu_fruit_eat(fr[s], a.param, eaten);
            d = (m.f[s] >> GU_CELL_TERM_BIT) & 1;
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
        a.mask[e] = eaten;
        if (a.ret) {
            a.ret[e] = ret;
            a.episodes_fin[e] = fin;
        }
    }
    const uint64_t bits = __ballot(d != 0);
    if ((threadIdx.x & 63) == 0 && e < a.N) a.done_bits[e >> 6] = bits;
}

void gu_fruit_rollout(gu_engine *h, const GuRolloutPlan &p, const OverlayRolloutArgs &a)
{
    gu_pick<3, 2, 1, 0>(p.policy, [&](auto policy_c) {
        gu_pick<0, 1>(p.lds != 0, [&](auto lds_c) {
            constexpr int POLICY = decltype(policy_c)::value;
            constexpr bool LDS = decltype(lds_c)::value != 0;
            gu_lds_launch<gu_fruit_rollout_kernel<POLICY, LDS>, false>(h, p.blocks, p.block, p.lds, a);
        });
    });
}

// ------------------------------------------------------------------------------------
// entry points
// ------------------------------------------------------------------------------------
extern "C" {

int gu_set_fruit(gu_handle h, const uint8_t *fruit, const int32_t value[3])
{
    GU_ENTER(h);
    GU_NEED_GRID(h);
    GU_TRY(gu_overlay_admits(h, GU_OVERLAY_FRUIT));
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
    uint32_t values = 0;  // four int8 bytes, byte 0 (kind 0: no fruit) zero
    for (int k = 0; fruit && k < 3; ++k) values |= (uint32_t)(uint8_t)(int8_t)value[k] << (8 * (k + 1));
    GU_TRY(gu_overlay_install(h, GU_OVERLAY_FRUIT, fruit, F, values));
    if (fruit) std::copy(value, value + 3, h->fruit_value);  // (gu_overlay_free has zeroed them)
    return GU_OK;
}

int gu_get_fruit(gu_handle h, uint8_t *fruit, int32_t value[3], int32_t *n_fruit)
{
    GU_ENTER(h);
    GU_NEED_GRID(h);
    if (n_fruit) *n_fruit = h->overlay == GU_OVERLAY_FRUIT ? h->overlay_bits : 0;
    if (value) std::copy(h->fruit_value, h->fruit_value + 3, value);
    return fruit ? gu_overlay_get_plane(h, GU_OVERLAY_FRUIT, fruit) : GU_OK;
}

int gu_get_fruit_state(gu_handle h, int64_t env0, int64_t n, uint32_t *eaten)
{
    GU_ENTER(h);
    return gu_overlay_get_masks(h, GU_OVERLAY_FRUIT, env0, n, eaten, "eaten");
}

int gu_set_fruit_state(gu_handle h, int64_t env0, int64_t n, const uint32_t *eaten)
{
    GU_ENTER(h);
    return gu_overlay_set_masks(h, GU_OVERLAY_FRUIT, env0, n, eaten, "eaten");
}

}  // extern "C"
