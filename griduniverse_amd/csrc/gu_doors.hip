// gu_doors.hip -- doors, keys and levers for gfx950: the first feature whose move rule depends on the lane's own bits of state
// (include/gu.h: gu_set_doors; restated on the CPU by tests/_doors_oracle.py).  The doors are an overlay (DESIGN.md "Overlays"): a
// third byte plane behind the engine's two cell planes (gu_engine::d_overlay_cell holds all three in one piece) and one uint32 mask of
// open slots per env (gu_engine::d_overlay_mask).  Here are the plane's validation, the door step kernel (gu_step, gu_step_device) and
// the door rollout kernel (gu_rollout); the slot, the launches' arguments, the masks and everything else the overlays share is
// gu_overlay.hip's and gu_overlay.hpp's; the door learners are instantiations of gu_td_kernel (gu_td.hip, through DoorOverlay of
// gu_tabular_overlay.hpp).
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
// learners' lane (DoorOverlay::move, gu_tabular_overlay.hpp) gates the same way, with the bytes of s read beside each other instead of carried.
// The step kernel takes one step per launch and reads door[c] behind the candidate, as the rule is written.
//
// One lane per env.  The mask stays in a VGPR for the whole launch: one load at the start, one store at the end.  Plain stores, no
// schedule (GuPacer).
#include "gu_overlay.hpp"

#include <algorithm>
#include <vector>

// ------------------------------------------------------------------------------------
// single step: gu_step_kernel's rules (rejected actions, lazy auto-reset, done ballot, host copies) behind the gate of the candidate cell
// ------------------------------------------------------------------------------------
template <bool LDS>
__global__ void __launch_bounds__(GU_BLOCK) gu_doors_step_kernel(const OverlayStepArgs a)
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
            uint32_t open = a.mask[e];
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
            a.mask[e] = open;
        }
        if (a.host_obs) a.host_obs[e] = s;
        if (a.host_reward) a.host_reward[e] = r;
        if (a.host_done) a.host_done[e] = d;
    }
    const uint64_t bits = __ballot(d != 0);
    if ((threadIdx.x & 63) == 0 && e < a.N) a.done_bits[e >> 6] = bits;
    gu_step_publish(a.host_seq, a.seq, a.blocks_done);
}

void gu_doors_step(gu_engine *h, bool lds, const OverlayStepArgs &a)
{
    const dim3 grid(gu_blocks(h->N, GU_BLOCK)), block(GU_BLOCK);
    if (lds) hipLaunchKernelGGL(gu_doors_step_kernel<true>, grid, block, 3 * (size_t)h->cell_bytes, h->stream, a);
    else hipLaunchKernelGGL(gu_doors_step_kernel<false>, grid, block, 0, h->stream, a);
}

// ------------------------------------------------------------------------------------
// rollout: T steps per lane in one launch; the four policies with the calm kernels' streams 0, 1 and 2
// ------------------------------------------------------------------------------------
// Auto-reset, rows and statistics are launch-uniform tests on the arguments.  The step count is 64 bits wide and streams 0 and 2 are
// re-keyed in the step that crosses a multiple of 2^32, so no launch needs another form.
template <int POLICY, bool LDS>
__global__ void __launch_bounds__(GU_BLOCK) gu_doors_rollout_kernel(const OverlayRolloutArgs a)
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
        uint32_t ep = a.episode[e], open = a.mask[e];
        uint32_t fs = m.f[s];   // the flags and the reward byte of the cell stood on, carried from step to step (the head of this file)
        int32_t rs = m.r[s];
        const uint64_t t0 = a.steps_taken + (uint64_t)(int64_t)(int32_t)a.tcount[e];
        const uint32_t start_prefix = gu_rng_prefix(a.seed_prefix, env);  // stream 1: no epoch
        OverlayPolicy<POLICY> P;
        P.begin(a, env, t0);
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
            const uint32_t act = P.act(a, i, e, s);
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
        a.mask[e] = open;
        if (a.ret) {
            a.ret[e] = ret;
            a.episodes_fin[e] = fin;
        }
    }
    const uint64_t bits = __ballot(d != 0);
    if ((threadIdx.x & 63) == 0 && e < a.N) a.done_bits[e >> 6] = bits;
}

void gu_doors_rollout(gu_engine *h, const GuRolloutPlan &p, const OverlayRolloutArgs &a)
{
    gu_pick<3, 2, 1, 0>(p.policy, [&](auto policy_c) {
        gu_pick<0, 1>(p.lds != 0, [&](auto lds_c) {
            constexpr int POLICY = decltype(policy_c)::value;
            constexpr bool LDS = decltype(lds_c)::value != 0;
            gu_lds_launch<gu_doors_rollout_kernel<POLICY, LDS>, false>(h, p.blocks, p.block, p.lds, a);
        });
    });
}

// ------------------------------------------------------------------------------------
// entry points
// ------------------------------------------------------------------------------------
extern "C" {

int gu_set_doors(gu_handle h, const uint8_t *door)
{
    GU_ENTER(h);
    GU_NEED_GRID(h);
    GU_TRY(gu_overlay_admits(h, GU_OVERLAY_DOORS));
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
    return gu_overlay_install(h, GU_OVERLAY_DOORS, door, D, 0u);
}

int gu_get_doors(gu_handle h, uint8_t *door, int32_t *n_slots)
{
    GU_ENTER(h);
    GU_NEED_GRID(h);
    if (n_slots) *n_slots = h->overlay == GU_OVERLAY_DOORS ? h->overlay_bits : 0;
    return door ? gu_overlay_get_plane(h, GU_OVERLAY_DOORS, door) : GU_OK;
}

int gu_get_doors_state(gu_handle h, int64_t env0, int64_t n, uint32_t *open)
{
    GU_ENTER(h);
    return gu_overlay_get_masks(h, GU_OVERLAY_DOORS, env0, n, open, "open");
}

int gu_set_doors_state(gu_handle h, int64_t env0, int64_t n, const uint32_t *open)
{
    GU_ENTER(h);
    return gu_overlay_set_masks(h, GU_OVERLAY_DOORS, env0, n, open, "open");
}

}  // extern "C"
