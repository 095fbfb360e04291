// gu_wind.hip -- wind for gfx950: per-cell pushes with gusts (include/gu.h: gu_set_wind; restated on the CPU by tests/_wind_oracle.py).
// The wind is an overlay (DESIGN.md "Overlays"): a third byte plane behind the engine's two cell planes, gu_engine::d_overlay_cell
// holds all three in one piece.  A step is the engine's move followed by up to four more moves in the wind's direction
// (gu_map.hpp: gu_wind_push).  Here are the
// plane's validation, the windy step kernel (gu_step, gu_step_device) and the windy rollout kernel (gu_rollout); the slot, the launches'
// arguments and everything else the overlays share is gu_overlay.hip's and gu_overlay.hpp's; the windy learners are instantiations
// of gu_td_kernel (gu_td.hip, through WindOverlay of gu_tabular_overlay.hpp).
//
// One lane per env, like the calm kernels.  The three planes are staged in LDS where they fit 64 KiB (gu_lds_block(h, bs, 3)),
// else all three are read from L2.  A windy step is a chain of 2 + k dependent plane reads (the wind byte and the flags of the
// cell left, the flags behind every push) instead of one, so these kernels are bound by that latency, not by the store stream:
// they keep no schedule (GuPacer) and do not depend on where the trajectory buffer lies.
#include "gu_overlay.hpp"

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
template <bool LDS, bool GUST>
__global__ void __launch_bounds__(GU_BLOCK) gu_wind_step_kernel(const OverlayStepArgs a)
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
        const int32_t s2 = gu_wind_move<LDS, GUST>(m, wd, (live && ok) ? s : 0, raw & 3u, prefix, t, a.param, a.lut, a.W);
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
    gu_step_publish(a.host_seq, a.seq, a.blocks_done);
}

void gu_wind_step(gu_engine *h, bool lds, const OverlayStepArgs &a)
{
    const dim3 grid(gu_blocks(h->N, GU_BLOCK)), block(GU_BLOCK);
    const size_t bytes = lds ? 3 * (size_t)h->cell_bytes : 0;
    if (lds && a.param) hipLaunchKernelGGL((gu_wind_step_kernel<true, true>), grid, block, bytes, h->stream, a);
    else if (lds) hipLaunchKernelGGL((gu_wind_step_kernel<true, false>), grid, block, bytes, h->stream, a);
    else if (a.param) hipLaunchKernelGGL((gu_wind_step_kernel<false, true>), grid, block, 0, h->stream, a);
    else hipLaunchKernelGGL((gu_wind_step_kernel<false, false>), grid, block, 0, h->stream, a);
}

// ------------------------------------------------------------------------------------
// rollout: T windy steps per lane in one launch; the four policies with the calm kernels' action and sampling streams (0 and 2)
// ------------------------------------------------------------------------------------
// GUST is a template parameter: the calm-gust instantiations carry no stream-9 hash.  Auto-reset, rows and statistics are
// launch-uniform tests on the arguments (a windy step is a chain of dependent plane reads: the tests hide behind it).
template <int POLICY, bool LDS, bool GUST>
__global__ void __launch_bounds__(GU_BLOCK) gu_wind_rollout_kernel(const OverlayRolloutArgs a)
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
    const uint64_t t0 = a.steps_taken + (uint64_t)(int64_t)(int32_t)a.tcount[el];
    const uint32_t start_prefix = gu_rng_prefix(a.seed_prefix, env);  // stream 1: no epoch
    OverlayPolicy<POLICY> P;  // (its prefix is stream 9's too)
    P.begin(a, env, t0);
    int32_t ret = 0, fin = 0;
    for (int64_t i = 0; i < a.T; ++i) {
        if (a.auto_reset && d) {  // lazy `if done: env.reset()`
            s = a.starts[gu_rng_start_index(start_prefix, ep, a.n_starts)];
            ++ep;
            d = 0;
        }
        const uint32_t act = P.act(a, i, el, s);
        s = gu_wind_move<LDS, GUST>(m, wd, s, act, P.prefix, P.t, a.param, a.lut, a.W);
        r = m.r[s];
        d = (m.f[s] >> GU_CELL_TERM_BIT) & 1;
        P.next(a);
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

// (the lists run backwards so that the kernels keep their order in the code object: an unchanged binary is how a change here is checked)
void gu_wind_rollout(gu_engine *h, const GuRolloutPlan &p, const OverlayRolloutArgs &a)
{
    gu_pick<3, 2, 1, 0>(p.policy, [&](auto policy_c) {
        gu_pick<0, 1>(p.lds != 0, [&](auto lds_c) {
            gu_pick<0, 1>(a.param != 0, [&](auto gust_c) {
                constexpr int POLICY = decltype(policy_c)::value;
                constexpr bool LDS = decltype(lds_c)::value != 0, GUST = decltype(gust_c)::value != 0;
                gu_lds_launch<gu_wind_rollout_kernel<POLICY, LDS, GUST>, false>(h, p.blocks, p.block, p.lds, a);
            });
        });
    });
}

// ------------------------------------------------------------------------------------
// entry points
// ------------------------------------------------------------------------------------
extern "C" {

int gu_set_wind(gu_handle h, const uint8_t *wind, uint32_t gust_q16)
{
    GU_ENTER(h);
    GU_NEED_GRID(h);
    GU_TRY(gu_overlay_admits(h, GU_OVERLAY_WIND));
    GU_REQUIRE(gust_q16 <= 65536u, GU_ERR_INVALID, "gust_q16 %u above 65536", gust_q16);
    if (wind)
        for (int32_t s = 0; s < h->S; ++s)
            GU_REQUIRE((wind[s] & 0xF0u) == 0, GU_ERR_INVALID, "wind byte 0x%02x of cell %d: bits 4 .. 7 must be zero", wind[s], s);
    return gu_overlay_install(h, GU_OVERLAY_WIND, wind, 0, gust_q16);
}

int gu_get_wind(gu_handle h, uint8_t *wind, uint32_t *gust_q16, int32_t *present)
{
    GU_ENTER(h);
    GU_NEED_GRID(h);
    const bool set = h->overlay == GU_OVERLAY_WIND;
    if (present) *present = set ? 1 : 0;
    if (gust_q16) *gust_q16 = set ? h->overlay_param : 0u;
    return wind ? gu_overlay_get_plane(h, GU_OVERLAY_WIND, wind) : GU_OK;
}

}  // extern "C"
