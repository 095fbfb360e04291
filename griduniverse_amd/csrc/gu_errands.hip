// gu_errands.hip -- errands for gfx950: ordered fruit-collection instructions, one per episode (include/gu.h: gu_set_errands; restated on
// the CPU by tests/_errands_oracle.py).  Errands are the fifth overlay kind (DESIGN.md "Overlays"): fruit's byte plane behind the engine's
// two cell planes, two engine-wide parameter words (the instructions, and the pay with the field widths: gu_map.hpp) and one uint32 word
// per env -- the fruit eaten, the progress p and the index j of the instruction the env was given at its last reset.  Here are the
// plane's and the instructions' validation, the words' reset kernel (it DRAWS: stream 11 at the episode count before the reset), the step
// kernel and the rollout kernel; the slot, the launches' arguments and everything else the overlays share is gu_overlay.hip's and
// gu_overlay.hpp's; the learners are instantiations of gu_td_kernel (gu_td.hip, through ErrandOverlay of gu_tabular_overlay.hpp).
//
// One lane per env, like the fruit kernels.  The three planes are staged in LDS where they fit 64 KiB, else all three are read from
// L2.  An errand never changes a move: the errand byte of the candidate cell is read BESIDE its flags and its reward byte, so the
// dependent chain of a step is the calm kernel's; a completed word keeps the cell behind the reads.  The word stays in a VGPR for the
// whole launch (one load, one store) beside `rem`, the env's instruction byte shifted right by 2p: the wanted kind is rem & 3 and
// "complete" is rem == 0, so no step indexes the instruction table.  The stream-11 hash sits in the reset branch only.
#include "gu_overlay.hpp"

#include <algorithm>
#include <vector>

// ------------------------------------------------------------------------------------
// the reset of the words: gu_reset and gu_reset_done, in front of gu_reset_kernel (which increments episode[])
// ------------------------------------------------------------------------------------
__global__ void __launch_bounds__(GU_BLOCK) gu_errands_reset_kernel(uint32_t *__restrict__ words, const uint8_t *__restrict__ mask, const int32_t *__restrict__ done,
                                                                     const uint32_t *__restrict__ episode, int32_t only_done, int64_t N, uint32_t seed_prefix,
                                                                     uint32_t env_id0, uint32_t instr, uint32_t q)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= N) return;
    bool take = !mask || mask[e];
    if (only_done && !done[e]) take = false;
    if (take) {
        uint32_t word, rem;
        gu_errand_draw(gu_rng_prefix(seed_prefix, env_id0 + (uint32_t)e), episode[e], instr, q, word, rem);
        words[e] = word;
    }
}

int gu_errands_before_reset(gu_engine *h, const uint8_t *d_mask, bool only_done)
{
    hipLaunchKernelGGL(gu_errands_reset_kernel, dim3(gu_blocks(h->N, GU_BLOCK)), dim3(GU_BLOCK), 0, h->stream, h->d_overlay_mask, d_mask, h->done(), h->d_episode,
                       only_done ? 1 : 0, h->N, h->seed_prefix, (uint32_t)h->env_id0, h->overlay_param, h->overlay_param2);
    GU_HIP(hipGetLastError());
    return GU_OK;
}

// ------------------------------------------------------------------------------------
// single step: gu_step_kernel's rules (rejected actions, lazy auto-reset, done ballot, host copies) with the errand of s'
// ------------------------------------------------------------------------------------
template <bool LDS>
__global__ void __launch_bounds__(GU_BLOCK) gu_errands_step_kernel(const OverlayStepArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const CellMap m = gu_stage_map<LDS>(a.cell, a.cell_bytes, smem, a.gs, 3);
    const uint8_t *er = m.f + 2 * a.cell_bytes;
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int32_t d = 0;
    if (e < a.N) {
        const uint32_t raw = (uint32_t)a.actions[e];
        const uint32_t act = raw & 3u;
        int32_t s = a.pos[e], r;
        if (a.host_err && !GU_ACTION_OK(raw)) {  // (gu_step_kernel: this env does not step, eats nothing, draws nothing, and the host is told)
            __hip_atomic_store(a.host_err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            a.tcount[e] -= 1u;
            r = a.reward[e];
            d = a.done[e];
        } else {
            uint32_t word = a.mask[e], rem;
            if ((a.flags & GU_F_AUTO_RESET) && a.done[e]) {  // lazy `if done: env.reset()`: the fruit grows back, another instruction is given
                const uint32_t ep = a.episode[e];
                const uint32_t start_prefix = gu_rng_prefix(a.seed_prefix, a.env_id0 + (uint32_t)e);
                s = a.starts[gu_rng_start_index(start_prefix, ep, a.n_starts)];
                a.episode[e] = ep + 1;
                gu_errand_draw(start_prefix, ep, a.param, a.param2, word, rem);
            } else {
                rem = gu_errand_rem(word, a.param, a.param2);
            }
            const int32_t c = gu_move(s, m.f[s], act, gu_delta<LDS>(act, a.lut, a.W));
            const bool stay = gu_errand_touch(er[c], m.r[c], (m.f[c] >> GU_CELL_TERM_BIT) & 1, a.param2, word, rem, r, d);
            s = stay ? s : c;
            a.pos[e] = s;
            a.reward[e] = r;
            a.done[e] = d;
            a.mask[e] = word;
        }
        if (a.host_obs) a.host_obs[e] = s;
        if (a.host_reward) a.host_reward[e] = r;
        if (a.host_done) a.host_done[e] = d;
    }
    const uint64_t bits = __ballot(d != 0);
    if ((threadIdx.x & 63) == 0 && e < a.N) a.done_bits[e >> 6] = bits;
    gu_step_publish(a.host_seq, a.seq, a.blocks_done);
}

void gu_errands_step(gu_engine *h, bool lds, const OverlayStepArgs &a)
{
    const dim3 grid(gu_blocks(h->N, GU_BLOCK)), block(GU_BLOCK);
    if (lds) hipLaunchKernelGGL(gu_errands_step_kernel<true>, grid, block, 3 * (size_t)h->cell_bytes, h->stream, a);
    else hipLaunchKernelGGL(gu_errands_step_kernel<false>, grid, block, 0, h->stream, a);
}

// ------------------------------------------------------------------------------------
// rollout: T steps per lane in one launch; the four policies with the calm kernels' action and sampling streams (0 and 2)
// ------------------------------------------------------------------------------------
template <int POLICY, bool LDS>
__global__ void __launch_bounds__(GU_BLOCK) gu_errands_rollout_kernel(const OverlayRolloutArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const CellMap m = gu_stage_map<LDS>(a.cell, a.cell_bytes, smem, a.gs, 3);
    const uint8_t *er = m.f + 2 * a.cell_bytes;
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int32_t d = 0;
    if (e < a.N) {
        const uint32_t env = a.env_id0 + (uint32_t)e;
        int32_t s = a.pos[e], r = a.reward[e];
        d = a.done[e];
        uint32_t ep = a.episode[e], word = a.mask[e];
        uint32_t rem = gu_errand_rem(word, a.param, a.param2);
        const uint64_t t0 = a.steps_taken + (uint64_t)(int64_t)(int32_t)a.tcount[e];
        const uint32_t start_prefix = gu_rng_prefix(a.seed_prefix, env);  // streams 1 and 11: no epoch
        OverlayPolicy<POLICY> P;
        P.begin(a, env, t0);
        int32_t ret = 0, fin = 0;
        for (int64_t i = 0; i < a.T; ++i) {
            if (a.auto_reset && d) {  // lazy `if done: env.reset()`: the fruit grows back, another instruction is given
                s = a.starts[gu_rng_start_index(start_prefix, ep, a.n_starts)];
                gu_errand_draw(start_prefix, ep, a.param, a.param2, word, rem);
                ++ep;
                d = 0;
            }
            const uint32_t act = P.act(a, i, e, s);
            const int32_t c = gu_move(s, m.f[s], act, gu_delta<LDS>(act, a.lut, a.W));
            // three reads behind the one address c: flags, reward byte, errand byte
            const bool stay = gu_errand_touch(er[c], m.r[c], (m.f[c] >> GU_CELL_TERM_BIT) & 1, a.param2, word, rem, r, d);
            s = stay ? s : c;
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
        a.mask[e] = word;
        if (a.ret) {
            a.ret[e] = ret;
            a.episodes_fin[e] = fin;
        }
    }
    const uint64_t bits = __ballot(d != 0);
    if ((threadIdx.x & 63) == 0 && e < a.N) a.done_bits[e >> 6] = bits;
}

void gu_errands_rollout(gu_engine *h, const GuRolloutPlan &p, const OverlayRolloutArgs &a)
{
    gu_pick<3, 2, 1, 0>(p.policy, [&](auto policy_c) {
        gu_pick<0, 1>(p.lds != 0, [&](auto lds_c) {
            constexpr int POLICY = decltype(policy_c)::value;
            constexpr bool LDS = decltype(lds_c)::value != 0;
            gu_lds_launch<gu_errands_rollout_kernel<POLICY, LDS>, false>(h, p.blocks, p.block, p.lds, a);
        });
    });
}

// ------------------------------------------------------------------------------------
// entry points
// ------------------------------------------------------------------------------------
// the length of instruction byte b, or -1 where a kind follows the end mark
static int gu_errand_length(uint32_t b)
{
    int L = 0;
    while (L < 4 && ((b >> (2 * L)) & 3u)) ++L;
    return (b >> (2 * L)) ? -1 : L;
}

static uint32_t gu_bit_length(uint32_t x)
{
    uint32_t n = 0;
    for (; x; x >>= 1) ++n;
    return n;
}

extern "C" {

int gu_set_errands(gu_handle h, const uint8_t *errand, int32_t n_instr, const uint8_t instr[4], const int32_t pay[3])
{
    GU_ENTER(h);
    GU_NEED_GRID(h);
    GU_TRY(gu_overlay_admits(h, GU_OVERLAY_ERRANDS));
    if (!errand) return gu_overlay_install(h, GU_OVERLAY_ERRANDS, nullptr, 0, 0u);
    GU_REQUIRE(instr != nullptr && pay != nullptr, GU_ERR_INVALID, "instr or pay is NULL");
    GU_REQUIRE(n_instr >= 1 && n_instr <= 4, GU_ERR_INVALID, "%d instructions (1 .. 4)", n_instr);
    // right in 0 .. 16, wrong in -16 .. 0, finish in 0 .. 16: a fruit cannot lie on a terminal cell, so the step that eats one pays the
    // cell's -1 beside right or wrong (|r| <= 17) and the completing step pays finish alone -- fruit's bound on a launch's int32 sum holds
    GU_REQUIRE(pay[0] >= 0 && pay[0] <= 16, GU_ERR_INVALID, "right = %d outside 0 .. 16", pay[0]);
    GU_REQUIRE(pay[1] >= -16 && pay[1] <= 0, GU_ERR_INVALID, "wrong = %d outside -16 .. 0", pay[1]);
    GU_REQUIRE(pay[2] >= 0 && pay[2] <= 16, GU_ERR_INVALID, "finish = %d outside 0 .. 16", pay[2]);
    std::vector<uint8_t> flags((size_t)h->S);
    GU_HIP(hipStreamSynchronize(h->stream));
    GU_HIP(hipMemcpy(flags.data(), h->d_cell, (size_t)h->S, hipMemcpyDeviceToHost));
    int32_t F = 0, of_kind[4] = {0, 0, 0, 0};
    uint32_t slots = 0;
    for (int32_t s = 0; s < h->S; ++s) {
        const uint32_t c = errand[s], kind = (c >> 5) & 3u, slot = c & 31u;
        if (!c) continue;
        GU_REQUIRE(!(c & 0x80u) && kind != 0u, GU_ERR_INVALID, "errand byte 0x%02x of cell %d: bit 7 must be zero, and kind 0 means the whole byte is zero", c, s);
        GU_REQUIRE(F < 8, GU_ERR_INVALID, "more than 8 fruits");
        GU_REQUIRE(!(flags[s] & (GU_CELL_WALL | GU_CELL_TERM)), GU_ERR_INVALID, "fruit on cell %d, which is a wall or a goal or lava cell", s);
        GU_REQUIRE(slot < 8u && !((slots >> slot) & 1u), GU_ERR_INVALID, "slot %u of cell %d is used twice or lies above 7", slot, s);
        slots |= 1u << slot;
        ++of_kind[kind];
        ++F;
    }
    GU_REQUIRE(F >= 1, GU_ERR_INVALID, "no fruit in the plane (NULL takes the errands away)");
    GU_REQUIRE(slots == (1u << F) - 1u, GU_ERR_INVALID, "the %d fruits must use the slots 0 .. %d, each once (slot mask 0x%02x)", F, F - 1, slots);
    uint32_t packed = 0, max_len = 0;
    for (int32_t j = 0; j < 4; ++j) {
        if (j >= n_instr) {
            GU_REQUIRE(instr[j] == 0, GU_ERR_INVALID, "instr[%d] = 0x%02x behind the %d instructions must be zero", j, instr[j], n_instr);
            continue;
        }
        const int L = gu_errand_length(instr[j]);
        GU_REQUIRE(L >= 1, GU_ERR_INVALID, "instr[%d] = 0x%02x: 1 .. 4 kinds in bits 2p .. 2p + 1, kind 0 ends the list and nothing follows it", j, instr[j]);
        int32_t named[4] = {0, 0, 0, 0};
        for (int p = 0; p < L; ++p) ++named[(instr[j] >> (2 * p)) & 3u];
        for (int k = 1; k < 4; ++k)
            GU_REQUIRE(named[k] <= of_kind[k], GU_ERR_INVALID, "instr[%d] names kind %d %d times and the plane holds %d of it: a fresh episode could not carry it out", j, k,
                       named[k], of_kind[k]);
        packed |= (uint32_t)instr[j] << (8 * j);
        max_len = std::max(max_len, (uint32_t)L);
    }
    const uint32_t pb = gu_bit_length(max_len), ib = gu_bit_length((uint32_t)n_instr - 1u);
    // every word starts as 0: instruction 0, nothing eaten
    return gu_overlay_install(h, GU_OVERLAY_ERRANDS, errand, F + (int32_t)(pb + ib), packed, 0u, GU_ERRAND_PARAM2(pay[0], pay[1], pay[2], F, pb, n_instr));
}

int gu_get_errands(gu_handle h, uint8_t *errand, int32_t *n_instr, uint8_t instr[4], int32_t pay[3], int32_t *n_fruit)
{
    GU_ENTER(h);
    GU_NEED_GRID(h);
    const bool set = h->overlay == GU_OVERLAY_ERRANDS;
    const uint32_t q = h->overlay_param2;
    if (n_instr) *n_instr = set ? (int32_t)GU_ERRAND_I(q) : 0;
    if (n_fruit) *n_fruit = set ? (int32_t)GU_ERRAND_F(q) : 0;
    for (int j = 0; instr && j < 4; ++j) instr[j] = set ? (uint8_t)(h->overlay_param >> (8 * j)) : 0;
    for (int k = 0; pay && k < 3; ++k) pay[k] = set ? (int32_t)(int8_t)(q >> (8 * k)) : 0;
    return errand ? gu_overlay_get_plane(h, GU_OVERLAY_ERRANDS, errand) : GU_OK;
}

int gu_get_errands_state(gu_handle h, int64_t env0, int64_t n, uint32_t *words)
{
    GU_ENTER(h);
    return gu_overlay_get_masks(h, GU_OVERLAY_ERRANDS, env0, n, words, "words");
}

int gu_set_errands_state(gu_handle h, int64_t env0, int64_t n, const uint32_t *words)
{
    GU_ENTER(h);
    // the fields of every word, before the slot's own checks (which refuse again a bit above the bits in use, with the same code)
    if (h->has_grid && h->overlay == GU_OVERLAY_ERRANDS && words && env0 >= 0 && n >= 0 && env0 + n <= h->N) {
        const uint32_t q = h->overlay_param2, F = GU_ERRAND_F(q), pb = GU_ERRAND_PB(q), I = GU_ERRAND_I(q);
        for (int64_t i = 0; i < n; ++i) {
            GU_REQUIRE((words[i] >> h->overlay_bits) == 0u, GU_ERR_INVALID, "words[%lld] = 0x%08x has a bit at or above the %d bits in use", (long long)i, words[i],
                       h->overlay_bits);
            const uint32_t p = (words[i] >> F) & ((1u << pb) - 1u), j = words[i] >> (F + pb);
            GU_REQUIRE(j < I, GU_ERR_INVALID, "words[%lld]: instruction %u of %u", (long long)i, j, I);
            const int L = gu_errand_length((h->overlay_param >> (8 * j)) & 0xFFu);
            GU_REQUIRE((int)p <= L, GU_ERR_INVALID, "words[%lld]: progress %u in instruction %u, which has %d entries", (long long)i, p, j, L);
        }
    }
    return gu_overlay_set_masks(h, GU_OVERLAY_ERRANDS, env0, n, words, "words");
}

}  // extern "C"
