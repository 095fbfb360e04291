// gu_errands.hip -- errands for gfx950: ordered fruit-collection instructions, one per episode (include/gu.h: gu_set_errands; restated on
// the CPU by tests/_errands_oracle.py).  Errands are the fifth overlay kind (DESIGN.md "Overlays"): fruit's byte plane behind the engine's
// two cell planes, two engine-wide parameter words (the instructions, and the pay with the field widths: gu_map.hpp) and one uint32 word
// per env -- the fruit eaten, the progress p and the index j of the instruction the env was given at its last reset.  Here are the
// instructions' validation, the words' reset kernel (it DRAWS: stream 11 at the episode count before the reset) and the errand rule,
// ErrandRule, around which gu_overlay.hpp's two frames are the step kernel and the rollout kernel; the slot, the launches' arguments,
// the plane's format (fruit's) and everything else the overlays share is gu_overlay.hip's and gu_overlay.hpp's; the learners are
// instantiations of gu_td_kernel (gu_td.hip, through ErrandOverlay of gu_tabular_overlay.hpp).
//
// One lane per env, like the fruit kernels.  The three planes are staged in LDS where they fit 64 KiB, else all three are read from
// L2.  An errand never changes a move: the errand byte of the candidate cell is read BESIDE its flags and its reward byte, so the
// dependent chain of a step is the calm kernel's; a completed word keeps the cell behind the reads.  The word stays in a VGPR for the
// whole launch (one load, one store) beside `rem`, the env's instruction byte shifted right by 2p: the wanted kind is rem & 3 and
// "complete" is rem == 0, so no step indexes the instruction table.  The stream-11 hash sits in the reset branch only.
#include "gu_overlay.hpp"

#include <algorithm>

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
// the rule (the interface: gu_overlay.hpp): the engine's move, and the errand byte of the candidate cell beside its flags and its reward byte
// ------------------------------------------------------------------------------------
struct ErrandRule {
    static constexpr bool DONE_IN_PLACE = true;  // (gu_overlay.hpp: its kernel handed d to the rule by reference)
    uint32_t w, rem;  // (`rem`: the head of this file)

    template <class ARGS>
    __device__ __forceinline__ void load(const ARGS &a, const OverlayMap &, uint32_t word, int32_t)
    {
        w = word;
        rem = gu_errand_rem(w, a.param, a.param2);
    }

    template <class ARGS>
    __device__ __forceinline__ void reset(const ARGS &a, const OverlayMap &, uint32_t start_prefix, uint32_t ep, int32_t)
    {
        gu_errand_draw(start_prefix, ep, a.param, a.param2, w, rem);  // the fruit grows back, another instruction is given
    }

    template <bool LDS, class ARGS>
    __device__ __forceinline__ void move(const ARGS &a, const OverlayMap &m, uint32_t act, int32_t &s, int32_t &r, int32_t &d)
    {
        const int32_t c = gu_move(s, m.f[s], act, gu_delta<LDS>(act, a.lut, a.W));
        // three reads behind the one address c: flags, reward byte, errand byte
        const bool stay = gu_errand_touch(m.o[c], m.r[c], (m.f[c] >> GU_CELL_TERM_BIT) & 1, a.param2, w, rem, r, d);
        s = stay ? s : c;
    }

    __device__ __forceinline__ uint32_t word() const { return w; }
};

void gu_errands_step(gu_engine *h, bool lds, const OverlayStepArgs &a) { gu_overlay_step_launch<ErrandRule>(h, lds, a); }
void gu_errands_rollout(gu_engine *h, const GuRolloutPlan &p, const OverlayRolloutArgs &a) { gu_overlay_rollout_launch<ErrandRule>(h, p, a); }

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
    int32_t F = 0, of_kind[4] = {0, 0, 0, 0};
    GU_TRY(gu_overlay_fruit_plane(h, GU_OVERLAY_ERRANDS, errand, 8, &F, of_kind));
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
