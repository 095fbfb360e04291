// gu_boxes.hip -- pushable boxes (Sokoban) for gfx950: the first feature whose per-env state is a set of POSITIONS that the agent's own
// moves rewrite (include/gu.h: gu_set_boxes; restated on the CPU by tests/_boxes_oracle.py).  The boxes are an overlay (DESIGN.md
// "Overlays"): a third byte plane behind the engine's two cell planes (bit 0: target, bit 1: a box stands here at every reset) and one
// uint32 word per env (gu_engine::d_overlay_mask) that holds the cell of box k in bits [k * b, (k + 1) * b).  Here are the plane's and
// the words' validation, the box step kernel (gu_step, gu_step_device) and the box rollout kernel (gu_rollout); the slot, the launches'
// arguments, the words' copies and resets are gu_overlay.hip's and gu_overlay.hpp's; the field arithmetic and the push are gu_map.hpp's
// (gu_box_at, gu_box_push), shared with the learners' lane (BoxOverlay, gu_tabular_overlay.hpp; gu_td.hip instantiates it).
//
// THE HOT PATH, decided on purpose (none of it is measured beside an alternative: only the form below was built; what is measured is
// this kernel beside the doors kernel of the same shape, tools/boxes_rate.py).
//   "Does a box stand on c" is B field extractions (shift, and) and compares against c, selects and no branch: 3 B VALU operations on
//   the step's chain behind the candidate.  B and b are launch-uniform (the parameter word), so the loop over the boxes is a scalar
//   loop of at most five trips (eight on sixteen cells), run by every lane, with no branch of its own.  A per-cell occupancy plane would make it one read, but the plane would be per ENV.
//   THE PUSH is a second dependent round of LDS reads -- flags[c2] and box[c2] behind c2, which is behind flags[c] -- that only a
//   push needs.  It sits behind a branch on "this lane pushes", which the compiler turns into a mask of the pushing lanes and a skip
//   where the mask is empty: a wave in which nobody pushes pays the B compares, one test of the mask and one untaken scalar branch
//   -- what wind's ballot-and-branch pays --, and a wave with one pushing lane pays the round for all.  Away from the boxes that is
//   every step, so the loop keeps the doors kernel's ONE round of reads: like that kernel (the head of gu_doors.hip) the rollout
//   carries the flags and the reward byte of the cell stood on in VGPRs and reads the candidate's three bytes together.  Inside the
//   push the two bytes of c2 are read together and the three refusals are or-ed without a short circuit (gu_box_push), so a pushing
//   wave has ONE more round, not one per test.  Read in the compiled gfx950 code of the rollout kernels: behind the three reads of c
//   and the scalar loop of compares, one exec-mask skip around the push, and inside it two LDS reads and the second scalar loop.
//   SOLVED is a carried count: `on`, the number of boxes on a target, lives in a VGPR beside the word; a push adds target[c2] -
//   target[c], which the push round holds anyway, and solved is on == B: one compare per step instead of B reads.  The count is
//   derived from the word with B reads once, at the start of the launch; behind a lazy reset it is the count of the reset word, a
//   launch-uniform constant that the host works out (it travels in the parameter word).  Cost: one VGPR.
//   A solved word is absorbing without a branch: the step is computed as ever and a select keeps s and w.
// The step kernel takes one step per launch: it derives the count with its B reads and carries nothing.
//
// One lane per env.  The word stays in a VGPR for the whole launch: one load at the start, one store at the end.  Plain stores, no
// schedule (GuPacer).
#include "gu_overlay.hpp"

#include <algorithm>
#include <vector>

// One step of rules 2 .. 6 of gu_set_boxes from cell s (flags fs, reward byte rs) under the word w with `on` boxes on a target:
// leaves s', its two bytes, w' and the count in place and returns the reward; d is the done flag.  `m` and `bx` are the staged planes.
template <bool LDS>
__device__ __forceinline__ int32_t gu_boxes_move(const CellMap &m, const uint8_t *bx, uint32_t param, uint32_t act, uint64_t lut, int32_t W, int32_t &s, uint32_t &fs,
                                                 int32_t &rs, uint32_t &w, uint32_t &on, int32_t &d)
{
    const uint32_t B = GU_BOX_B(param), b = GU_BOX_BITS(param);
    const int32_t delta = gu_delta<LDS>(act, lut, W);
    const bool solved = on == B;  // rule 2: nothing moves
    const int32_t c = gu_move(s, fs, act, delta);
    // three reads behind the one address c: flags, reward byte, box byte
    const uint32_t fc = m.f[c], bc = bx[c];
    const int32_t rc = m.r[c];
    const int32_t at = gu_box_at(w, c, B, b);  // (computed for every lane: selects, no branch of its own)
    const int32_t k = ((c != s) & !solved) ? at : -1;
    bool stay = solved;
    int32_t gain = 0;
    if (k >= 0) stay = gu_box_push(m.f, bx, c, fc, bc, act, delta, k, B, b, w, gain);  // the second round: pushing lanes only
    s = stay ? s : c;
    fs = stay ? fs : fc;
    rs = stay ? rs : rc;
    on += (uint32_t)gain;
    const bool done = on == B;
    d = done ? 1 : (int32_t)(fs >> GU_CELL_TERM_BIT) & 1;
    return done ? GU_BOX_SOLVED_REWARD : rs + GU_BOX_V(param) * gain;
}

// ------------------------------------------------------------------------------------
// single step: gu_step_kernel's rules (rejected actions, lazy auto-reset, done ballot, host copies) around the box rule
// ------------------------------------------------------------------------------------
template <bool LDS>
__global__ void __launch_bounds__(GU_BLOCK) gu_boxes_step_kernel(const OverlayStepArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const CellMap m = gu_stage_map<LDS>(a.cell, a.cell_bytes, smem, a.gs, 3);
    const uint8_t *bx = m.f + 2 * a.cell_bytes;
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int32_t d = 0;
    if (e < a.N) {
        const uint32_t raw = (uint32_t)a.actions[e];
        const uint32_t act = raw & 3u;
        int32_t s = a.pos[e], r;
        if (a.host_err && !GU_ACTION_OK(raw)) {  // (gu_step_kernel: this env does not step, its word stays, and the host is told)
            __hip_atomic_store(a.host_err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            a.tcount[e] -= 1u;
            r = a.reward[e];
            d = a.done[e];
        } else {
            uint32_t w = a.mask[e];
            if ((a.flags & GU_F_AUTO_RESET) && a.done[e]) {  // lazy `if done: env.reset()`: the boxes are back where they began
                const uint32_t ep = a.episode[e];
                s = a.starts[gu_rng_start_index(gu_rng_prefix(a.seed_prefix, a.env_id0 + (uint32_t)e), ep, a.n_starts)];
                a.episode[e] = ep + 1;
                w = a.init;
            }
            uint32_t fs = m.f[s], on = gu_box_on_target(bx, w, GU_BOX_B(a.param), GU_BOX_BITS(a.param));
            int32_t rs = m.r[s];
            r = gu_boxes_move<LDS>(m, bx, a.param, act, a.lut, a.W, s, fs, rs, w, on, d);
            a.pos[e] = s;
            a.reward[e] = r;
            a.done[e] = d;
            a.mask[e] = w;
        }
        if (a.host_obs) a.host_obs[e] = s;
        if (a.host_reward) a.host_reward[e] = r;
        if (a.host_done) a.host_done[e] = d;
    }
    const uint64_t bits = __ballot(d != 0);
    if ((threadIdx.x & 63) == 0 && e < a.N) a.done_bits[e >> 6] = bits;
    gu_step_publish(a.host_seq, a.seq, a.blocks_done);
}

void gu_boxes_step(gu_engine *h, bool lds, const OverlayStepArgs &a)
{
    const dim3 grid(gu_blocks(h->N, GU_BLOCK)), block(GU_BLOCK);
    if (lds) hipLaunchKernelGGL(gu_boxes_step_kernel<true>, grid, block, 3 * (size_t)h->cell_bytes, h->stream, a);
    else hipLaunchKernelGGL(gu_boxes_step_kernel<false>, grid, block, 0, h->stream, a);
}

// ------------------------------------------------------------------------------------
// rollout: T steps per lane in one launch; the four policies with the calm kernels' streams 0, 1 and 2
// ------------------------------------------------------------------------------------
// Auto-reset, rows and statistics are launch-uniform tests on the arguments.  The step count is 64 bits wide and streams 0 and 2 are
// re-keyed in the step that crosses a multiple of 2^32, so no launch needs another form.
template <int POLICY, bool LDS>
__global__ void __launch_bounds__(GU_BLOCK) gu_boxes_rollout_kernel(const OverlayRolloutArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const CellMap m = gu_stage_map<LDS>(a.cell, a.cell_bytes, smem, a.gs, 3);
    const uint8_t *bx = m.f + 2 * a.cell_bytes;
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int32_t d = 0;
    if (e < a.N) {
        const uint32_t env = a.env_id0 + (uint32_t)e;
        int32_t s = a.pos[e], r = a.reward[e];
        d = a.done[e];
        uint32_t ep = a.episode[e], w = a.mask[e];
        uint32_t fs = m.f[s];  // the flags and the reward byte of the cell stood on, and the count of boxes on a target, carried from step to step
        int32_t rs = m.r[s];
        uint32_t on = gu_box_on_target(bx, w, GU_BOX_B(a.param), GU_BOX_BITS(a.param));
        const uint64_t t0 = a.steps_taken + (uint64_t)(int64_t)(int32_t)a.tcount[e];
        const uint32_t start_prefix = gu_rng_prefix(a.seed_prefix, env);  // stream 1: no epoch
        OverlayPolicy<POLICY> P;
        P.begin(a, env, t0);
        int32_t ret = 0, fin = 0;
        for (int64_t i = 0; i < a.T; ++i) {
            if (a.auto_reset && d) {  // lazy `if done: env.reset()`: the boxes are back where they began
                s = a.starts[gu_rng_start_index(start_prefix, ep, a.n_starts)];
                ++ep;
                w = a.init;
                on = GU_BOX_ON0(a.param);
                fs = m.f[s];
                rs = m.r[s];
            }
            const uint32_t act = P.act(a, i, e, s);
            r = gu_boxes_move<LDS>(m, bx, a.param, act, a.lut, a.W, s, fs, rs, w, on, d);
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
        a.mask[e] = w;
        if (a.ret) {
            a.ret[e] = ret;
            a.episodes_fin[e] = fin;
        }
    }
    const uint64_t bits = __ballot(d != 0);
    if ((threadIdx.x & 63) == 0 && e < a.N) a.done_bits[e >> 6] = bits;
}

void gu_boxes_rollout(gu_engine *h, const GuRolloutPlan &p, const OverlayRolloutArgs &a)
{
    gu_pick<3, 2, 1, 0>(p.policy, [&](auto policy_c) {
        gu_pick<0, 1>(p.lds != 0, [&](auto lds_c) {
            constexpr int POLICY = decltype(policy_c)::value;
            constexpr bool LDS = decltype(lds_c)::value != 0;
            gu_lds_launch<gu_boxes_rollout_kernel<POLICY, LDS>, false>(h, p.blocks, p.block, p.lds, a);
        });
    });
}

// ------------------------------------------------------------------------------------
// entry points
// ------------------------------------------------------------------------------------
// the flags plane of the engine's grid on the host (wall and terminal bits: what neither a box nor a target may lie on)
static int gu_boxes_flags(gu_engine *h, std::vector<uint8_t> &flags)
{
    flags.resize((size_t)h->S);
    GU_HIP(hipStreamSynchronize(h->stream));
    GU_HIP(hipMemcpy(flags.data(), h->d_cell, (size_t)h->S, hipMemcpyDeviceToHost));
    return GU_OK;
}

static int32_t gu_boxes_width(int32_t S)  // the smallest b with S <= 1 << b (at least 1)
{
    int32_t b = 1;
    while (((int64_t)1 << b) < S) ++b;
    return b;
}

extern "C" {

int gu_set_boxes(gu_handle h, const uint8_t *box, int32_t on_target)
{
    GU_ENTER(h);
    GU_NEED_GRID(h);
    GU_TRY(gu_overlay_admits(h, GU_OVERLAY_BOXES));
    if (!box) return gu_overlay_install(h, GU_OVERLAY_BOXES, nullptr, 0, 0u);
    GU_REQUIRE(on_target >= 0 && on_target <= 16, GU_ERR_INVALID, "on_target %d out of range (0 .. 16)", on_target);
    std::vector<uint8_t> flags;
    GU_TRY(gu_boxes_flags(h, flags));
    std::vector<int32_t> starts((size_t)h->n_starts);
    GU_HIP(hipMemcpy(starts.data(), h->d_starts, starts.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    const int32_t b = gu_boxes_width(h->S);
    int32_t B = 0, targets = 0, on0 = 0;
    uint64_t init = 0;
    for (int32_t s = 0; s < h->S; ++s) {
        const uint32_t c = box[s];
        if (!c) continue;
        GU_REQUIRE(!(c & ~(GU_BOX_TARGET | GU_BOX_INITIAL)), GU_ERR_INVALID, "box byte 0x%02x of cell %d: bit 0 is a target, bit 1 a box, bits 2 .. 7 must be zero", c, s);
        GU_REQUIRE(!(flags[s] & (GU_CELL_WALL | GU_CELL_TERM)), GU_ERR_INVALID, "a box or target on cell %d, which is a wall or a goal or lava cell", s);
        if (c & GU_BOX_TARGET) ++targets;
        if (c & GU_BOX_INITIAL) {
            GU_REQUIRE(std::find(starts.begin(), starts.end(), s) == starts.end(), GU_ERR_INVALID, "a box on cell %d, which is a start cell", s);
            GU_REQUIRE((B + 1) * b <= 32, GU_ERR_INVALID, "more than %d boxes of %d bits each (%d cells): an env's word has 32 bits", 32 / b, b, h->S);
            init |= (uint64_t)s << (B * b);  // box k, by ascending cell, in bits [k * b, (k + 1) * b)
            ++B;
            if (c & GU_BOX_TARGET) ++on0;
        }
    }
    GU_REQUIRE(B >= 1, GU_ERR_INVALID, "no box in the plane (NULL takes the boxes away)");
    GU_REQUIRE(targets >= B, GU_ERR_INVALID, "%d targets for %d boxes: every box needs a target", targets, B);
    GU_REQUIRE(on0 < B, GU_ERR_INVALID, "every box stands on a target: an env would be born solved");
    GU_TRY(gu_overlay_install(h, GU_OVERLAY_BOXES, box, b * B, GU_BOX_PARAM(on_target, B, b, on0), (uint32_t)init));
    h->box_flags = std::move(flags);  // (the grid cannot change under the boxes: a new grid drops them)
    return GU_OK;
}

int gu_get_boxes(gu_handle h, uint8_t *box, int32_t *on_target, int32_t *n_boxes, int32_t *bits_per_box)
{
    GU_ENTER(h);
    GU_NEED_GRID(h);
    const bool set = h->overlay == GU_OVERLAY_BOXES;
    if (on_target) *on_target = set ? GU_BOX_V(h->overlay_param) : 0;
    if (n_boxes) *n_boxes = set ? (int32_t)GU_BOX_B(h->overlay_param) : 0;
    if (bits_per_box) *bits_per_box = set ? (int32_t)GU_BOX_BITS(h->overlay_param) : 0;
    return box ? gu_overlay_get_plane(h, GU_OVERLAY_BOXES, box) : GU_OK;
}

int gu_get_boxes_state(gu_handle h, int64_t env0, int64_t n, uint32_t *words)
{
    GU_ENTER(h);
    return gu_overlay_get_masks(h, GU_OVERLAY_BOXES, env0, n, words, "words");
}

int gu_set_boxes_state(gu_handle h, int64_t env0, int64_t n, const uint32_t *words)
{
    GU_ENTER(h);
    // the fields of every word, before the slot's own checks (which refuse again what is refused here, with the same codes): a box
    // outside the grid would be an address outside the planes
    if (h->has_grid && h->overlay == GU_OVERLAY_BOXES && words && env0 >= 0 && n >= 0 && env0 + n <= h->N) {
        const uint32_t B = GU_BOX_B(h->overlay_param), b = GU_BOX_BITS(h->overlay_param), field = (1u << b) - 1u;
        const std::vector<uint8_t> &flags = h->box_flags;  // (kept by gu_set_boxes: no copy from the device per call)
        for (int64_t i = 0; i < n; ++i) {
            if (h->overlay_bits < 32)
                GU_REQUIRE((words[i] >> h->overlay_bits) == 0u, GU_ERR_INVALID, "words[%lld] = 0x%08x has a bit at or above the %d bits in use", (long long)i, words[i],
                           h->overlay_bits);
            for (uint32_t k = 0; k < B; ++k) {
                const uint32_t c = (words[i] >> (k * b)) & field;
                GU_REQUIRE(c < (uint32_t)h->S, GU_ERR_INVALID, "words[%lld]: box %u on cell %u, outside the %d cells", (long long)i, k, c, h->S);
                GU_REQUIRE(!(flags[c] & (GU_CELL_WALL | GU_CELL_TERM)), GU_ERR_INVALID, "words[%lld]: box %u on cell %u, which is a wall or a goal or lava cell", (long long)i, k, c);
                for (uint32_t j = 0; j < k; ++j)
                    GU_REQUIRE(((words[i] >> (j * b)) & field) != c, GU_ERR_INVALID, "words[%lld]: boxes %u and %u both on cell %u", (long long)i, j, k, c);
            }
        }
    }
    return gu_overlay_set_masks(h, GU_OVERLAY_BOXES, env0, n, words, "words");
}

}  // extern "C"
