// gu_boxes.hip -- pushable boxes (Sokoban) for gfx950: the first feature whose per-env state is a set of POSITIONS that the agent's own
// moves rewrite (include/gu.h: gu_set_boxes; restated on the CPU by tests/_boxes_oracle.py).  The boxes are an overlay (DESIGN.md
// "Overlays"): a third byte plane behind the engine's two cell planes (bit 0: target, bit 1: a box stands here at every reset) and one
// uint32 word per env (gu_engine::d_overlay_mask) that holds the cell of box k in bits [k * b, (k + 1) * b).  Here are the plane's and
// the words' validation and the box rule, BoxRule, around which gu_overlay.hpp's two frames are the box step kernel (gu_step,
// gu_step_device) and the box rollout kernel (gu_rollout); the slot, the launches' arguments, the words' copies and resets are
// gu_overlay.hip's and gu_overlay.hpp's; the field arithmetic and the push are gu_map.hpp's
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
// The step kernel takes one step per launch: BoxRule::load derives the count with its B reads, as at the start of a rollout.
//
// One lane per env.  The word stays in a VGPR for the whole launch: one load at the start, one store at the end.  Plain stores, no
// schedule (GuPacer).
#include "gu_overlay.hpp"

#include <algorithm>
#include <vector>

// ------------------------------------------------------------------------------------
// the rule (the interface: gu_overlay.hpp): rules 2 .. 6 of gu_set_boxes
// ------------------------------------------------------------------------------------
struct BoxRule {
    static constexpr bool DONE_IN_PLACE = true;  // (gu_overlay.hpp: its kernel handed d to the rule by reference)
    uint32_t w;
    uint32_t fs;  // the flags and the reward byte of the cell stood on, and the count of boxes on a target, carried from step to step
    int32_t rs;
    uint32_t on;

    template <class ARGS>
    __device__ __forceinline__ void load(const ARGS &a, const OverlayMap &m, uint32_t word, int32_t s)
    {
        w = word;
        fs = m.f[s];
        rs = m.r[s];
        on = gu_box_on_target(m.o, w, GU_BOX_B(a.param), GU_BOX_BITS(a.param));  // (the B reads, once per launch)
    }

    template <class ARGS>
    __device__ __forceinline__ void reset(const ARGS &a, const OverlayMap &m, uint32_t, uint32_t, int32_t s)
    {
        w = a.init;  // the boxes are back where they began
        on = GU_BOX_ON0(a.param);
        fs = m.f[s];
        rs = m.r[s];
    }

    // One step from cell s (flags fs, reward byte rs) under the word w with `on` boxes on a target: leaves s', its two bytes, w' and the
    // count in place
    template <bool LDS, class ARGS>
    __device__ __forceinline__ void move(const ARGS &a, const OverlayMap &m, uint32_t act, int32_t &s, int32_t &r, int32_t &d)
    {
        const uint32_t B = GU_BOX_B(a.param), b = GU_BOX_BITS(a.param);
        const int32_t delta = gu_delta<LDS>(act, a.lut, a.W);
        const bool solved = on == B;  // rule 2: nothing moves
        const int32_t c = gu_move(s, fs, act, delta);
        // three reads behind the one address c: flags, reward byte, box byte
        const uint32_t fc = m.f[c], bc = m.o[c];
        const int32_t rc = m.r[c];
        const int32_t at = gu_box_at(w, c, B, b);  // (computed for every lane: selects, no branch of its own)
        const int32_t k = ((c != s) & !solved) ? at : -1;
        bool stay = solved;
        int32_t gain = 0;
        if (k >= 0) stay = gu_box_push(m.f, m.o, c, fc, bc, act, delta, k, B, b, w, gain);  // the second round: pushing lanes only
        s = stay ? s : c;
        fs = stay ? fs : fc;
        rs = stay ? rs : rc;
        on += (uint32_t)gain;
        const bool done = on == B;
        d = done ? 1 : (int32_t)(fs >> GU_CELL_TERM_BIT) & 1;
        r = done ? GU_BOX_SOLVED_REWARD : rs + GU_BOX_V(a.param) * gain;
    }

    __device__ __forceinline__ uint32_t word() const { return w; }
};

void gu_boxes_step(gu_engine *h, bool lds, const OverlayStepArgs &a) { gu_overlay_step_launch<BoxRule>(h, lds, a); }
void gu_boxes_rollout(gu_engine *h, const GuRolloutPlan &p, const OverlayRolloutArgs &a) { gu_overlay_rollout_launch<BoxRule>(h, p, a); }

// ------------------------------------------------------------------------------------
// entry points
// ------------------------------------------------------------------------------------
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
    GU_TRY(gu_overlay_grid_flags(h, flags));  // (wall and terminal bits: what neither a box nor a target may lie on)
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
