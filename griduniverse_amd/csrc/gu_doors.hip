// gu_doors.hip -- doors, keys and levers for gfx950: the first feature whose move rule depends on the lane's own bits of state
// (include/gu.h: gu_set_doors; restated on the CPU by tests/_doors_oracle.py).  The doors are an overlay (DESIGN.md "Overlays"): a
// third byte plane behind the engine's two cell planes (gu_engine::d_overlay_cell holds all three in one piece) and one uint32 mask of
// open slots per env (gu_engine::d_overlay_mask).  Here are the plane's validation and the door rule, DoorRule, around which
// gu_overlay.hpp's two frames are the door step kernel (gu_step, gu_step_device) and the door rollout kernel (gu_rollout); the slot, the
// launches' arguments, the masks and everything else the overlays share is gu_overlay.hip's and gu_overlay.hpp's; the door learners
// are instantiations of gu_td_kernel (gu_td.hip, through DoorOverlay of gu_tabular_overlay.hpp).
//
// THE GATE, decided on purpose.  The rule reads door[c] after flags[s] has produced the candidate c: taken literally that is a second
// dependent LDS read in front of the reads at s', in a loop whose speed is its dependent chain.  A derived 16-bit plane that names,
// at s, the slot guarding each direction would take the gate off the chain at five bytes per cell instead of three (grids between
// 64 KiB / 5 and 64 KiB / 3 cells would fall to L2).  The rule here does neither.  It CARRIES the flags and the reward
// byte of the cell it stands on in VGPRs and reads all three bytes of the CANDIDATE -- flags[c], reward[c], door[c], three
// independent reads behind one address, as fruit reads s'.  Open or no door: the candidate's bytes become the carried ones.  Closed:
// the carried ones stay (they are the bytes of s' = s, which is what a bump pays).  So a step has ONE round of LDS reads on its
// chain, the calm kernel's count, the plane stays the byte the interface takes, and the LDS limit stays fruit's (three planes).  The
// cost is two VGPRs and three selects per step, and one more round of reads behind a lazy reset (the start cell's bytes).  The
// derived-plane form was not built, so there is no measured difference between the two to quote; what was measured is this kernel
// beside the fruit kernel, which has no gate at all (tools/doors_rate.py, profiles/doors_rate.json: 0.98 .. 1.08 of its rate).  The
// learners' lane (DoorOverlay::move, gu_tabular_overlay.hpp) gates the same way, with the bytes of s read beside each other instead of carried.
// The step kernel runs the same DoorRule::move for its one step: it reads the two bytes of s beside each other where the rollout
// carries them -- one independent read more than the rule as it is written needs, in a launch that is bound by the launch itself.
//
// One lane per env.  The mask stays in a VGPR for the whole launch: one load at the start, one store at the end.  Plain stores, no
// schedule (GuPacer).
#include "gu_overlay.hpp"

#include <algorithm>
#include <vector>

// ------------------------------------------------------------------------------------
// the rule (the interface: gu_overlay.hpp): the gate of the candidate cell between its bytes and the carried ones
// ------------------------------------------------------------------------------------
struct DoorRule {
    static constexpr bool DONE_IN_PLACE = false;  // (gu_overlay.hpp: its kernel assigned d itself)
    uint32_t open;
    uint32_t fs;  // the flags and the reward byte of the cell stood on, carried from step to step (the head of this file)
    int32_t rs;

    template <class ARGS>
    __device__ __forceinline__ void load(const ARGS &, const OverlayMap &m, uint32_t word, int32_t s)
    {
        open = word;
        fs = m.f[s];
        rs = m.r[s];
    }

    template <class ARGS>
    __device__ __forceinline__ void reset(const ARGS &, const OverlayMap &m, uint32_t, uint32_t, int32_t s)
    {
        open = 0u;  // the doors are shut again, the keys are back (a reset onto a key or lever cell touches nothing)
        fs = m.f[s];
        rs = m.r[s];
    }

    template <bool LDS, class ARGS>
    __device__ __forceinline__ void move(const ARGS &a, const OverlayMap &m, uint32_t act, int32_t &s, int32_t &r, int32_t &d)
    {
        const int32_t c = gu_move(s, fs, act, gu_delta<LDS>(act, a.lut, a.W));
        // three reads behind the one address c: flags, reward byte, door byte -- and the gate picks between them and the carried ones
        const uint32_t fc = m.f[c], dc = m.o[c];
        const int32_t rc = m.r[c];
        const bool shut = gu_door_closed(dc, open);
        open = gu_door_touch(dc, open, !shut && c != s);
        s = shut ? s : c;
        fs = shut ? fs : fc;
        rs = shut ? rs : rc;
        r = rs;
        d = (int32_t)(fs >> GU_CELL_TERM_BIT) & 1;
    }

    __device__ __forceinline__ uint32_t word() const { return open; }
};

void gu_doors_step(gu_engine *h, bool lds, const OverlayStepArgs &a) { gu_overlay_step_launch<DoorRule>(h, lds, a); }
void gu_doors_rollout(gu_engine *h, const GuRolloutPlan &p, const OverlayRolloutArgs &a) { gu_overlay_rollout_launch<DoorRule>(h, p, a); }

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
        std::vector<uint8_t> flags;
        GU_TRY(gu_overlay_grid_flags(h, flags));
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
