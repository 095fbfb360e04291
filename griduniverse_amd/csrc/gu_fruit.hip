// gu_fruit.hip -- fruit for gfx950: collectable rewards, each eaten once per episode (include/gu.h: gu_set_fruit; restated on the
// CPU by tests/_fruit_oracle.py).  The fruit is an overlay (DESIGN.md "Overlays"): a third byte plane behind the engine's two cell
// planes (gu_engine::d_overlay_cell holds all three in one piece), three engine-wide values and one uint32 "eaten" mask per env
// (gu_engine::d_overlay_mask).  Here are the entry points and the fruit rule, FruitRule, around which gu_overlay.hpp's two frames are the
// fruit step kernel (gu_step, gu_step_device) and the fruit rollout kernel (gu_rollout); the slot, the launches' arguments, the masks,
// the plane's format (errands share it) and everything else the overlays share is gu_overlay.hip's and gu_overlay.hpp's; the fruit
// learners are instantiations of gu_td_kernel (gu_td.hip, through FruitOverlay of gu_tabular_overlay.hpp).
//
// One lane per env, like the calm kernels.  The three planes are staged in LDS where they fit 64 KiB (gu_lds_block(h, bs, 3)),
// else all three are read from L2.  Fruit never changes a move: the fruit byte of s' is read BESIDE the flags and the reward byte of
// s' (three independent reads behind one address), so the dependent chain of a step is as long as the calm kernel's.  The mask
// stays in a VGPR for the whole launch: one load at the start, one store at the end.  Plain stores, no schedule (GuPacer).
#include "gu_overlay.hpp"

#include <algorithm>

// ------------------------------------------------------------------------------------
// the rule (the interface: gu_overlay.hpp): the engine's move, and the fruit of s' beside its flags and its reward byte
// ------------------------------------------------------------------------------------
struct FruitRule {
    static constexpr bool DONE_IN_PLACE = false;  // (gu_overlay.hpp: its kernel assigned d itself)
    uint32_t eaten;

    template <class ARGS>
    __device__ __forceinline__ void load(const ARGS &, const OverlayMap &, uint32_t word, int32_t)
    {
        eaten = word;
    }

    template <class ARGS>
    __device__ __forceinline__ void reset(const ARGS &, const OverlayMap &, uint32_t, uint32_t, int32_t)
    {
        eaten = 0u;  // the fruit grows back
    }

    template <bool LDS, class ARGS>
    __device__ __forceinline__ void move(const ARGS &a, const OverlayMap &m, uint32_t act, int32_t &s, int32_t &r, int32_t &d)
    {
        s = gu_move(s, m.f[s], act, gu_delta<LDS>(act, a.lut, a.W));
        // three reads behind the one address s': flags, reward byte, fruit byte
        r = m.r[s] + gu_fruit_eat(m.o[s], a.param, eaten);
        d = (m.f[s] >> GU_CELL_TERM_BIT) & 1;
    }

    __device__ __forceinline__ uint32_t word() const { return eaten; }
};

void gu_fruit_step(gu_engine *h, bool lds, const OverlayStepArgs &a) { gu_overlay_step_launch<FruitRule>(h, lds, a); }
void gu_fruit_rollout(gu_engine *h, const GuRolloutPlan &p, const OverlayRolloutArgs &a) { gu_overlay_rollout_launch<FruitRule>(h, p, a); }

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
    if (fruit) {
        GU_REQUIRE(value != nullptr, GU_ERR_INVALID, "value is NULL");
        // Each value in -16 .. 16 keeps a launch's int32 reward sum in range at T <= 1e8.  A step ends on ONE cell, so it eats at most
        // one fruit; a fruit is eaten at most once per episode and cannot lie on a terminal cell, so the step that eats it pays the
        // cell's -1 beside it (|r| <= 17) and an episode that eats k fruits has at least k + 1 steps, the last one a terminal step
        // of |r| <= 10.  No step pays more than 17 in absolute value, and 1e8 * 17 = 1.7e9 < 2^31.  (Reward planes that put +-10 on a
        // cell that is not terminal could take a step to 26: 2^31 / 26 = 8.2e7 steps are safe for those.)
        for (int k = 0; k < 3; ++k) GU_REQUIRE(value[k] >= -16 && value[k] <= 16, GU_ERR_INVALID, "value[%d] = %d outside -16 .. 16", k, value[k]);
        GU_TRY(gu_overlay_fruit_plane(h, GU_OVERLAY_FRUIT, fruit, 32, &F));
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
