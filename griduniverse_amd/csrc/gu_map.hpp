// gu_map.hpp -- device helpers shared by the step / rollout / look-ahead kernels: the per-cell record map (global,
// block-shared LDS or private LDS), the action -> delta LUT, the branch-free move and the wind's pushes.
#pragma once
#include "gu_internal.hpp"
#include "gu_rng.hpp"

// ------------------------------------------------------------------------------------
// helpers
// ------------------------------------------------------------------------------------
struct CellMap {
    const uint8_t *f;  // flags plane
    const int8_t *r;   // reward plane
};

// LDS variants: the whole block uses ONE grid (single-grid engines, or multi-grid engines whose group size is a
// multiple of the block size -- the launcher guarantees it), whose planes are staged into LDS.
__device__ __forceinline__ uint32_t gu_block_grid(const GridSel &gs)
{
    if (gs.n_grids <= 1) return 0u;
    const int64_t first = (int64_t)blockIdx.x * blockDim.x + (gs.per_wave ? (int64_t)(threadIdx.x & ~63u) : 0);  // the workgroup's / the wave's first env
    const int64_t grid = first / gs.group;
    return (uint32_t)(grid < gs.n_grids ? grid : gs.n_grids - 1);  // (a wave past the batch stages the last grid: its lanes leave right after)
}

template <bool LDS>
__device__ __forceinline__ CellMap gu_stage_map(const uint8_t *__restrict__ g, int32_t cell_bytes, uint8_t *smem, const GridSel &gs,
                                                int planes = 2)
{
    if (LDS) {
        g += (int64_t)gu_block_grid(gs) * gs.grid_stride;
        if (gs.per_wave) {  // every wave its own grid, in its own region of the workgroup's LDS
            smem += (threadIdx.x >> 6) * (uint32_t)(planes * cell_bytes);
            for (int32_t i = (threadIdx.x & 63) * 16; i < planes * cell_bytes; i += 64 * 16)
                *reinterpret_cast<uint4 *>(smem + i) = *reinterpret_cast<const uint4 *>(g + i);
        } else {
            for (int32_t i = threadIdx.x * 16; i < planes * cell_bytes; i += blockDim.x * 16)
                *reinterpret_cast<uint4 *>(smem + i) = *reinterpret_cast<const uint4 *>(g + i);
        }
        __syncthreads();
        return CellMap{smem, reinterpret_cast<const int8_t *>(smem + cell_bytes)};
    }
    return CellMap{g, reinterpret_cast<const int8_t *>(g + cell_bytes)};
}

// Which grid does lane e use?  In the LDS variants it is the block's grid (start table selected with scalar
// arithmetic); the L2 variants serve any group size: env e uses grid e / group, its planes sit g * grid_stride
// bytes into the plane buffer.
struct LaneGrid {
    const int32_t *starts;
    uint32_t n_starts;
};

template <bool LDS>
__device__ __forceinline__ LaneGrid gu_lane_grid(const GridSel &gs, const int32_t *starts, uint32_t n_starts0, uint32_t e, CellMap &m)
{
    if (gs.n_grids <= 1) return LaneGrid{starts, n_starts0};
    if (LDS) {
        const uint32_t gb = gu_block_grid(gs);
        return LaneGrid{starts + (int64_t)gb * gs.max_starts, (uint32_t)gs.n_starts[gb]};
    }
    const uint32_t g = e / (uint32_t)gs.group;
    m.f += (int64_t)g * gs.grid_stride;
    m.r += (int64_t)g * gs.grid_stride;
    return LaneGrid{starts + (int64_t)g * gs.max_starts, (uint32_t)gs.n_starts[g]};
}

// delta[a]: LUT = four int16 lanes {-W, +1, +W, -1}; ARITH = any W (grids too big for the LUT / LDS)
// SHIFT64: the lookup as ONE 64-bit shift by 16 a (v_lshrrev_b64) -- or, false, a select between the LUT's halves and a 16-bit field
// of the one selected (32-bit instructions only, one more of them).  The 64-bit shift has a FAULT on gfx950: when the register that
// holds its shift amount is the LAST of the wave's VGPR allocation (v63 of 64, v31 of 32) and other waves share the SIMD, it now and
// then shifts by the low six bits of what lies behind the allocation -- the lane index, v0 of the neighbour's registers -- instead:
// the move's delta is then lut >> lane, the env leaves the grid (docs/HISTORY.md "64-bit shift by the last VGPR";
// tests/test_gpu_launch_shapes.py saw it, tests/test_shift_amount_register.py keeps every kernel of the built library clear of it).
// Where the register allocator puts the amount is not ours to say, so only the kernels measured with the one shift keep it.
template <bool LUT, bool SHIFT64 = true>
__device__ __forceinline__ int32_t gu_delta(uint32_t a, uint64_t lut, int32_t W)
{
    if (LUT && SHIFT64) return __builtin_amdgcn_sbfe((int32_t)(uint32_t)(lut >> (a << 4)), 0, 16);
    if (LUT) return __builtin_amdgcn_sbfe((int32_t)(a > 1u ? (uint32_t)(lut >> 32) : (uint32_t)lut), (a & 1u) << 4, 16);
    const int32_t sign = (int32_t)(a & 2u) - 1;  // UP,RIGHT -> -1 ; DOWN,LEFT -> +1
    return (a & 1u) ? -sign : sign * W;
}

// reward code in bits 5 (RPLUS) and 6 (RMINUS) of the record -> -1, +10, -10, -10 (lava over goal, env:86-88): one byte of a constant
__device__ __forceinline__ int32_t gu_reward_packed(uint32_t flags)
{
    return __builtin_amdgcn_sbfe((int32_t)0xF6F60AFFu, (flags >> 2) & 24u, 8);
}

__device__ __forceinline__ int32_t gu_move(int32_t s, uint32_t flags, uint32_t a, int32_t delta)
{
    return __mul24((int32_t)__builtin_amdgcn_ubfe(flags, a, 1), delta) + s;  // v_bfe_u32 + v_mad_i32_i24
}

// ------------------------------------------------------------------------------------
// wind (include/gu.h: gu_set_wind): one byte per cell behind the two cell planes, bits 0..1 the direction, bits 2..3 the strength
// ------------------------------------------------------------------------------------
#define GU_WIND_STRENGTH(c) (((c) >> 2) & 3u)

// the strength after the gust test on the stream-9 word w of the step: k > 0 becomes k + 1 or k - 1 where (w >> 16) < gust_q16
__device__ __forceinline__ uint32_t gu_wind_gust(uint32_t k, uint32_t w, uint32_t gust_q16)
{
    const uint32_t moved = (w & 1u) ? k + 1u : k - 1u;
    return (k > 0u && (w >> 16) < gust_q16) ? moved : k;
}

// k pushes of the cell's wind from s (where the action left the agent), each one move of the engine's rule: the OPEN bit of the
// cell stood on.  A WAVE-UNIFORM loop with an early exit: it runs while some lane of the wave still has pushes left, so a wave
// over calm cells pays one ballot and one untaken scalar branch, and a lane that a wall, the border or a terminal cell has stopped
// leaves the count at once (the same push from the same cell would fail again).  Every trip is one dependent read of the flags plane.
template <bool LUT>
__device__ __forceinline__ int32_t gu_wind_push(const uint8_t *f, int32_t s, uint32_t c, uint32_t k, uint64_t lut, int32_t W)
{
    const uint32_t dir = c & 3u;
    const int32_t delta = gu_delta<LUT>(dir, lut, W);
    while (__builtin_amdgcn_ballot_w64(k > 0u) != 0ull) {
        const uint32_t go = k > 0u ? __builtin_amdgcn_ubfe((uint32_t)f[s], dir, 1) : 0u;
        s += __mul24((int32_t)go, delta);
        k = go ? k - 1u : 0u;
    }
    return s;
}

// ------------------------------------------------------------------------------------
// fruit (include/gu.h: gu_set_fruit): one byte per cell behind the two cell planes, bits 0..4 the slot, bits 5..6 the kind (0: none)
// ------------------------------------------------------------------------------------
// What the fruit byte c of the cell just reached adds to the step's reward, and its slot into the env's mask.  `values` holds the
// three kinds' values as int8 bytes 1 .. 3 (byte 0, "no fruit", is zero), so the pick is one v_bfe_i32 on kind * 8 and nothing
// branches: a shift (an UNSIGNED 1: slot 31 is in range), an and-not for "not eaten yet" and an or.
__device__ __forceinline__ int32_t gu_fruit_eat(uint32_t c, uint32_t values, uint32_t &eaten)
{
    const uint32_t kind = (c >> 5) & 3u;
    const uint32_t bit = (kind ? 1u : 0u) << (c & 31u);
    const int32_t v = __builtin_amdgcn_sbfe((int32_t)values, kind << 3, 8);
    const int32_t gain = (bit & ~eaten) ? v : 0;
    eaten |= bit;
    return gain;
}

// ------------------------------------------------------------------------------------
// doors (include/gu.h: gu_set_doors): one byte per cell behind the two cell planes, bits 0..2 the slot, bits 4..5 the kind (0: nothing,
// 1: door, 2: key, 3: lever)
// ------------------------------------------------------------------------------------
// Does the door byte c of the candidate cell refuse entry under the mask `open`?  (kind 1 and the slot's bit clear)
__device__ __forceinline__ bool gu_door_closed(uint32_t c, uint32_t open)
{
    return ((c >> 4) & 3u) == 1u && !((open >> (c & 7u)) & 1u);
}

// The mask behind a step that ENTERED the cell of door byte c (`entered`: s' != s): a key sets its slot's bit, a lever flips it;
// standing still touches nothing.  Nothing branches: the bit is zero for the other kinds, and a key's or-in is a flip of a clear bit.
__device__ __forceinline__ uint32_t gu_door_touch(uint32_t c, uint32_t open, bool entered)
{
    const uint32_t kind = (c >> 4) & 3u;
    const uint32_t bit = ((entered && kind >= 2u) ? 1u : 0u) << (c & 7u);
    return kind == 3u ? open ^ bit : open | bit;
}

// ------------------------------------------------------------------------------------
// boxes (include/gu.h: gu_set_boxes): one byte per cell behind the two cell planes, bit 0 = target, bit 1 = a box stands here at every
// reset; the env's word holds the cell of box k in bits [k * b, (k + 1) * b), b the smallest width with S <= 1 << b (at most 16, and
// b * B <= 32: the last field's shift is (B - 1) * b < 32, so nothing ever shifts by 32)
// ------------------------------------------------------------------------------------
// The kernels' parameter word (gu_engine::overlay_param): on_target, B, b and the number of boxes that stand on a target at a reset.
#define GU_BOX_PARAM(v, B, b, on0) ((uint32_t)(v) | ((uint32_t)(B) << 8) | ((uint32_t)(b) << 16) | ((uint32_t)(on0) << 24))
#define GU_BOX_V(p) ((int32_t)((p) & 31u))
#define GU_BOX_B(p) (((p) >> 8) & 15u)  /* at most 8: b = 4, sixteen cells */
#define GU_BOX_BITS(p) (((p) >> 16) & 31u)
#define GU_BOX_ON0(p) (((p) >> 24) & 15u)
#define GU_BOX_TARGET 1u
#define GU_BOX_INITIAL 2u
#define GU_BOX_SOLVED_REWARD 10

// the box that stands on cell c under the word w, or -1: B field extractions and compares (B and b are launch-uniform)
__device__ __forceinline__ int32_t gu_box_at(uint32_t w, int32_t c, uint32_t B, uint32_t b)
{
    const uint32_t field = (1u << b) - 1u;
    int32_t k = -1;
    for (uint32_t i = 0; i < B; ++i) k = ((w >> (i * b)) & field) == (uint32_t)c ? (int32_t)i : k;
    return k;
}

// how many boxes of w stand on a target: B reads of the box plane (once per launch; the rollout and the learners carry the count)
__device__ __forceinline__ uint32_t gu_box_on_target(const uint8_t *bx, uint32_t w, uint32_t B, uint32_t b)
{
    const uint32_t field = (1u << b) - 1u;
    uint32_t on = 0;
    for (uint32_t i = 0; i < B; ++i) on += bx[(w >> (i * b)) & field] & GU_BOX_TARGET;
    return on;
}

// The push of box k, which stands on the candidate cell c (flags fc, box byte bc), by action `act`: the SECOND round of reads of a
// step, behind c -- the flags and the box byte of c2, the engine's move from c.  Returns true where the push is refused (c2 == c: the
// border or a wall; a goal or lava cell; another box) and leaves w alone; else moves the box in w and sets `gain` to target[c2] -
// target[c].  Only lanes that push call it, so a wave in which nobody pushes skips the round (the caller's branch).
__device__ __forceinline__ bool gu_box_push(const uint8_t *f, const uint8_t *bx, int32_t c, uint32_t fc, uint32_t bc, uint32_t act, int32_t delta, int32_t k,
                                            uint32_t B, uint32_t b, uint32_t &w, int32_t &gain)
{
    const int32_t c2 = gu_move(c, fc, act, delta);
    const uint32_t f2 = f[c2], b2 = bx[c2];
    const bool other = gu_box_at(w, c2, B, b) >= 0;  // (no short circuit: the two reads and the compares are ONE round, not three)
    const bool refused = (c2 == c) | ((f2 & GU_CELL_TERM) != 0u) | other;
    const uint32_t field = (1u << b) - 1u, at = (uint32_t)k * b;
    w = refused ? w : ((w & ~(field << at)) | ((uint32_t)c2 << at));
    gain = refused ? 0 : (int32_t)(b2 & GU_BOX_TARGET) - (int32_t)(bc & GU_BOX_TARGET);
    return refused;
}

// ------------------------------------------------------------------------------------
// errands (include/gu.h: gu_set_errands): the plane is fruit's (bits 0..4 the slot, bits 5..6 the kind); the env's word holds the
// fruit eaten in bits [0, F), the progress p in bits [F, F + pb) and the instruction index j in bits [F + pb, F + pb + ib)
// ------------------------------------------------------------------------------------
// The two parameter words (gu_engine::overlay_param, overlay_param2), both wave-uniform.  The first holds the instructions, byte j
// instruction j, position p in bits 2p .. 2p + 1, kind 0 the end mark (a list of four has none).  The second holds the pay as int8
// bytes 0 .. 2 (right, wrong, finish) and F - 1, pb and I - 1 above them.
#define GU_ERRAND_PARAM2(right, wrong, finish, F, pb, I)                                                                                   \
    ((uint32_t)(uint8_t)(int8_t)(right) | ((uint32_t)(uint8_t)(int8_t)(wrong) << 8) | ((uint32_t)(uint8_t)(int8_t)(finish) << 16) |    \
     ((uint32_t)((F) - 1) << 24) | ((uint32_t)(pb) << 27) | ((uint32_t)((I) - 1) << 29))
#define GU_ERRAND_F(q) ((((q) >> 24) & 7u) + 1u)
#define GU_ERRAND_PB(q) (((q) >> 27) & 3u)
#define GU_ERRAND_I(q) ((((q) >> 29) & 3u) + 1u)

// `rem` is what a lane carries beside its word: the env's instruction byte shifted right by 2p.  The wanted kind is rem & 3 and the
// instruction is complete where rem == 0 (a list of four included: the byte is shifted out), so nothing in a step indexes the table.
__device__ __forceinline__ uint32_t gu_errand_rem(uint32_t word, uint32_t instr, uint32_t q)
{
    const uint32_t F = GU_ERRAND_F(q), pb = GU_ERRAND_PB(q);
    const uint32_t p = (word >> F) & ((1u << pb) - 1u), j = (word >> (F + pb)) & 3u;
    return ((instr >> (8u * j)) & 0xFFu) >> (2u * p);
}

// Rule 1: the word and `rem` of an env that is being reset at episode count ep (the count BEFORE the reset increments it).
// start_prefix is stream 1's (seed and env, no epoch).  One instruction: no word is hashed (the test is wave-uniform).
__device__ __forceinline__ void gu_errand_draw(uint32_t start_prefix, uint32_t ep, uint32_t instr, uint32_t q, uint32_t &word, uint32_t &rem)
{
    const uint32_t I = GU_ERRAND_I(q);
    uint32_t j = 0u;
    if (I > 1u) j = (uint32_t)(((uint64_t)gu_rng_word(start_prefix, GU_RNG_STREAM_ERRAND, ep) * (uint64_t)I) >> 32);
    word = j << (GU_ERRAND_F(q) + GU_ERRAND_PB(q));
    rem = (instr >> (8u * j)) & 0xFFu;
}

// Rules 2, 4 and 5 on the bytes of the candidate cell (c the errand byte, rb the reward byte, term the terminal bit), all three read
// beside each other: sets r and d and moves the word on.  Returns true where the word was complete already (rule 2): the caller
// then keeps s.  Nothing branches.
__device__ __forceinline__ bool gu_errand_touch(uint32_t c, int32_t rb, int32_t term, uint32_t q, uint32_t &word, uint32_t &rem, int32_t &r, int32_t &d)
{
    const bool complete = rem == 0u;
    const uint32_t kind = (c >> 5) & 3u;
    const uint32_t bit = (kind ? 1u : 0u) << (c & 31u);
    const bool fresh = !complete && (bit & ~word) != 0u;
    const bool right = fresh && kind == (rem & 3u);
    word |= fresh ? bit : 0u;
    word += right ? (1u << GU_ERRAND_F(q)) : 0u;
    rem = right ? rem >> 2 : rem;
    const bool fin = complete || (right && rem == 0u);
    const int32_t pay = __builtin_amdgcn_sbfe((int32_t)q, right ? 0u : 8u, 8);
    r = fin ? __builtin_amdgcn_sbfe((int32_t)q, 16u, 8) : rb + (fresh ? pay : 0);
    d = fin ? 1 : term;
    return complete;
}
