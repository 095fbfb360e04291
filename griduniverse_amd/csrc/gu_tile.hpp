// gu_tile.hpp -- the class of a cell, one rule for the frames (gu_render.hip) and the agent's sensor (gu_sense.hip).
#pragma once
#include "gu_internal.hpp"

// Which texture a cell gets is the reference's rule (core/envs/rendering.py:119-133: goal, else lava, else wall, else ground = 3, 2,
// 1, 0; pinned by tests/golden/arrows.json "tiles").  `kind` is the engine's class plane (gu_engine::d_kind), `index` the cell's
// place in it, `f` the cell's flags byte.
__device__ __forceinline__ uint32_t gu_tile_kind(const uint8_t *kind, uint32_t f, int64_t index)
{
    if (kind) return kind[index];
    // device-generated mazes: one goal, no lava, the goal never on a wall -- the flags are unambiguous
    return (f & GU_CELL_TERM) ? ((f & GU_CELL_RMINUS) ? 2u : 3u) : (f & GU_CELL_WALL) ? 1u : 0u;
}
