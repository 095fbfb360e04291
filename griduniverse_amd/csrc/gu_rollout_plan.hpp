// gu_rollout_plan.hpp -- which kernel a gu_rollout call runs on, and in which shape: ONE pure function (DESIGN.md "Rollout dispatch").
//
// gu_rollout_plan() makes no HIP call and allocates nothing: engine fields and gu_opt() in, everything that is decided about a launch
// out, asked in the order layout, overlay, K-step, rows, general; every threshold keeps its measurement beside it.  gu_launch_rollout
// (gu_kernels.hip) executes and records the plan; tests/test_rollout_plan.py runs it against tests/golden/rollout_plan.json, no device.
#pragma once
#include "gu_internal.hpp"

#include <algorithm>
#include <type_traits>

enum { GU_PLAN_GENERAL = 1, GU_PLAN_ROWS = 2, GU_PLAN_KSTEP = 3, GU_PLAN_WIND = 4, GU_PLAN_FRUIT = 5, GU_PLAN_DOORS = 6, GU_PLAN_BOXES = 7, GU_PLAN_ERRANDS = 8 };  // kernel families (gu_diag_rollout_form, word 1)
static_assert(GU_PLAN_FRUIT - GU_PLAN_WIND == GU_OVERLAY_FRUIT - GU_OVERLAY_WIND && GU_PLAN_DOORS - GU_PLAN_WIND == GU_OVERLAY_DOORS - GU_OVERLAY_WIND &&
                  GU_PLAN_BOXES - GU_PLAN_WIND == GU_OVERLAY_BOXES - GU_OVERLAY_WIND && GU_PLAN_ERRANDS - GU_PLAN_WIND == GU_OVERLAY_ERRANDS - GU_OVERLAY_WIND,
              "an overlay's family is GU_PLAN_WIND + its kind - GU_OVERLAY_WIND");
// `exclude`: families (1u << family) and forms that the executor found it cannot run -- a table that could not be allocated, dynamic LDS
// that does not start at address 0 -- and plans again without
#define GU_PLAN_NO_PAIRS (1u << 8)  /* the transition-row kernel's pair tables */
#define GU_PLAN_NO_MAP5 (1u << 9)   /* the general kernel's four-bit images    */

#define GU_MAX_BLOCK 1024        /* __launch_bounds__ of the general and the K-step kernel */
#define GU_ROWS_MAX_BLOCK 512    /* ... of the transition-row kernel                       */
#define GU_ROW_ADDR_MASK 0xFFFFFu /* transition rows: LDS byte address of the next row in bits 0 .. 19 (gu_rollout_rows.hip) */
#define GU_PAIR_SHIFT 7          /* log2 of a pair table's row pitch                       */
#define GU_FORM_WORDS 12

struct GuRolloutPlan {
    int family;                  // GU_PLAN_*
    int32_t policy;
    int auto_mode;               // 0 no reset, 1 auto-reset onto the one start cell, 2 onto one of several
    int traj;                    // row layout: 0 none, 1 three int32 planes, 2 packed, 3 int32 triples
    bool stats, straddle;
    // the general kernel: MAP 0 / 1 / 3 / 5 (gu_rollout.hpp; -1 on the other kernels); every wave stages its own grid; the sampling
    // thresholds sit in LDS; the engine's four-bit images (MAP 5) must exist; GU_POLICY_STREAM: action words staged per lane, and where
    int map;
    bool per_wave, pi_lds, need_nib;
    int stream_lds_off, stream_lds_words;
    // the transition-row kernel: table 0 absorbing / 1 with the auto-reset folded in; log2 of the row pitch as the kernel gets it, and of
    // the one-step table [S][4] (which a launch on the pair tables keeps built too); copies across the banks (K-step: the same three)
    int which, row_shift, table_shift, copies;
    bool table_policy, pair, half;
    int K;                       // the K-step kernel: steps per LDS round trip (0 elsewhere)
    // the launch, as finally passed
    int block;
    unsigned blocks;
    size_t lds;
    bool xcd_remap, entry_table;
    // store pacing (gu_pace_for): the kind's slot (-1: no rows that are paced), what its schedule is sized by; 0 no limiter, 1 the
    // kind's closed loop, 2 a fixed period
    int pace_slot, row_bytes, pace_block, pace_mode;
    unsigned pace_blocks;
    bool pace_eligible;
};

// ---- small helpers of the plan -------------------------------------------------------
static inline unsigned gu_blocks(int64_t n, int block) { return (unsigned)((n + block - 1) / block); }

// Largest block size <= preferred for which every block uses one grid (0 = none: use the L2 variant)
static inline int gu_lds_block(const gu_engine *h, int preferred, int planes)
{
    if (h->S > GU_MAX_LDS_CELLS || (size_t)planes * h->cell_bytes > 65536) return 0;
    if (h->n_grids == 1) return preferred;
    for (int bs = preferred; bs >= 64; bs >>= 1)
        if (h->group % bs == 0) return bs;
    return 0;
}

static inline int gu_rollout_block(const gu_engine *h) { return (int)gu_opt(h, GU_OPT_ROLLOUT_BLOCK); }

// MAP 5: dwords per env of the padded four-bits-per-cell image (eight cells per dword, rounded up to whole uint4 per lane), bytes per wave
static inline int32_t gu_nibble_cells(const gu_engine *h) { return (h->H + 2) * (h->W + 1) + 1; }
static inline int32_t gu_nibble_dwords(const gu_engine *h) { return (((gu_nibble_cells(h) + 7) / 8) + 3) & ~3; }
static inline size_t gu_nibble_bytes_per_wave(const gu_engine *h) { return (size_t)gu_nibble_dwords(h) * 256u; }

// The slot of a launch kind's pace ring (gu_engine::pace): policy x auto mode for the general kernel, the same behind 12 for the
// transition-row kernel's int32 rows and behind 24 for its packed rows.
static inline int gu_pace_slot(bool row_kernel, int traj, int32_t policy, int auto_mode)
{
    return (row_kernel ? (traj != 2 ? 12 : 24) : 0) + policy * 3 + auto_mode;
}

// Launches that cannot be bound by the HBM write path (less than 128 MB of rows, or fewer workgroups than half the CUs), launches of
// fewer than 64 steps (fewer than four groups to schedule) and batches of more than four waves per SIMD (524 288 envs and more on
// 256 CUs: a per-wave schedule found nothing to gain there, 0.96 .. 0.98 ms = 6.4 .. 6.6 TB/s with and without, and a batch that does
// not fit the device at once is not on one schedule anyway; profiles/archive/r03n_batch_sizes.txt) keep no schedule and no record --
// a fixed period applies to them all the same.
static inline bool gu_pace_eligible(const gu_engine *h, int64_t T, unsigned blocks, int row_bytes)
{
    return !((double)h->N * (double)T * (double)row_bytes < 128e6 || (int64_t)blocks * 2 < h->n_cu || T < 64 || h->N > (int64_t)h->n_cu * 1024);
}

// the pair tables fit this engine's grid: one grid, 144 bytes of LDS per cell in one workgroup's share, and GU_OPT_ROLLOUT_ROWS does
// not forbid them
static inline bool gu_rows_pairs_fit(const gu_engine *h)
{
    const int mode = (int)gu_opt(h, GU_OPT_ROLLOUT_ROWS);
    return h->n_grids == 1 && (int64_t)h->S * 144 <= h->lds_per_cu - 2048 && ((int64_t)h->S << GU_PAIR_SHIFT) <= (int64_t)GU_ROW_ADDR_MASK && mode != 0 && mode != 2;
}

// (block size, copies) for the row table, or false when it does not fit: row_bytes * copies bytes per cell and block, one table
// shared by all waves of a block; the batch must fit in (blocks per CU the LDS admits) x 256 CUs blocks.
static inline bool gu_rows_shape(const gu_engine *h, int row_bytes, int max_copies, int *block, int *copies)
{
    if (h->n_grids != 1) return false;
    // the smallest workgroup that fits, with as many copies as its LDS share admits (the copy count matters little once the
    // table is staged with wide, pipelined stores; the workgroup size does: profiles/archive/r02e_rows_copies.txt)
    // (128- and 64-thread workgroups, which spread a 32 768-env launch over all CUs instead of half of them, are no faster: 70 .. 72 us
    // either way, profiles/archive/r03h_rows_block.txt)
    for (int bs = 256; bs <= GU_ROWS_MAX_BLOCK; bs <<= 1) {
        const int64_t blocks = (h->N + bs - 1) / bs, per_cu = (blocks + h->n_cu - 1) / h->n_cu;
        for (int c = max_copies; c >= 1; c >>= 1) {
            if ((int64_t)h->S * row_bytes * c * per_cu <= h->lds_per_cu - 2048) {
                *block = bs;
                *copies = c;
                return true;
            }
        }
    }
    return false;
}

// copies of every row across the LDS banks: up to 8 (uniform / stream), 16 (greedy), 4 (sampled); GU_ROWS_COPIES overrides
// (a power of two; diagnostics)
static inline int gu_rows_max_copies(const gu_engine *h, int32_t policy)
{
    const int v = (int)gu_opt(h, GU_OPT_ROWS_COPIES);
    if (v == 1 || v == 2 || v == 4 || v == 8 || v == 16 || v == 32) return v;
    return policy == GU_POLICY_GREEDY ? 16 : policy == GU_POLICY_SAMPLE ? 4 : 8;
}

// the K-step kernel's (K, workgroup size, copies) or false: (4^K * 4 * copies + 16) bytes per cell and workgroup, as many workgroups
// per CU as the batch needs on 256 CUs
static inline bool gu_multi_shape(const gu_engine *h, int *K, int *block, int *copies)
{
    // diagnostics: force K, replicate the table (a second copy across the banks buys nothing: profiles/archive/r02h_multi_ab.txt)
    const int only = (int)gu_opt(h, GU_OPT_ROLLOUT_MULTI_K), max_copies = gu_opt(h, GU_OPT_ROLLOUT_MULTI_COPIES) == 2 ? 2 : 1;
    for (int bs = 256; bs <= GU_MAX_BLOCK; bs <<= 1) {
        const int64_t blocks = (h->N + bs - 1) / bs, per_cu = (blocks + h->n_cu - 1) / h->n_cu;
        for (int k = 4; k >= 2; k -= 2) {
            if (only && only != k) continue;
            const int64_t row = (int64_t)4 << (2 * k);
            for (int c = max_copies; c >= 1; c >>= 1) {
                if (((int64_t)h->S * (row * c + 16)) * per_cu <= h->lds_per_cu - 2048) {
                    *K = k, *block = bs, *copies = c;
                    return true;
                }
            }
        }
    }
    return false;
}

// ---- the families, in the order in which a launch is offered to them ---------------------
// the K-step kernel (gu_rollout_multi.hip): uniform policy and caller's streams, no rows, one grid, one start cell
static inline bool gu_plan_kstep(const gu_engine *h, int64_t T, bool xcd, GuRolloutPlan *p)
{
    if ((p->policy != GU_POLICY_UNIFORM && p->policy != GU_POLICY_STREAM) || p->traj != 0 || p->auto_mode == 2 || h->n_grids != 1) return false;
    const int mode = (int)gu_opt(h, GU_OPT_ROLLOUT_MULTI);
    if (mode == 0 || (mode != 1 && T < 64)) return false;  // (short launches: the second table's staging is not worth it)
    int K = 0, bs = 0, copies = 0;
    if (!gu_multi_shape(h, &K, &bs, &copies)) return false;
    p->family = GU_PLAN_KSTEP, p->K = K, p->copies = copies, p->which = p->auto_mode ? 1 : 0;
    p->row_shift = 2 * K + 2 + (copies == 2 ? 1 : 0);
    p->lds = ((size_t)h->S << p->row_shift) + (size_t)h->S * 16;
    p->block = bs, p->blocks = gu_blocks(h->N, bs), p->xcd_remap = xcd && p->blocks % 8 == 0;
    return true;
}

// the transition-row kernel (gu_rollout_rows.hip)
static inline bool gu_plan_rows(const gu_engine *h, unsigned exclude, bool xcd, GuRolloutPlan *p)
{
    const int32_t policy = p->policy;
    const int traj = p->traj, auto_mode = p->auto_mode;
    if (policy < GU_POLICY_UNIFORM || policy > GU_POLICY_SAMPLE) return false;
    if (auto_mode == 2) return false;  // several start cells: the reset draws from the RNG, it cannot be tabulated
    const int mode = (int)gu_opt(h, GU_OPT_ROLLOUT_ROWS);
    // Default policy (profiles/archive/r02b_map_ab.txt, profiles/archive/r02d_rows_crossover.txt, profiles/archive/r02e_policy_rows.txt; interleaved
    // A/B in one process): every launch that is bound by the dependent chain rather than by the HBM write path --
    //   stats only           : every batch size (uniform: 62 -> 40 us at 65 536 envs, 68 -> 35 us at 262 144)
    //   packed rows (4 B)    : up to one 256-env workgroup per CU (83 -> 51 us at 65 536 envs; 103 against 111 us at 131 072)
    //   int32 rows (12 B)    : uniform / stream / greedy up to 32 768 envs (80 -> 59 us at 4096..16 384 envs, 84 -> 74 us at
    //                          32 768 -- config 2, and a config-4 shard; beyond that the general kernel's store timing is the
    //                          better one: 124 against 133 us at 65 536 envs); sampled up to one workgroup per CU
    //   sampled policy       : only with auto-reset (122 against 141 us stats only, 148 against 168 us int32 rows at 65 536
    //                          envs); without it the general kernel's shorter step wins (107 against 122 us) -- a sampled step
    //                          is bound by its ~45 vector instructions, half of them the MurmurHash3 of its RNG word, not by
    //                          the LDS round trips the row table saves
    if (mode == 0) return false;
    if (mode != 1 && mode != 2 && mode != 3) {
        const unsigned blocks = gu_blocks(h->N, 256);
        // (a caller-supplied stream with int32 rows: the row-table kernel reads its action words straight from HBM, and a load
        // among streaming stores waits for all of them -- beyond 16 384 envs the general kernel, which stages the words in LDS,
        // is the quicker one: 88 against 116 us at 32 768 envs, profiles/archive/r02j_stream_crossover.txt)
        // (measured on the 256 CUs of an MI355X; stated relative to the CU count: one workgroup per CU, a quarter, half of them)
        const unsigned cus = (unsigned)h->n_cu;
        // (round 3, under the schedule limiter, 65 536 envs with int32 rows, profiles/archive/r03s_rows_vs_general.txt: greedy with auto-reset
        // 108 .. 111 us here against 119 .. 120 on the general kernel, whose step then has two dependent LDS reads; sampled without
        // auto-reset 135 against 142; uniform / stream / greedy without auto-reset: the same on both, they stay where they were)
        // (the whole table, 8192 .. 65 536 envs x four policy kinds x int32 / packed rows on both kernels: profiles/archive/r03s_rows_crossover.txt.
        // A caller-supplied stream with int32 rows used to leave this kernel at 16 384 envs -- its action words are read straight
        // from HBM among the streaming stores --; with sc1 + nt stores it is the quicker one up to 32 768 like the uniform policy:
        // 60 .. 61 against 66 .. 71 us)
        const unsigned int32_limit = (policy == GU_POLICY_SAMPLE || (policy == GU_POLICY_GREEDY && auto_mode == 1)) ? cus : cus / 2;
        if (((traj == 1 || traj == 3) && blocks > int32_limit) || (traj == 2 && blocks > cus)) return false;
        if (policy == GU_POLICY_SAMPLE && auto_mode != 1 && traj == 0) return false;
    }
    const bool table_policy = policy == GU_POLICY_GREEDY || policy == GU_POLICY_SAMPLE;
    const int row_log2 = policy == GU_POLICY_GREEDY ? 2 : policy == GU_POLICY_SAMPLE ? 5 : 4;
    int bs = 0, copies = 0;
    if (!gu_rows_shape(h, 1 << row_log2, gu_rows_max_copies(h, policy), &bs, &copies)) return false;
    int shift = row_log2;
    while ((1 << (shift - row_log2)) < copies) ++shift;
    // Pair tables (two steps per LDS round trip) where they pay: state-independent actions, PACKED rows (int32 rows are as fast or
    // faster on the one-step table -- 58 .. 61 against 65 us at 32 768 envs, 110 against 115 at 65 536: six stores and two records'
    // worth of unpacking per round trip cost what the shorter chain saves, and those launches are close to the write path's rate
    // anyway -- round 4, forced for int32 rows again, the chain fenced (GU_CHAIN_FENCE): 43.8 against 44.6 ns per step at config 2's
    // 4096 envs, slower at 32 768 and 65 536.  What bounds a wave that has its SIMD alone is the ISSUE of its stores, ~25 clocks per
    // 256-byte buffer_store_dword: 107 clocks per step with three of them, 143 per packed pair with two, 210 per int32 pair with six
    // (slopes over T = 2000 .. 4000); without rows the K-step kernel of gu_rollout_multi.hip is the tool), one 256-lane workgroup per CU at most (144 bytes
    // of LDS per cell).  GU_OPT_ROLLOUT_ROWS = 2 keeps the one-step table (A/B, tests).  profiles/archive/r03r_pair_rows.txt
    // (int32 TRIPLES, round 5: two 12-byte stores per pair instead of six 4-byte ones -- 37 against 50 us at config 2's 4096 envs, 39 at
    // 8192, level with the one-step table at 16 384, slower beyond; the layout hands triples to this kernel only where they pay,
    // GU_OPT_ROLLOUT_ROWS = 3 forces the pairs for every triples launch)
    const bool pair = !table_policy && (traj == 2 || (traj == 3 && (mode == 3 || policy == GU_POLICY_UNIFORM) && (mode == 3 || (int64_t)gu_blocks(h->N, 256) * 4 <= h->n_cu))) &&
                      mode != 2 && gu_blocks(h->N, 256) <= (unsigned)h->n_cu && gu_rows_pairs_fit(h) && !(exclude & GU_PLAN_NO_PAIRS);
    p->table_shift = shift;
    if (pair) bs = 256, shift = GU_PAIR_SHIFT;
    // Half waves (see the kernel).  Measured (profiles/archive/r05m_half_sizes.txt, r05m_half_ab.txt): the stores of a wave do NOT get cheaper
    // with fewer lanes -- planes at 4096 .. 8192 envs: 52.3 us either way, 55.4 against 53.3 at 16 384, and 223 against 126 us
    // where two half waves share a SIMD -- so this is no cure for the issue-bound launches.  It pays in ONE place: triples with
    // the pair tables between 8192 and 16 384 envs (43.6 against 47.6 us; the planes: 53.3), where a workgroup per four CUs
    // becomes one per two.  That is the default; GU_OPT_ROLLOUT_HALF_WAVES = 1 / 0 forces / forbids it.
    const int64_t half_opt = gu_opt(h, GU_OPT_ROLLOUT_HALF_WAVES);
    const bool half = traj != 0 && h->N % 32 == 0 &&
                      (half_opt == 1 || (half_opt == -1 && traj == 3 && pair && (int64_t)gu_blocks(h->N, 256) * 8 > h->n_cu && (int64_t)gu_blocks(h->N, 256) * 4 <= h->n_cu));
    p->family = GU_PLAN_ROWS, p->table_policy = table_policy, p->which = auto_mode ? 1 : 0, p->copies = copies, p->pair = pair, p->half = half;
    p->row_shift = shift;
    p->lds = pair ? (size_t)h->S * 144 : ((size_t)h->S << row_log2) << (shift - row_log2);
    p->block = bs, p->blocks = gu_blocks(h->N, half ? bs / 2 : bs), p->xcd_remap = xcd && p->blocks % 8 == 0;
    if (traj)  // rows to write: the store stream is rate-limited here too (gu_rollout.hpp: GuPacer)
        p->pace_slot = gu_pace_slot(true, traj, policy, auto_mode), p->row_bytes = traj != 2 ? 12 : 4, p->pace_blocks = p->blocks, p->pace_block = bs;
    return true;
}

// the general kernel (gu_rollout.hpp): which MAP, and the workgroup that goes with it
static inline void gu_plan_general(const gu_engine *h, int64_t T, unsigned exclude, bool xcd, GuRolloutPlan *p)
{
    const int32_t policy = p->policy;
    const int bs = gu_rollout_block(h);
    const bool moves_alone = policy == GU_POLICY_UNIFORM || policy == GU_POLICY_STREAM;  // (the table policies keep one grid anyway)
    auto blocks_ok = [&](int block) { return gu_blocks(h->N, block) % 8 == 0; };
    p->family = GU_PLAN_GENERAL;
    if (p->traj == 1 || p->traj == 3)  // int32 rows on the general kernel: the store stream is rate-limited (gu_rollout.hpp: GuPacer)
        p->pace_slot = gu_pace_slot(false, p->traj, policy, p->auto_mode), p->row_bytes = 12, p->pace_blocks = gu_blocks(h->N, bs), p->pace_block = bs;
    const int planes = policy == GU_POLICY_GREEDY ? 3 : 2;
    int lds_bs = gu_lds_block(h, bs, planes);
    // Groups of 64 .. 192 envs (a multiple of 64, smaller than the workgroup): every wave stages its own grid's planes, so the launch
    // keeps the workgroup size of the shared-grid launch -- whose store stream the memory takes at a shorter period than that of
    // one-wave workgroups (profiles/r06m_multigrid_ab.txt).  Uniform and stream policies (the table policies keep one grid anyway).
    if (moves_alone && lds_bs && lds_bs < bs && h->n_grids > 1 && h->group % 64 == 0 && (size_t)(bs / 64) * planes * h->cell_bytes <= 32768)
        p->per_wave = true, lds_bs = bs;
    if (lds_bs) {
        size_t lds = (size_t)planes * h->cell_bytes * (p->per_wave ? (size_t)(bs / 64) : 1);
        if (policy == GU_POLICY_SAMPLE && lds + (size_t)h->S * sizeof(uint4) <= 65536) {
            p->pi_lds = true;
            lds += (size_t)h->S * sizeof(uint4);
        }
        p->map = 1, p->block = lds_bs, p->blocks = gu_blocks(h->N, lds_bs), p->xcd_remap = xcd && blocks_ok(lds_bs);
        if (policy == GU_POLICY_STREAM && p->traj != 0) {
            // staged action words: as many per lane as the LDS share of a block admits at the occupancy this batch needs
            const int64_t per_cu = std::min<int64_t>(8, std::max<int64_t>(1, ((int64_t)p->blocks + h->n_cu - 1) / h->n_cu));
            const int64_t room = h->lds_per_cu / per_cu - (int64_t)lds - 512;
            const int64_t kw = std::min<int64_t>({room / ((int64_t)lds_bs * 4), (int64_t)64, (T + 15) / 16});
            if (kw >= 4) {
                p->stream_lds_off = (int)lds;
                p->stream_lds_words = (int)kw;
                lds += (size_t)kw * lds_bs * 4;
            }
        }
        p->lds = lds;
        return;
    }
    p->block = bs, p->blocks = gu_blocks(h->N, bs);
    // one grid too big for two planes in 64 KiB: its flags plane alone, up to the whole 160 KB of a CU
    if (moves_alone && h->n_grids == 1 && h->W <= 32767 && (int64_t)h->cell_bytes <= h->lds_per_cu - 512) {
        p->map = 3, p->lds = (size_t)h->cell_bytes, p->xcd_remap = xcd && blocks_ok(bs);
        return;
    }
    // misaligned multi-grid engine (e.g. one maze per env): every lane's grid at four bits per cell in LDS, if a wave's 64 fit
    if (p->need_nib && !(exclude & GU_PLAN_NO_MAP5)) {
        // workgroups of four waves where four images fit a CU's LDS (32 x 32: 144 KB): the launch shape of the shared-grid kernel,
        // whose store stream the memory takes at a shorter period than that of 1024 one-wave workgroups (profiles/r06m_multigrid_ab.txt)
        int mbs = 256;
        while (mbs > 64 && (size_t)(mbs / 64) * gu_nibble_bytes_per_wave(h) > (size_t)h->lds_per_cu - 512) mbs >>= 1;
        p->map = 5, p->lds = (size_t)(mbs / 64) * gu_nibble_bytes_per_wave(h), p->block = mbs, p->blocks = gu_blocks(h->N, mbs), p->xcd_remap = xcd;
        return;
    }
    p->map = 0, p->lds = 0, p->xcd_remap = xcd && h->n_grids == 1 && blocks_ok(bs);
}

inline GuRolloutPlan gu_rollout_plan(const gu_engine *h, int64_t T, int32_t policy, uint32_t flags, bool straddle, unsigned exclude)
{
    GuRolloutPlan p{};
    p.policy = policy, p.stats = (flags & GU_F_STATS) != 0, p.straddle = straddle, p.map = -1, p.pace_slot = -1;
    p.auto_mode = (flags & GU_F_AUTO_RESET) ? (h->all_single_start ? 1 : 2) : 0;
    // ---- layout.  int32 rows: three planes [T][N], or one plane of (obs, reward, done) triples [T][N][3] -- the same words, one 12-byte store
    // per lane and step (gu_rollout.hpp: TRAJ == 3; the readers take them apart again: gu_read_trajectory, gu_mc_evaluate).
    // GU_OPT_TRAJ_LAYOUT: 0 = planes, 1 = triples wherever possible, -1 (default) = triples where they are faster.  Measured
    // (profiles/archive/r05b_layout_ab.txt, r05c_layout_sizes.txt, five variants interleaved in one process): a launch bound by the HBM write path is
    // SLOWER with triples -- 65 536 envs: 117 against 112 us, a config-4 shard of 32 768: 68 against 63 -- and so is every table
    // policy; a launch of a few waves, bound by the ISSUE of its stores (~25 clocks per 256-byte store of a wave that has its SIMD
    // alone), gains little from the triple alone (config 2, 4096 envs: 49.4 against 49.9 us) but 25 % together with the pair tables
    // (two steps per LDS round trip, two stores per pair instead of six: 37.3 us), up to 8192 envs = one workgroup per eight
    // CUs; at 16 384 the two are level -- unless the batch is spread over twice the waves (32 envs each: 43.6 against 53.3 us,
    // profiles/archive/r05m_half_sizes.txt) --, beyond it the planes win.  So: triples for the uniform policy where the pair tables fit,
    // up to n_cu / 4 workgroups of 256 (half waves for the upper half of that range).  Batches of more than 2^24 envs (lane offset + 15 rows must stay
    // below 2^32 bytes) and engines with the agent trail on or an overlay set always keep the planes.
    // (AS IT STANDS the default does not ask the auto mode: with several start cells the triples go to the general kernel.  DESIGN.md 4.0)
    p.traj = (flags & GU_F_PACKED) ? 2 : ((flags & GU_F_TRAJECTORY) ? 1 : 0);
    if (p.traj == 1 && h->N <= ((int64_t)1 << 24) && !h->trail_cap && !h->overlay) {
        const int64_t layout = gu_opt(h, GU_OPT_TRAJ_LAYOUT);
        if (layout == 1 || (layout == -1 && policy == GU_POLICY_UNIFORM && gu_rows_pairs_fit(h) && (int64_t)gu_blocks(h->N, 256) * 4 <= h->n_cu)) p.traj = 3;
    }
    p.entry_table = h->entry_table_ok && gu_opt(h, GU_OPT_ROLLOUT_ENTRY) != 0;
    // groups that do not align with blocks (one maze per env): the general kernel's MAP 5 wants every env's grid at four bits per cell
    // (cells of the padded image times 32: W <= 1022 keeps a row's step inside an int16)
    p.need_nib = h->n_grids > 1 && (policy == GU_POLICY_UNIFORM || policy == GU_POLICY_STREAM) && !gu_lds_block(h, gu_rollout_block(h), 2) && h->W <= 1022 &&
                 gu_nibble_bytes_per_wave(h) <= (size_t)h->lds_per_cu - 512;
    const bool xcd = gu_opt(h, GU_OPT_ROLLOUT_XCD) != 0 && h->n_grids == 1;  // XCD-aware env-block order (see gu_env_block; measured slower, off)
    // ---- overlay, K-step, rows, general.  A launch during which an env passes a multiple of 2^32 steps goes to the general kernel,
    // which asks the RNG's epoch per lane and step.
    if (h->overlay) {  // an overlay's kernel (gu_wind.hip, gu_fruit.hip, gu_doors.hip, gu_boxes.hip, gu_errands.hip) serves every shape: three planes in LDS where they fit, int32 planes only
        p.family = GU_PLAN_WIND + h->overlay - GU_OVERLAY_WIND, p.block = GU_BLOCK, p.blocks = gu_blocks(h->N, GU_BLOCK);
        p.lds = gu_lds_block(h, GU_BLOCK, 3) ? 3 * (size_t)h->cell_bytes : 0;
        p.straddle = p.entry_table = false;  // (its kernel reads neither: it counts steps in 64 bits and asks the RNG's epoch per step)
    } else if (!straddle && !(exclude & (1u << GU_PLAN_KSTEP)) && gu_plan_kstep(h, T, xcd, &p)) {}
    else if (!straddle && !(exclude & (1u << GU_PLAN_ROWS)) && gu_plan_rows(h, exclude, xcd, &p)) {}
    else gu_plan_general(h, T, exclude, xcd, &p);
    if (p.pace_slot >= 0) {
        const int64_t opt = gu_opt(h, GU_OPT_ROLLOUT_PACE);
        p.pace_eligible = gu_pace_eligible(h, T, p.pace_blocks, p.row_bytes);
        p.pace_mode = opt == 0 ? 0 : opt > 0 ? 2 : p.pace_eligible ? 1 : 0;
    }
    return p;
}

// the plan as gu_diag_rollout_form reports it (include/gu.h)
inline void gu_rollout_plan_form(const GuRolloutPlan &p, int32_t form[GU_FORM_WORDS])
{
    const int32_t words[GU_FORM_WORDS] = {p.family, p.traj, p.map, p.block, (int32_t)p.blocks, (int32_t)p.lds,
                                          (p.pair ? 1 : 0) | (p.half ? 2 : 0) | (p.per_wave ? 4 : 0) | (p.pi_lds ? 8 : 0) | (p.straddle ? 16 : 0) | (p.entry_table ? 32 : 0) | (p.xcd_remap ? 64 : 0),
                                          p.K, p.row_shift, p.stream_lds_words, p.pace_slot, p.pace_mode};
    std::copy(words, words + GU_FORM_WORDS, form);
}

// run-time value -> template argument: f(std::integral_constant<int, V>{}) for the V among Vs that equals v (false: none does)
template <int... Vs, class F>
static inline bool gu_pick(int v, F &&f)
{
    return ((v == Vs ? (f(std::integral_constant<int, Vs>{}), true) : false) || ...);
}
