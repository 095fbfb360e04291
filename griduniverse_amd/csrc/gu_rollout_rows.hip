// gu_rollout_rows.hip -- the fused rollout on a TRANSITION-ROW table: the latency-bound form of the caller loop of
// core/algorithms/monte_carlo.py:7-26 for one small grid with a single start cell (or no auto-reset).
//
// The general kernel (gu_rollout.hpp) walks the per-cell records: per step  record -> TERM test + two selects (lazy reset)
// -> OPEN bit -> multiply-add -> LDS gather, i.e. ~6 dependent vector ops around one LDS round trip.  Here the whole
// transition of core/envs/griduniverse_env.py:136-155 INCLUDING the harness's `if done: env.reset()` is tabulated per
// (cell, action) once per grid by gu_build_rows_kernel:
//
//     row[s][a] = { LDS byte address of row[next] : bits 0..19 | done(next) : bit 23 | reward_matrix[next] int8 : bits 24..31 }
//     next      = look_step_ahead(base, a).next,   base = start cell if (auto-reset and s is terminal) else s
//
// so that one env-step is   addr = (rec & 0xFFFFF) | (copy * 16 + action * 4);   rec = LDS[addr]   -- ONE v_and_or_b32 and one
// ds_read_b32 on the dependent chain; cell index, reward, done flag, episode count and the trajectory stores all hang off
// `rec` beside the chain.  The 16-byte rows are replicated `copies` (<= 8) times so that the lanes of a half-wave spread
// over the LDS banks (bank = copy * 4 + action).  The invariant the table relies on -- "the env is done exactly when its
// cell is terminal" -- holds after any step but not for an arbitrary stored state (gu_set_state, a reset onto a terminal
// start), so a launch takes its FIRST step on the per-cell planes, like the general kernel -- unless it follows a rollout of
// the same engine (RolloutArgs::entry_table, round 5: the state a rollout leaves behind always agrees with its cell).
//
// Table policies use the same idea with policy-dependent rows, rebuilt by every launch (the policy table may have changed):
//   GU_POLICY_GREEDY  row[s]    = the one record reached by the greedy action of the (post-reset) cell: 4 bytes, up to 32
//                                 copies; a step is v_and_or_b32 + ds_read_b32
//   GU_POLICY_SAMPLE  row[s]    = { inverse-CDF thresholds of pi[cell], SORTED (uint4, from gu_pi_threshold_kernel) | the four next
//                                 records }: 32 bytes, up to 4 copies; a step is ONE round trip for two ds_read_b128, the three
//                                 threshold compares and a three-select pick of the next record (the general kernel: a
//                                 threshold gather, the compares, the move, and a second gather for the record)
//
// Store waves -- a second half of the workgroup that drains an LDS ring of records and issues the rows' stores, so that the stepping
// waves' in-order instruction stream carries neither the stores nor their stalls -- were built in round 4 and measured SLOWER for
// every launch whose chain is short (uniform / greedy at 4096 .. 32 768 envs: 75 against 50 .. 60 us per 1000 steps: the hand-over
// itself, a produced / consumed count pair per wave and eight records per group, costs ~180 clocks per step) and no faster where the
// chain is long (sampled policy at 65 536 envs: 130 against 128; 110 against 117 at 32 768): profiles/archive/r04s_rows_store_waves_ab.json.
// Removed again; the sampled launch with int32 rows stays bound by its one wave per SIMD issuing chain and stores in order.
//
// Results are bit-identical to the general kernel (tests/test_gpu_rows_kernel.py runs both on the same seeds); the launcher
// picks this one where it is faster (profiles/archive/r02b_map_ab.txt, profiles/archive/r02d_rows_crossover.txt).
#include "gu_rollout.hpp"

#define GU_ROW_DONE_BIT 23

struct BuildRowsArgs {
    const uint8_t *cell;  // absorbing-aware planes [flags | reward]
    int32_t cell_bytes, S, W, start0, auto_reset, row_shift;
    uint32_t *rows;       // [S][4]
};

__global__ void __launch_bounds__(256) gu_build_rows_kernel(const BuildRowsArgs a)
{
    const int32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= a.S) return;
    const int32_t base = (a.auto_reset && (a.cell[s] & GU_CELL_TERM)) ? a.start0 : s;  // lazy `if done: env.reset()` (env:187-193)
    const uint32_t fb = a.cell[base];  // OPEN bits of the absorbing map: a terminal cell does not move (env:145-146)
    uint32_t out[4];
#pragma unroll
    for (uint32_t act = 0; act < 4; ++act) {
        const int32_t n = base + (((fb >> act) & 1u) ? gu_delta<false>(act, 0, a.W) : 0);
        const uint32_t d = (a.cell[n] >> GU_CELL_TERM_BIT) & 1u;
        const uint32_t r = (uint8_t)a.cell[a.cell_bytes + n];
        out[act] = ((uint32_t)n << a.row_shift) | (d << GU_ROW_DONE_BIT) | (r << 24);
    }
    *reinterpret_cast<uint4 *>(a.rows + 4 * (int64_t)s) = make_uint4(out[0], out[1], out[2], out[3]);
}

// Table-policy rows.  `thr` == nullptr: greedy (one dword per cell); else sampled (8 dwords per cell).
struct BuildPolicyRowsArgs {
    const uint8_t *cell;
    const uint8_t *greedy;  // first-argmax action per cell
    const uint4 *thr;       // inverse-CDF thresholds per cell
    int32_t cell_bytes, S, W, start0, auto_reset, row_shift;
    uint32_t *rows;
};

__device__ __forceinline__ uint32_t gu_row_record(const uint8_t *cell, int32_t cell_bytes, int32_t base, uint32_t act, int32_t W, int32_t row_shift)
{
    const uint32_t fb = cell[base];
    const int32_t n = base + (((fb >> act) & 1u) ? gu_delta<false>(act, 0, W) : 0);
    const uint32_t d = (cell[n] >> GU_CELL_TERM_BIT) & 1u;
    const uint32_t r = (uint8_t)cell[cell_bytes + n];
    return ((uint32_t)n << row_shift) | (d << GU_ROW_DONE_BIT) | (r << 24);
}

__global__ void __launch_bounds__(256) gu_build_policy_rows_kernel(const BuildPolicyRowsArgs a)
{
    const int32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= a.S) return;
    // the policy is consulted at the POST-reset cell, like the general kernel's table policies
    const int32_t base = (a.auto_reset && (a.cell[s] & GU_CELL_TERM)) ? a.start0 : s;
    if (!a.thr) {
        a.rows[s] = gu_row_record(a.cell, a.cell_bytes, base, a.greedy[base], a.W, a.row_shift);
        return;
    }
    // The step's action is  #{k : word >= thr_k} - never  (gu_sample_action; thresholds no word can reach are stored as 0 and
    // counted in `never`).  A count does not care about the order of its thresholds: with them SORTED, "word >= the c-th" implies
    // "word >= every one before it", and the record of count c can be picked by three chained selects -- 3 compares + 3 selects
    // on the step's dependent chain instead of the count, its carry adds, and a two-level select on the action's bits (21
    // instructions with their wait states).  The records are stored BY COUNT: entry c = the record of action c - never.
    uint4 *out = reinterpret_cast<uint4 *>(a.rows + 8 * (int64_t)s);
    const uint4 q = a.thr[base];
    uint32_t t0 = q.x, t1 = q.y, t2 = q.z;
    if (t0 > t1) { const uint32_t x = t0; t0 = t1; t1 = x; }
    if (t1 > t2) { const uint32_t x = t1; t1 = t2; t2 = x; }
    if (t0 > t1) { const uint32_t x = t0; t0 = t1; t1 = x; }
    out[0] = make_uint4(t0, t1, t2, q.w);
    uint32_t rec[4];
#pragma unroll
    for (uint32_t c = 0; c < 4; ++c) {
        const uint32_t act = c >= q.w ? (c - q.w > 3u ? 3u : c - q.w) : 0u;  // (a count below `never` cannot occur)
        rec[c] = gu_row_record(a.cell, a.cell_bytes, base, act, a.W, a.row_shift);
    }
    out[1] = make_uint4(rec[0], rec[1], rec[2], rec[3]);
}

// PAIR tables (uniform policy / caller-supplied stream, launches that write rows): TWO env-steps per LDS round trip.  The actions
// of these policies do not depend on the env state, so the transitions of two consecutive steps compose ahead of time like the
// K-step tables of gu_rollout_multi.hip -- but here every step leaves a trajectory row behind, so an entry keeps BOTH records:
//
//     pair[s][a1 | a2 << 2] = { record reached by a1 from s,  record reached by a2 from there }          (8 bytes, 128 per cell)
//
// each in the format above with the cell's PAIR row as its address.  One ds_read_b64 then advances an env by two steps, and the
// two records are emitted beside the chain as before.  Steps that do not fill a pair of an action word (the first step of a
// launch, the steps up to the next 16-step word, the last T mod 16) run on a one-step table of the same record format that sits
// behind the pair table in LDS (144 bytes per cell in all: grids of up to ~1100 cells, one workgroup per CU).  What it buys:
// launches bound by the dependent chain, not by the write path -- packed rows at 65 536 envs, int32 rows at a config-4 shard of
// 32 768 envs (profiles/archive/r03r_pair_rows.txt).
__device__ __forceinline__ uint32_t gu_row_record(const uint8_t *cell, int32_t cell_bytes, int32_t base, uint32_t act, int32_t W, int32_t row_shift);

struct BuildPairRowsArgs {
    const uint8_t *cell;
    int32_t cell_bytes, S, W, start0, auto_reset;
    uint32_t *rows2;  // [S][16][2] pair records, then [S][4] one-step records (row_shift 7)
};


__global__ void __launch_bounds__(256) gu_build_pair_rows_kernel(const BuildPairRowsArgs a)
{
    const int32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= a.S * 16) return;
    const int32_t s = idx >> 4;
    const uint32_t a1 = (uint32_t)idx & 3u, a2 = ((uint32_t)idx >> 2) & 3u;
    const int32_t b1 = (a.auto_reset && (a.cell[s] & GU_CELL_TERM)) ? a.start0 : s;  // lazy `if done: env.reset()` (env:187-193)
    const uint32_t r1 = gu_row_record(a.cell, a.cell_bytes, b1, a1, a.W, GU_PAIR_SHIFT);
    const int32_t n1 = (int32_t)((r1 & GU_ROW_ADDR_MASK) >> GU_PAIR_SHIFT);
    const int32_t b2 = (a.auto_reset && (a.cell[n1] & GU_CELL_TERM)) ? a.start0 : n1;
    const uint32_t r2 = gu_row_record(a.cell, a.cell_bytes, b2, a2, a.W, GU_PAIR_SHIFT);
    reinterpret_cast<uint2 *>(a.rows2)[idx] = make_uint2(r1, r2);
}

typedef __attribute__((address_space(3))) const uint32_t *lds_u32_ptr;
typedef uint32_t gu_v2u __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) const gu_v2u *lds_v2u_ptr;
typedef uint32_t gu_v4u __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) const gu_v4u *lds_v4u_ptr;

// bytes per row (log2): 4 next records / one record / thresholds + 4 next records
template <int POLICY>
struct RowBytes {
    static constexpr int log2 = POLICY == GU_POLICY_GREEDY ? 2 : POLICY == GU_POLICY_SAMPLE ? 5 : 4;
};

// nothing but the chain between the arrival of a record and the issue of the read it addresses (see word16)
#define GU_CHAIN_FENCE() __builtin_amdgcn_sched_barrier(0)
// (workgroups of up to 512 lanes, i.e. 256 registers: the staging below keeps up to twelve 16-byte rows per lane in flight beside the
// 32 registers of the first wave's pacing slots)
template <int POLICY, int TRAJ, bool STATS, bool PAIR = false>
__global__ void __launch_bounds__(GU_ROWS_MAX_BLOCK) gu_rollout_rows_kernel(const RolloutArgs a, const int32_t auto_reset)
{
    static_assert(!PAIR || POLICY == GU_POLICY_UNIFORM || POLICY == GU_POLICY_STREAM, "pair tables: policies whose actions do not depend on the state");
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    GuPacer pacer;
    pacer.fetch(a.pace, TRAJ != 0);  // (asked for ahead of the staging: gu_rollout.hpp)
    const int32_t shift = PAIR ? GU_PAIR_SHIFT : a.row_shift;  // log2(row bytes * copies)
    const int32_t copies_log2 = shift - RowBytes<POLICY>::log2;
    // LDS address of the staged table.  This kernel has no static LDS: its dynamic block starts at LDS address 0 and a record's
    // address bits ARE the ds_read address -- no base is added on the dependent chain.  (Until late in round 5 the block's address
    // was folded into every record; the compiler cannot know that it is 0 -- a link-time constant to it -- and spent one vector
    // instruction per emitted record on `rec - base`, a seventh of config 2's per-step vector work.  The launcher checks it:
    // gu_lds_launch refuses an instantiation that reports static LDS.)
    constexpr uint32_t lds_base = 0u;
    // ---- The launch's fixed cost (round 5: 8.6 us of a 60 us config-4 shard, profiles/archive/r05r_rows_intercept.txt) is LATENCY: the table
    // came in through four dependent rounds of global loads (every copy of a row fetched separately, eight loads in flight), and
    // the first step's three dependent global reads (state -> the cell's flags -> the next cell's flags and reward) started behind
    // the staging barrier.  Now: every SOURCE row is loaded once, all of a thread's loads in flight together, and written to its
    // `copies` places from registers; the env's state is asked for right behind the table's first loads; and the first step's reads
    // are issued between the stages of that, so that their round trips pass under it.
    const uint32_t half = (uint32_t)a.half_waves;
    const uint32_t slot_in_block = half ? ((threadIdx.x >> 6) << 5) | (threadIdx.x & 31u) : threadIdx.x;
    const int64_t e64 = (int64_t)gu_env_block(a.xcd_remap) * (blockDim.x >> half) + slot_in_block;
    const bool live = e64 < a.N && !(half && (threadIdx.x & 32u));
    const uint32_t e = live ? (uint32_t)e64 : 0u;  // (a lane without an env reads the state of env 0 and stores nothing)
    const uint32_t prefix = gu_rng_prefix(a.seed_prefix, a.env_id0 + e);
    const int32_t start0 = auto_reset ? a.starts[0] : 0;
    const char *pa = (const char *)a.actions;
    const uint32_t e4 = e * 4u;
    // First step of the launch, on the per-cell planes: the stored done flag decides the lazy reset (it may disagree with the
    // cell: fresh reset onto a terminal start, gu_set_state).  In four parts, each one global round trip behind the one before:
    // the state; the (post-reset) cell's flags and what the policy wants to know there; the flags and the reward of the cell the
    // move ends on; the record.  (The `asm volatile` pins: left to itself the compiler hoists the first USE of a load to right
    // behind its issue -- a wait for the state ahead of the table's loads.)
    int32_t s = 0;
    uint32_t d = 0, ep = 0, t_lane = 0, f0 = 0, first_x = 0, f1 = 0, r1 = 0, first_word = 0;
    uint4 first_thr = make_uint4(0u, 0u, 0u, 0u);
    auto first_0 = [&]() {
        uint32_t ee = e;
        asm volatile("" : "+v"(ee));
        s = a.pos[ee];
        d = (uint32_t)a.done[ee];
        ep = a.episode[ee];
        t_lane = a.tcount[ee];
    };
    // ... unless the state was left by a rollout (a.entry_table: gu_launch_rollout vouches for it).  Then the done flag IS the TERM bit
    // of the cell, the table's rows apply to the first step like to any other, and the launch's fixed cost is ONE global round
    // trip (the state, under the staging) instead of three.
    const bool entry_table = a.entry_table != 0;
    auto first_a = [&]() {
        asm volatile("" : "+v"(t_lane), "+v"(s), "+v"(d));
        t_lane += a.steps_taken;
        if (POLICY == GU_POLICY_SAMPLE) first_word = gu_rng_sample_word(prefix, t_lane);
        if (auto_reset && d) {
            if (!entry_table) s = start0;  // (on the table the row of a terminal cell is the row of the start cell)
            ++ep;
        }
        if (!entry_table) {
            f0 = a.cell[s];
            if (POLICY == GU_POLICY_GREEDY) first_x = a.greedy[s];
            if (POLICY == GU_POLICY_SAMPLE) first_thr = a.pi_thr[s];
        }
        if (POLICY == GU_POLICY_UNIFORM) first_x = (gu_rng_word(prefix, GU_RNG_STREAM_ACTION, t_lane >> 4) >> (2u * (t_lane & 15u))) & 3u;
        if (POLICY == GU_POLICY_STREAM) first_x = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(__builtin_amdgcn_make_buffer_rsrc((void *)pa, 0, 0xFFFFFFFFu, 0x00020000), e4, 0, 0) & 3u;
    };
    auto first_b = [&]() {
        if (entry_table) return;
        asm volatile("" : "+v"(f0));
        const uint32_t act = POLICY == GU_POLICY_SAMPLE ? gu_sample_action(first_word, first_thr) : first_x;
        const int8_t *rew = reinterpret_cast<const int8_t *>(a.cell + a.cell_bytes);
        s += ((f0 >> act) & 1u) ? gu_delta<false>(act, 0, a.W) : 0;
        f1 = a.cell[s];
        r1 = (uint32_t)(uint8_t)rew[s];
    };
    {
        uint4 *dst = reinterpret_cast<uint4 *>(smem);
        const uint32_t copies = 1u << copies_log2;
        if (POLICY == GU_POLICY_GREEDY && copies_log2 < 2) {  // (fewer than four copies of a dword row: the old way, dword by dword)
            const int32_t units = (a.S << shift) >> 4;
            first_0();
            first_a();
#pragma unroll 8
            for (int32_t u = threadIdx.x; u < units; u += blockDim.x) {
                const int32_t d0 = u << 2;
                uint4 v = make_uint4(a.rows[d0 >> copies_log2], a.rows[(d0 + 1) >> copies_log2], a.rows[(d0 + 2) >> copies_log2], a.rows[(d0 + 3) >> copies_log2]);
                v.x += lds_base, v.y += lds_base, v.z += lds_base, v.w += lds_base;
                dst[u] = v;
            }
            first_b();
        } else {
            // Source rows: the LDS image itself (PAIR: pair table, then the one-step table; nothing is replicated), or one dword per
            // cell (greedy), one 16-byte unit per cell (uniform / stream), two per cell (sampled: thresholds, next records), each
            // written to `places` places: place k of a row is copy (k + cell) mod copies, so that the lanes of a store, which hold
            // consecutive cells, hit different 16-byte slots of the bank row instead of all the same one.
            // No guards: a lane beyond the end works on the LAST row again, same value to the same place, and the code is chosen once,
            // by the number of source rows per thread, among straight-line variants.  (A per-lane guard is an exec-mask region of ~25
            // clocks around every one of a thread's 30 .. 60 loads and stores; wave-uniform guards make the compiler wait for ALL loads
            // before every guarded one -- for all it knows a guarded load's guarded use was skipped --; an unrolled loop with a
            // `break` came back as a loop over an array in scratch memory.)
            const int32_t B = (int32_t)blockDim.x, log2_b = 31 - __builtin_clz((uint32_t)B);
            const int32_t n_src = PAIR ? a.S * 9 : POLICY == GU_POLICY_SAMPLE ? 2 * a.S : a.S;
            const uint4 *g4 = reinterpret_cast<const uint4 *>(PAIR ? a.rows2 : a.rows);
            const uint32_t places = PAIR ? 1u : POLICY == GU_POLICY_GREEDY ? copies >> 2 : copies;  // 16-byte places per source row
            auto put = [&](uint4 v, int32_t g) {
                if (PAIR || (POLICY != GU_POLICY_GREEDY && (POLICY != GU_POLICY_SAMPLE || (g & 1)))) v.x += lds_base, v.y += lds_base, v.z += lds_base, v.w += lds_base;
                if (PAIR) {
                    dst[g] = v;
                    return;
                }
                const uint32_t cell = POLICY == GU_POLICY_SAMPLE ? (uint32_t)g >> 1 : (uint32_t)g;
                auto at = [&](uint32_t k) {
                    const uint32_t place = (k + cell) & (places - 1u);
                    return POLICY == GU_POLICY_SAMPLE ? ((cell * places + place) << 1) | ((uint32_t)g & 1u) : cell * places + place;
                };
                if (places == 8u) {
#pragma unroll
                    for (uint32_t k = 0; k < 8u; ++k) dst[at(k)] = v;
                } else if (places == 4u) {
#pragma unroll
                    for (uint32_t k = 0; k < 4u; ++k) dst[at(k)] = v;
                } else {
                    for (uint32_t k = 0; k < places; ++k) dst[at(k)] = v;
                }
            };
            // NB rows per thread from `base` on: all loads out, `between()`, then the stores
            auto stage = [&](auto nb, int32_t base, auto between) {
                constexpr int NB = decltype(nb)::value;
                uint4 v[NB];
#pragma unroll
                for (int32_t j = 0; j < NB; ++j) {
                    const uint32_t g = (uint32_t)min(base + j * B + (int32_t)threadIdx.x, n_src - 1);  // (unsigned: base register + 32-bit offset, no address pair per load)
                    if (POLICY == GU_POLICY_GREEDY && !PAIR) {
                        const uint32_t w = a.rows[g] + lds_base;
                        v[j] = make_uint4(w, w, w, w);
                    } else {
                        v[j] = g4[g];
                    }
                }
                __builtin_amdgcn_sched_barrier(0);  // (the state BEHIND the table's loads: an address of theirs otherwise waits for it, see first_0)
                between();
#pragma unroll
                for (int32_t j = 0; j < NB; ++j) put(v[j], min(base + j * B + (int32_t)threadIdx.x, n_src - 1));
            };
            auto first_0a = [&]() {
                first_0();
                first_a();
            };
            auto nothing = []() {};
            const int32_t rows_total = (n_src + B - 1) >> log2_b;  // source rows per thread
            if (rows_total <= 1) {
                stage(std::integral_constant<int, 1>{}, 0, first_0a);
                first_b();
            } else if (rows_total <= 2) {
                stage(std::integral_constant<int, 2>{}, 0, first_0a);
                first_b();
            } else if (rows_total <= 4) {
                stage(std::integral_constant<int, 4>{}, 0, first_0a);
                first_b();
            } else if (TRAJ != 0 && rows_total <= 8) {
                stage(std::integral_constant<int, 8>{}, 0, first_0a);
                first_b();
            } else {
                // (launches that write no rows run several workgroups per CU: they keep to four rows in flight, 16 registers)
                constexpr int WIDE = TRAJ == 0 ? 4 : 12;
                stage(std::integral_constant<int, WIDE>{}, 0, first_0a);
                stage(std::integral_constant<int, WIDE>{}, WIDE * B, first_b);
#pragma unroll 1
                for (int32_t base = 2 * WIDE * B; base < n_src; base += WIDE * B) stage(std::integral_constant<int, WIDE>{}, base, nothing);
            }
        }
        __syncthreads();
    }
    // HALF WAVES (a.half_waves, round 5): lanes 0 .. 31 of every wave carry an env, the others leave -- twice as many waves for the
    // batch.  (The idea: a wave that has its SIMD to itself is bound by its own in-order issue, and the row stores might cost by the
    // lanes they carry.  They do not -- see the launcher for what was measured and where this is used.)
    if (half) pacer.decide_early(a.pace);  // (the launch's first wave sums the launch before while it still has its 64 lanes)
    if (!live) return;
    const uint32_t lane_copy = PAIR ? 0u : (threadIdx.x & ((1u << copies_log2) - 1u)) << RowBytes<POLICY>::log2;  // this lane's copy of every row
    const uint32_t base1 = lds_base + ((uint32_t)a.S << GU_PAIR_SHIFT);  // PAIR: the one-step table behind the pair table

    int32_t ret = 0;
    uint32_t fin = 0;
    uint32_t rec;

    char *po = (char *)a.tr_obs, *pr = (char *)a.tr_reward, *pd = (char *)a.tr_done;
    const int64_t row = a.N * 4;
    // the trajectory's own row pitch and lane offset (TRAJ == 3: one row of (obs, reward, done) triples per step, gu_rollout.hpp)
    const int64_t trow = TRAJ == 3 ? a.N * 12 : row;
    const uint32_t trow32 = (uint32_t)trow;
    const uint32_t te = TRAJ == 3 ? e * 12u : e4;
    __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc(po, 0, 0xFFFFFFFFu, 0x00020000);
    __amdgpu_buffer_rsrc_t rr = __builtin_amdgcn_make_buffer_rsrc(pr, 0, 0xFFFFFFFFu, 0x00020000);
    __amdgpu_buffer_rsrc_t rd = __builtin_amdgcn_make_buffer_rsrc(pd, 0, 0xFFFFFFFFu, 0x00020000);
    auto rebase = [&](int64_t rows) {
        po += rows * trow;
        ro = __builtin_amdgcn_make_buffer_rsrc(po, 0, 0xFFFFFFFFu, 0x00020000);
        if (TRAJ == 1) {
            pr += rows * trow;
            pd += rows * trow;
            rr = __builtin_amdgcn_make_buffer_rsrc(pr, 0, 0xFFFFFFFFu, 0x00020000);
            rd = __builtin_amdgcn_make_buffer_rsrc(pd, 0, 0xFFFFFFFFu, 0x00020000);
        }
    };
    // everything a step leaves behind hangs off the record that the step fetched -- none of it is on the chain.  It is
    // emitted one iteration late, i.e. AFTER the next step's LDS read has been issued, so that it fills that read's latency
    // instead of delaying its issue: iteration i fetches record i and emits record i - 1 into trajectory row i - 1.
    auto emit = [&](uint32_t rec, uint32_t soff) {
        const int32_t r = (int32_t)rec >> 24;
        const uint32_t dn = __builtin_amdgcn_ubfe(rec, GU_ROW_DONE_BIT, 1);
        fin += dn;
        if (STATS) ret += r;
        if (TRAJ) {
            const int32_t cell = (int32_t)__builtin_amdgcn_ubfe(rec - lds_base, (uint32_t)shift, 20u - (uint32_t)shift);
            if (TRAJ == 1) {
                __builtin_amdgcn_raw_buffer_store_b32(cell, ro, e4, soff, GU_STORE_AUX);
                __builtin_amdgcn_raw_buffer_store_b32(r, rr, e4, soff, GU_STORE_AUX);
                __builtin_amdgcn_raw_buffer_store_b32((int32_t)dn, rd, e4, soff, GU_STORE_AUX);
            } else if (TRAJ == 3) {
                const gu_v3u triple = {(uint32_t)cell, (uint32_t)r, dn};
                __builtin_amdgcn_raw_buffer_store_b96(triple, ro, te, soff, GU_STORE_AUX);
            GU_WIDE_STORE_PAD();
            } else {
                __builtin_amdgcn_raw_buffer_store_b32((int32_t)((uint32_t)cell | (((uint32_t)r & 0xFFu) << 16) | (dn << 24)), ro, e4, soff, GU_STORE_AUX_PACKED);
            }
        }
    };
    // last part of the launch's first step (its loads were issued under the staging, above): the record it ends on -- or, on the
    // table, the record the state at entry stands for (only its address counts: it is never emitted)
    rec = (((uint32_t)s << shift) + lds_base) | (((f1 >> GU_CELL_TERM_BIT) & 1u) << GU_ROW_DONE_BIT) | (r1 << 24);
    // `x`: the action (uniform / stream), nothing (greedy), the step's RNG word (sample); `between`: work that does not depend
    // on the env state (hashing the next step's RNG word), placed between the issue of the LDS reads and their first use
    auto step_e = [&](uint32_t x, uint32_t soff, auto between, auto emits) {
        const uint32_t prev = rec;
        if (POLICY == GU_POLICY_SAMPLE) {
            const uint32_t addr = (prev & GU_ROW_ADDR_MASK) | lane_copy;
            const gu_v4u q = *(lds_v4u_ptr)(uintptr_t)addr;            // thresholds of the cell ...
            const gu_v4u nx = *(lds_v4u_ptr)(uintptr_t)(addr + 16u);   // ... and its four next records, one round trip
            __builtin_amdgcn_sched_barrier(0);  // the two reads are issued BEFORE the ~17 vector ops of the hash, not behind them
            between();
            __builtin_amdgcn_sched_barrier(0);
            // sorted thresholds, records by count (gu_build_policy_rows_kernel).  The three compares FIRST, into three condition
            // registers, then the three selects: interleaved, every compare wrote VCC and every select waited out the two wait
            // states behind it -- twelve issue slots on the step's dependent chain instead of six.
            const bool c0 = x >= q.x, c1 = x >= q.y, c2 = x >= q.z;
            __builtin_amdgcn_sched_barrier(0);  // (statistics only 68.2 -> 65.0 us, packed rows 76.0 -> 73.7 at config 3; int32 rows, bound by their stores: 114 either way)
            // (A tree two selects deep -- lo = c0 ? y : x, hi = c2 ? w : z, rec = c1 ? hi : lo, which the sorted thresholds allow -- was
            // measured SLOWER than the chain of three: 55.4 against 54.7 us statistics only, 114 .. 115.5 against 113 with rows, round 5.)
            uint32_t sel = c0 ? nx.y : nx.x;
            sel = c1 ? nx.z : sel;
            rec = c2 ? nx.w : sel;
            asm volatile("" ::"v"(q.w));  // keep the unused fourth word of the read live up to here: the compiler otherwise takes its
                                          // register for the hash's temporaries and has to WAIT for the read before the hash can start
        } else if (POLICY == GU_POLICY_GREEDY) {
            rec = *(lds_u32_ptr)(uintptr_t)((prev & GU_ROW_ADDR_MASK) | lane_copy);
            between();
        } else {
            between();
            if (PAIR) {  // (a step outside the pairs: its 16-byte row of the one-step table; records carry PAIR-row addresses)
                rec = *(lds_u32_ptr)(uintptr_t)(base1 + (((prev & GU_ROW_ADDR_MASK) - lds_base) >> 3) + (x << 2));
            } else {
                uint32_t actoff = lane_copy | (x << 2);  // off the chain (the action does not depend on the env state)
                asm("" : "+v"(actoff));                  // keep it ONE value: otherwise the three-way OR is re-associated onto the chain
                const uint32_t addr = (prev & GU_ROW_ADDR_MASK) | actoff;  // v_and_or_b32: the only vector op between two LDS reads
                rec = *(lds_u32_ptr)(uintptr_t)addr;
            }
        }
        if (decltype(emits)::value) emit(prev, soff);
    };
    auto step = [&](uint32_t x, uint32_t soff, auto between) { step_e(x, soff, between, std::true_type{}); };
    auto nothing = [] {};
    // the first step on the table (a.entry_table): like any other, but the record it starts from is nobody's row
    if (entry_table) step_e(POLICY == GU_POLICY_SAMPLE ? first_word : first_x, 0, nothing, std::false_type{});
    pacer.start(a.pace, TRAJ != 0);
    const int32_t T32 = (int32_t)a.T;
    auto step1 = [&](uint32_t x) {
        step(x, 0, nothing);
        if (TRAJ) rebase(1);
    };
    // the 16 steps of one action word.  PAIR: eight round trips of two steps each; the records of a pair are emitted one round
    // trip late, behind the issue of the next read (rows base .. base + 15, the last record stays pending like everywhere here)
    auto word16 = [&](uint32_t word) {
        if (PAIR) {
            uint32_t r1[8], r2[8];
#pragma unroll
            for (uint32_t q = 0; q < 8; ++q) {
                const uint32_t prev = q ? r2[q - 1] : rec;
                uint32_t off = __builtin_amdgcn_ubfe(word, 4 * q, 4) << 3;  // off the chain
                asm("" : "+v"(off));
                // (nothing but the chain between the arrival of `prev` and the issue of the next read: left to itself the scheduler
                // put ~10 instructions of the records' emission there, ~50 clocks on every round trip of a wave that has its SIMD alone)
                GU_CHAIN_FENCE();
                const gu_v2u pr = *(lds_v2u_ptr)(uintptr_t)((prev & GU_ROW_ADDR_MASK) | off);
                GU_CHAIN_FENCE();
                r1[q] = pr.x;
                r2[q] = pr.y;
                if (q == 0) {
                    emit(rec, 0);
                } else {
                    emit(r1[q - 1], (2 * q - 1) * trow32);
                    emit(r2[q - 1], (2 * q) * trow32);
                }
            }
            emit(r1[7], 15 * trow32);
            rec = r2[7];
        } else {
#pragma unroll
            for (uint32_t j = 0; j < 16; ++j) step(__builtin_amdgcn_ubfe(word, 2 * j, 2), j * trow32, nothing);
        }
    };

    if (POLICY == GU_POLICY_UNIFORM) {
        uint32_t t = t_lane;
        uint32_t word = gu_rng_word(prefix, GU_RNG_STREAM_ACTION, t >> 4);  // (the first step is taken: first_a / first_b)
        ++t;
        int32_t i = 1;  // (32-bit counters: gu_rollout caps T at 1e8; the 64-bit ones cost the loop three scalar instructions per group)
        const uint32_t t_first = __builtin_amdgcn_readfirstlane(t);
        if (__all(t == t_first)) {  // every lane at the same step count: the 16-actions-per-word schedule is wave-uniform
            t = t_first;
            if (t & 15u) {  // head: finish the current word
                word = gu_rng_word(prefix, GU_RNG_STREAM_ACTION, t >> 4);
                for (; i < T32 && (t & 15u); ++i, ++t) step1((word >> (2u * (t & 15u))) & 3u);
                pacer.after((uint32_t)i);
            }
            auto groups = [&](auto paced) {  // (two copies: GuPacer::idle)
                for (; i + 16 <= T32; i += 16, t += 16) {
                    word = gu_rng_word(prefix, GU_RNG_STREAM_ACTION, t >> 4);
                    word16(word);
                    if (TRAJ) rebase(16);
                    if (decltype(paced)::value && i + 16 < T32) pacer.after(16);  // (gu_rollout.hpp: GuPacer)
                }
            };
            if (TRAJ == 0 || pacer.idle()) groups(std::false_type{});
            else groups(std::true_type{});
            if (i < T32) {
                word = gu_rng_word(prefix, GU_RNG_STREAM_ACTION, t >> 4);
                for (uint32_t j = 0; i < T32; ++i, ++j) step1((word >> (2u * j)) & 3u);
            }
        } else {
            if ((t & 15u) == 0u) word = gu_rng_word(prefix, GU_RNG_STREAM_ACTION, t >> 4);
            for (; i < T32; ++i) {
                step1((word >> (2u * (t & 15u))) & 3u);
                ++t;
                if ((t & 15u) == 0u) word = gu_rng_word(prefix, GU_RNG_STREAM_ACTION, t >> 4);
            }
        }
    } else if (POLICY == GU_POLICY_GREEDY || POLICY == GU_POLICY_SAMPLE) {
        // first step on the planes; the policy is consulted at the post-reset cell
        uint32_t t = t_lane;
        uint32_t word = first_word;  // (the first step is taken: first_a / first_b)
        if (POLICY == GU_POLICY_SAMPLE) word = gu_rng_sample_advance(prefix, t, word);
        ++t;
        int32_t i = 1;  // (32-bit counters: gu_rollout caps T at 1e8; the 64-bit ones cost the loop three scalar instructions per group)
        auto pstep = [&](uint32_t soff) {  // the word of the NEXT step is hashed while this step's reads are in flight
            uint32_t next_word = 0u;
            step(word, soff, [&] {
                if (POLICY == GU_POLICY_SAMPLE) next_word = gu_rng_sample_advance(prefix, t, word);
            });
            word = next_word;
            ++t;
        };
        // Sampled policy, every lane at the same step count: a head of single steps up to a multiple of four, then groups of eight
        // in which the steps that start a word (the fourth and the eighth) are known at compile time -- no ballot, no branch.
        const uint32_t t_first = __builtin_amdgcn_readfirstlane(t);
        if (POLICY == GU_POLICY_SAMPLE && __all(t == t_first)) {
            t = t_first;
            for (; i < T32 && (t & GU_RNG_SAMPLE_MASK); ++i) {
                pstep(0);
                if (TRAJ) rebase(1);
            }
            if (i > 1) pacer.after((uint32_t)i);
            constexpr uint32_t G = GU_RNG_SAMPLE_MASK + 1u < 8u ? 8u : GU_RNG_SAMPLE_MASK + 1u;  // steps per unrolled group
            auto groups = [&](auto paced) {  // (two copies: GuPacer::idle)
                for (; i + G <= T32; i += G) {
#pragma unroll
                    for (uint32_t j = 0; j < G; ++j) {
                        uint32_t next_word = 0u;
                        step(word, j * trow32, [&] {
                            next_word = (j & GU_RNG_SAMPLE_MASK) == GU_RNG_SAMPLE_MASK ? gu_rng_sample_advance_at<true>(prefix, t, word) : gu_rng_sample_advance_at<false>(prefix, t, word);
                        });
                        word = next_word;
                        ++t;
                    }
                    if (TRAJ) rebase(G);
                    if (decltype(paced)::value && i + G < T32) pacer.after(G);
                }
            };
            if (TRAJ == 0 || pacer.idle()) groups(std::false_type{});
            else groups(std::true_type{});
        } else {
            auto groups = [&](auto paced) {  // (two copies: GuPacer::idle)
                for (; i + 8 <= T32; i += 8) {
#pragma unroll
                    for (uint32_t j = 0; j < 8; ++j) pstep(j * trow32);
                    if (TRAJ) rebase(8);
                    if (decltype(paced)::value && i + 8 < T32) pacer.after(8);
                }
            };
            if (TRAJ == 0 || pacer.idle()) groups(std::false_type{});
            else groups(std::true_type{});
        }
        for (; i < T32; ++i) {
            pstep(0);
            if (TRAJ) rebase(1);
        }
    } else {  // GU_POLICY_STREAM: packed words of 16 two-bit actions (gu_pack_actions_kernel), see gu_stream_run
        gu_stream_run(
            pa, row, e4, a.T, 1,
            [&](uint32_t word) {
                word16(word);
                if (TRAJ) rebase(16);
                pacer.after(16);
            },
            step1);
    }
    emit(rec, 0);  // the last step's record (row T - 1: every loop above leaves the row base one step behind)
    pacer.finish();
    // resets performed = steps that started from a done env = (done at entry: counted in first_step) + done flags seen
    // on every step but the last
    const uint32_t d_last = __builtin_amdgcn_ubfe(rec, GU_ROW_DONE_BIT, 1);
    if (auto_reset) ep += fin - d_last;
    a.pos[e] = (int32_t)__builtin_amdgcn_ubfe(rec - lds_base, (uint32_t)shift, 20u - (uint32_t)shift);
    a.reward[e] = (int32_t)rec >> 24;
    a.done[e] = (int32_t)d_last;
    a.episode[e] = ep;
    if (STATS) {
        a.ret[e] = ret;
        a.episodes_fin[e] = (int32_t)fin;
    }
    const uint64_t bits = __ballot(d_last != 0);
    if ((threadIdx.x & 63) == 0) {
        if (half) reinterpret_cast<uint32_t *>(a.done_bits)[e >> 5] = (uint32_t)bits;  // (this wave's 32 envs: one half of a ballot word)
        else a.done_bits[e >> 6] = bits;
    }
}

// ------------------------------------------------------------------------------------ host side
// (when this kernel takes a launch, and in which shape: gu_rollout_plan.hpp, gu_plan_rows)
// The tables the plan names: allocated on first use, built when they are not what the plan wants.  false: no memory for one
// (*no_pairs: for the pair tables; the one-step table would do).
bool gu_rows_ensure(gu_engine *h, const GuRolloutPlan &p, bool *no_pairs)
{
    const int which = p.which;
    const unsigned s_blocks = (unsigned)((h->S + 255) / 256);
    auto alloc = [](uint32_t **table, size_t bytes) {
        if (*table || hipMalloc(table, bytes) == hipSuccess) return true;
        (void)hipGetLastError();
        return false;
    };
    *no_pairs = false;
    if (p.table_policy) {
        // policy-dependent rows: rebuilt by every launch (one tiny kernel), like the threshold table itself
        if (!alloc(&h->d_prow, (size_t)h->S * 32)) return false;
        BuildPolicyRowsArgs b{h->d_cell, h->d_greedy, p.policy == GU_POLICY_SAMPLE ? h->d_pi_thr : nullptr, h->cell_bytes, h->S, h->W,
                              h->start0, which, p.table_shift, h->d_prow};
        hipLaunchKernelGGL(gu_build_policy_rows_kernel, dim3(s_blocks), dim3(256), 0, h->stream, b);
    } else {
        if (!h->d_rows[which]) h->rows_shift[which] = -1;
        if (!alloc(&h->d_rows[which], (size_t)h->S * 4 * sizeof(uint32_t))) return false;
        if (h->rows_shift[which] != p.table_shift) {
            BuildRowsArgs b{h->d_cell, h->cell_bytes, h->S, h->W, h->start0, which, p.table_shift, h->d_rows[which]};
            hipLaunchKernelGGL(gu_build_rows_kernel, dim3(s_blocks), dim3(256), 0, h->stream, b);
            h->rows_shift[which] = p.table_shift;
        }
    }
    if (p.pair) {
        if (!h->d_rows2[which]) h->rows2_built[which] = false;
        if (!alloc(&h->d_rows2[which], (size_t)h->S * 144)) {
            *no_pairs = true;
            return false;
        }
        if (!h->rows2_built[which]) {
            BuildPairRowsArgs b2{h->d_cell, h->cell_bytes, h->S, h->W, h->start0, which, h->d_rows2[which]};
            hipLaunchKernelGGL(gu_build_pair_rows_kernel, dim3((unsigned)((h->S * 16 + 255) / 256)), dim3(256), 0, h->stream, b2);
            BuildRowsArgs b1{h->d_cell, h->cell_bytes, h->S, h->W, h->start0, which, GU_PAIR_SHIFT, h->d_rows2[which] + (size_t)h->S * 32};
            hipLaunchKernelGGL(gu_build_rows_kernel, dim3(s_blocks), dim3(256), 0, h->stream, b1);
            h->rows2_built[which] = true;
        }
    }
    return true;
}

// false: an instantiation with static LDS below its table -- not this build; the launch fails loudly
// (the lists run backwards so that the kernels keep their order in the code object: an unchanged binary is how a change here is checked)
template <int POLICY, bool PAIR>
static bool rows_launch(gu_engine *h, const GuRolloutPlan &p, const RolloutArgs &a)
{
    bool ok = false;
    gu_pick<0, 3, 2, 1>(p.traj, [&](auto traj_c) {
        gu_pick<0, 1>(p.stats, [&](auto stats_c) {
            constexpr int TRAJ = decltype(traj_c)::value;
            constexpr bool STATS = decltype(stats_c)::value != 0;
            ok = gu_lds_launch<gu_rollout_rows_kernel<POLICY, TRAJ, STATS, PAIR>, true>(h, p.blocks, p.block, p.lds, a, (int32_t)p.which);
        });
    });
    return ok;
}

bool gu_rows_launch(gu_engine *h, const GuRolloutPlan &p, const RolloutArgs &a)
{
    switch (p.policy) {
    case GU_POLICY_UNIFORM: return p.pair ? rows_launch<GU_POLICY_UNIFORM, true>(h, p, a) : rows_launch<GU_POLICY_UNIFORM, false>(h, p, a);
    case GU_POLICY_STREAM: return p.pair ? rows_launch<GU_POLICY_STREAM, true>(h, p, a) : rows_launch<GU_POLICY_STREAM, false>(h, p, a);
    case GU_POLICY_GREEDY: return rows_launch<GU_POLICY_GREEDY, false>(h, p, a);
    default: return rows_launch<GU_POLICY_SAMPLE, false>(h, p, a);
    }
}
