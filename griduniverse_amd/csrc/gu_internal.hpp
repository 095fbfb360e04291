// gu_internal.hpp -- engine object shared by the translation units of libgu.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>
#include <string>
#include <vector>

#include "../../include/gu.h"
#include "../../include/gu_diag.h"

// ---- per-cell records (two byte planes, staged in LDS by every kernel) ----------------
// Compiled on the host from the row bit-planes handed to gu_set_grid().  Together they
// encode the reference transition core/envs/griduniverse_env.py:136-155 for a cell:
//   flags[s]  bits 0..3  OPEN[a]: move a (UP,RIGHT,DOWN,LEFT; env:51-56) changes the position,
//                        i.e. NOT (grid edge (env:51-54) | wall at the candidate cell (env:149)
//                        | -- in the "absorbing" map only -- the cell itself is terminal (env:145-146))
//             bit  4     is_terminal(cell)            (env:163-168)
//             bit  7     the cell itself is a wall (env:157-161); used by the path search only
//             bits 5, 6  reward_matrix[cell] == +10 / == -10 (redundant with the reward plane; lets a kernel
//                        that keeps a PRIVATE copy of the flags plane per lane do without the second plane)
//   reward[s] int8       reward_matrix[cell]: -1, +10 or -10   (env:80-90)
// so that one env-step is   s += OPEN[a] * delta[a];  flags = F[s];  reward = R[s];  done = TERM.
// Device layout: one buffer [flags: cell_bytes | reward: cell_bytes], cell_bytes = S rounded up to 16.
#define GU_CELL_OPEN_MASK 0x0Fu
#define GU_CELL_TERM 0x10u
#define GU_CELL_TERM_BIT 4
#define GU_CELL_RPLUS 0x20u
#define GU_CELL_RMINUS 0x40u
// Actions: 0..3 = UP, RIGHT, DOWN, LEFT (env:56); -4..-1 address the same list from its end (env:148 indexes a Python list: -1 is
// LEFT), i.e. action & 3; anything else is an IndexError in the reference and rejected here.
// A buffer store of more than 64 bits reads its data registers late: a vector instruction that overwrites them in the slot behind
// the store wins for the last lanes of every row of sixteen.  The compiler pads that hazard only for stores WITHOUT a scalar offset
// (the rule of earlier chips); on gfx950 it bites with one too -- wrong first words of 12-byte rows in lanes 12 .. 15 of every
// sixteen (tools/triples_race.py, profiles/r06t_triples_race.txt: every workgroup size but one).  Two wait states behind such a store.
// tests/test_gpu_wide_stores.py runs both store sites against the C oracle at every workgroup size, map and wave shape; a build with
// the pad defined away (make variant VARIANT=_nopad EXTRA="-D'GU_WIDE_STORE_PAD()='") is how that file is shown to see the hazard.
#ifndef GU_WIDE_STORE_PAD
#define GU_WIDE_STORE_PAD()                         \
    do {                                            \
        __builtin_amdgcn_sched_barrier(0);          \
        asm volatile("s_nop 1" ::: "memory");       \
        __builtin_amdgcn_sched_barrier(0);          \
    } while (0)
#endif
#define GU_ACTION_OK(raw) ((uint32_t)((int32_t)(raw) + 4) < 8u)
#define GU_CELL_WALL 0x80u  /* the cell itself is a wall (only the path search needs it: wall nodes have no edges) */

#define GU_BLOCK 256 /* workgroup of every kernel that has no reason for another size */
#define GU_MAX_LDS_CELLS 32767 /* both planes of grids up to 32 767 cells (64 KiB) are LDS-resident; larger read L2 */

#define GU_HOST_ERR_WORD 4
#define GU_HOST_COUNT_WORD 8

#define GU_STREAM_PAD_WORDS 4  // spare rows behind the packed action stream: the rollout kernels read up to four words ahead

// ---- closed-loop store pacing (gu_rollout.hpp: GuPacer, gu_pace_next) -----------------
struct GuPaceEntry {   // one launch of one kind: how it runs, the loop's state behind it, and -- afterwards -- what became of it; 128 bytes
    uint32_t period_q;    // the period of launch `seq`, in 1/64 ticks (the schedule uses the rounded tick count): written by the
    uint32_t seq;         // first wave of launch seq - 1 (gu_rollout.hpp: GuPacer::decide); an entry with another number is stale
    uint64_t t_start;     // 100 MHz clock when the launch's first workgroup began (written by that launch)
    uint32_t unpaced;     // 1: launch `seq` runs WITHOUT the limiter (a probe, or because the limiter does not pay for this kind)
    uint32_t phase;       // GU_PACE_NORMAL .. : where the loop's "does the limiter pay at all" cycle stands (GuPacer::decide)
    uint32_t left;        // launches left in this phase
    uint32_t ema_paced;   // ticks: launches WITH the limiter, from one launch's start to the next one's (running mean)
    uint32_t ema_unpaced; // ... and WITHOUT it (the mean of the last probe's launches)
    // the log: what the waves of the launch reported, summed by the first wave of launch seq + 1
    uint32_t verdict;     // 0 not summed yet, 1 on schedule, 2 behind (the log's bar: GuPaceArgs::bar_num)
    uint32_t waves;       // waves that reported
    uint32_t elapsed;     // ticks from start to report, the slowest wave
    uint32_t ended_late;  // waves that were more than two periods behind their schedule when they reported
    uint32_t max_behind;  // ticks: the most any of them was behind (0 when none was more than two periods behind)
    uint32_t report_steps; // the step count behind which this launch's waves reported (launches of one kind may differ in length)
    uint32_t groups;      // 16-step groups of this launch
    // the slow loop around the rule: which SHARE of waves behind is the best one to aim for on this buffer (GuPacer::decide)
    uint32_t dec_q;       // what the period comes down by per launch, 1/64 ticks: the rule aims for a share of dec_q / gain_q
    uint32_t block_left;  // launches left in this block (the first GU_PACE_BLOCK_SKIP of a block are not counted: the period is on its way)
    uint32_t block_sum;   // ticks: start-to-start intervals of the block's counted launches, summed
    uint32_t block_n;     // ... and how many
    uint32_t last_mean;   // ticks: the mean of the block before (0: none yet)
    uint32_t up;          // 1: the last change of dec_q was upwards
    uint32_t quiet;       // 1: the limiter is off and stays off for now -- the waves of launch `seq` report nothing, its first wave only
                          // counts the launch and keeps the start-to-start mean (what a kind that is better off unpaced pays: ~nothing)
    uint32_t reserved2[9];
};
static_assert(sizeof(GuPaceEntry) == 128, "GuPaceEntry is two cache lines' halves: 128 bytes");
#define GU_PACE_BLOCK 192u      /* launches per block of the slow loop ...                       */
#define GU_PACE_BLOCK_SKIP 64u  /* ... of which the first ones only let the period settle        */
#define GU_PACE_NORMAL 0   /* the limiter is on, the period follows the rule                                                      */
#define GU_PACE_PROBE_OFF 1 /* a few launches without the limiter: how long do they take?                                          */
#define GU_PACE_OFF 2      /* the launches without it were quicker: the kind runs without a limiter                               */
#define GU_PACE_PROBE_ON 3 /* ... until it is tried again for a few launches                                                      */
// What a wave leaves behind for the loop: ONE 8-byte plain store into its own slot of its launch's set (two sets per kind, by launch
// parity), a few groups before the end of the launch.  bit 63: reported; bits 0 .. 30: ticks from the wave's start to this moment.
// (NOT atomics.  Round 5's first version had every wave add its counts to one word of its launch's record: the 3072 agent-scope
// atomics of a launch were executed one after the other at ~11 ns each and added 34 us to every 105 us launch.  Spread over 32
// neighbouring cache lines they still cost 6 .. 9 us per launch -- the lines share a memory channel, and that is where device-scope
// atomics are executed; profiles/archive/r05a_pace_c3.txt, r05c_pace_c3.txt "held ... WITHOUT records".)
#define GU_PACE_RING 64u  /* entries per launch kind: the last 61 launches can be read back (gu_rollout_pace_log) */
struct GuPaceArgs {
    GuPaceEntry *ring;      // nullptr: `period` as it is (0 = no limiter), nothing recorded
    uint64_t *slots;        // [2][slot_stride]: the waves' reports of this launch (set seq & 1) and of the launch before it
    uint32_t seq;           // this launch's number within its kind (the host counts)
    uint32_t period;        // ring == nullptr or `fixed`: the period in ticks; else the period of a kind's first launch (the model)
    uint32_t lo, hi;        // the loop keeps the period within [lo, hi] ticks
    uint32_t groups;        // 16-step groups of this launch (T / 16): the length of its schedule in periods
    uint32_t report_at;     // the waves report once they have done this many steps (a few groups before the end: gu_rollout.hpp, GuPacer::report)
    uint32_t n_waves, slot_stride;  // waves of this launch; slots per set
    uint16_t bar_num;       // of 256: the log calls a launch BEHIND when a wave was more than bar_num / 256 of the schedule behind it
    uint16_t fixed;         // 1: run with `period` and only record (measurement aid: tools/pace_loop.py)
    uint32_t gain_q;        // 1/64 ticks: what the period goes up by after a launch in which EVERY wave fell behind (a share of the waves: that share of it)
    uint32_t dec_q;         // 1/64 ticks: what it comes down by, every launch
    uint32_t probe_every;   // launches between two looks at the other side (limiter off while it is on, on while it is off); 0 = never
    uint32_t adapt;         // 1: the slow loop moves the rule's aim (dec_q) by what the launches' start-to-start time says
};

enum { GU_OVERLAY_NONE = 0, GU_OVERLAY_WIND, GU_OVERLAY_FRUIT, GU_OVERLAY_DOORS, GU_OVERLAY_BOXES, GU_OVERLAY_ERRANDS };  // gu_engine::overlay

// What a learner carries from one launch to the next (gu_engine::carry; DESIGN.md "What the engine carries between calls"): the last
// call that touched the envs was a launch of `owner` under `key` -- gu_td_run's and gu_fa_run's SARSA action (key 0), gu_nstep_run's
// and gu_lambda_run's window (gu_nstep_key, gu_lambda_key), the episode buffers of gu_reinforce_run and gu_is_run (L).  The next
// launch of the same owner and key starts from it; any other call that touches the envs or the learner's tables drops it.
enum { GU_CARRY_NONE = 0, GU_CARRY_TD_SARSA, GU_CARRY_FA_SARSA, GU_CARRY_NSTEP, GU_CARRY_LAMBDA, GU_CARRY_REINFORCE, GU_CARRY_IS };
struct GuCarry {
    int owner = GU_CARRY_NONE;
    int32_t key = 0;
};

struct gu_engine {
    int device = -1;
    int n_cu = 256;                  // compute units of the device (hipDeviceAttributeMultiprocessorCount)
    int64_t lds_per_cu = 160 * 1024; // LDS bytes of one CU (the most one workgroup can ask for)
    bool gfx950 = true;              // the device the absolute figures in this library were measured on
    int64_t opt[GU_OPT_COUNT];       // gu_set_option values of this engine (GU_OPT_UNSET: the process default applies)
    int64_t opt_x[GU_OPT_X_COUNT];   // experiment switches (only a -DGU_EXPERIMENTS build ever sets them)
    hipStream_t stream = nullptr;
    hipEvent_t ev_begin = nullptr, ev_end = nullptr, ev_sync = nullptr;  // ev_sync: gu_sync's marker (no timing)
    std::vector<hipEvent_t> ev_marks;  // gu_timer_mark pool (grows on demand, reused)
    size_t n_marks = 0;

    int64_t N = 0;        // envs on this device
    int64_t env_id0 = 0;  // global id of env 0

    // grid
    bool has_grid = false;
    int32_t W = 0, H = 0, S = 0;
    int32_t cell_bytes = 0;          // S rounded up to 16
    uint8_t *d_cell = nullptr;       // absorbing-aware planes    [2 * cell_bytes]
    uint8_t *d_cell_raw = nullptr;   // care_about_terminal=False [2 * cell_bytes]
    // the overlay slot (gu_overlay.hip; DESIGN.md "Overlays"): wind, fruit, doors, boxes or errands -- a third byte plane behind the two cell
    // planes of a single-grid engine and, for all but wind, one uint32 word per env; at most one of them at a time
    int overlay = GU_OVERLAY_NONE;       // which one is set (GU_OVERLAY_*)
    uint8_t *d_overlay_cell = nullptr;   // [3 * cell_bytes] the planes of d_cell with the overlay's plane behind them -- what its kernels
                                         // stage in one piece; nullptr: none
    uint32_t *d_overlay_mask = nullptr;  // [N] fruit: the envs' masks of eaten fruit, doors: of open slots (bit = slot), boxes: the boxes'
                                         // cells (b bits each), errands: eaten | progress | instruction (gu_map.hpp); set to overlay_init by every reset (errands: their
                                         // own reset kernel draws the instruction); nullptr under wind
    int32_t overlay_bits = 0;            // bits of a mask in use: F fruit cells (1 .. 32), D door slots (1 .. 8), b * B under boxes, F + pb + ib
                                         // under errands, 0 under wind; gu_td_run's tables have S << overlay_bits rows
    uint32_t overlay_param = 0;          // wind: gust_q16, the gust probability in 1/65536; fruit: the three kinds' values as int8 bytes
                                         // 1 .. 3 (byte 0 zero), as the kernels take them; boxes: GU_BOX_PARAM (gu_map.hpp); errands: the instructions, one byte each
    uint32_t overlay_param2 = 0;         // errands: GU_ERRAND_PARAM2 (gu_map.hpp) -- the pay and the word's field widths; 0 for every other kind
    uint32_t overlay_init = 0;           // the mask value at reset: 0 for fruit and doors, the initial boxes' cells under boxes
    std::vector<uint8_t> box_flags;      // boxes: the grid's flags plane [S] on the host, kept by gu_set_boxes for gu_set_boxes_state's checks
    int32_t fruit_value[3] = {0, 0, 0};  // ... and as gu_get_fruit hands them back
    uint8_t *d_kind = nullptr;       // [n_grids][cell_bytes] texture class of every cell as the reference's viewer picks it
                                     // (rendering.py:119-133: goal, else lava, else wall, else ground = 3, 2, 1, 0) -- the flags
                                     // cannot tell a goal+lava cell from a lava cell; nullptr for device-generated mazes (no
                                     // overlaps there: the flags decide)
    uint64_t delta_lut = 0;          // int16 x 4: {-W, +1, +W, -1} (valid when W <= 32767)
    int32_t *d_starts = nullptr;     // [n_grids][max_starts]
    int32_t *d_nstarts = nullptr;    // [n_grids]
    int32_t n_starts = 0;            // of grid 0 (the only grid unless n_grids > 1)
    int32_t start0 = 0;              // first start cell of grid 0 (host copy)
    int32_t max_starts = 0;
    bool all_single_start = true;
    // several distinct grids of one shape: env e uses grid e / group (contiguous equal groups)
    int32_t n_grids = 1;
    int64_t group = 0;               // envs per grid = N / n_grids

    // SoA env state
    int32_t *d_out3 = nullptr;  // pos[N] | reward[N] | done[N]
    uint32_t *d_episode = nullptr;
    int32_t *d_out3_alt = nullptr;      // a second set of the env-state arrays: config 5's per-XCD launch writes its results there and
    uint32_t *d_episode_alt = nullptr;  // the sets change places when it did not give up (gu_vi_xcd.hip: gu_vi_xcd_fused_run)
    uint64_t *d_done_bits_alt = nullptr;
    uint32_t *d_nib = nullptr;     // [ceil(N / 64)][nib_dwords][64]: every env's grid at four bits per cell (gu_nibble_planes; rollout MAP 5)
    bool nib_valid = false;
    uint32_t *d_tcount = nullptr;  // per-env step-count OFFSET (read as int32); effective 64-bit count = steps_taken + offset
    uint64_t steps_taken = 0;      // lock-step counter since gu_seed (all envs step together)
    int64_t off_lo = 0, off_hi = 0;  // what the host knows of the offsets: off_lo <= every offset <= off_hi (gu_set_state, rejected actions)
    bool off_exact = true;           // ... and whether both bounds are attained (false behind a rejected action: read back when it matters)
    uint64_t seed = 0;
    uint32_t seed_prefix = 0;

    // device-resident action stream
    int32_t *d_actions = nullptr;
    uint32_t *d_actions_packed = nullptr;  // the same stream, 16 two-bit actions per word: [ceil(T / 16)][N], what the rollout kernels read
    int64_t actions_T = 0;    // rows of the stream uploaded last (0: none / rejected)
    int64_t actions_cap = 0;  // rows the two buffers can hold

    // trajectory buffers obs|reward|done, each [traj_T][N]
    int32_t *d_traj = nullptr;
    int64_t traj_T = 0;
    int traj_kind = 0;  // what the last rollout left in the buffer: 0 nothing, 1 int32 rows (three planes), 2 packed rows, 3 int32 triples
    int traj_written = 0;  // ... as gu_launch_rollout chose it for the launch it issued last
    int32_t traj_candidates = 0;                // allocations tried for the buffer (gu_alloc_trajectory)
    float traj_probe_ms_best = 0.0f, traj_probe_ms_worst = 0.0f;
    std::vector<float> traj_probe_ms;           // per candidate, in the order tried
    std::vector<uint64_t> traj_probe_addr;
    int32_t traj_kept = -1;                     // index of the kept candidate
    float traj_search_ms = 0.0f;                // wall time of the search
    uint64_t traj_peak_bytes = 0;               // most device memory the search held at once
    bool traj_registered = false;               // counted in the per-device registry of chosen buffers

    // store pacing of the launches that write rows (gu_rollout.hpp: GuPacer): one ring of launch records per launch kind
    // (gu_rollout_plan.hpp: gu_pace_slot -- policy x auto mode for the general kernel, the transition-row kernel's int32 and packed rows)
    struct PaceKind {
        bool active = false;           // the kind's ring is in use
        const void *buffer = nullptr;  // the launch shape the ring belongs to: trajectory buffer, workgroups, launch length (within
        unsigned blocks = 0;           // a factor of two), bytes per env-step -- another shape starts the ring over
        int64_t T = 0;
        int row_bytes = 0;
        uint32_t seq = 0;              // launches of the kind recorded in the ring so far
        uint32_t model = 0;            // the period its first launch started from
        uint32_t n_waves = 0;          // waves of the kind's last launch (its reports: one word per wave)
    } pace[36];
    GuPaceEntry *d_pace_ring = nullptr;  // [36][GU_PACE_RING]
    uint64_t *d_pace_slots = nullptr;    // [36][2][pace_slot_stride] the waves' reports (allocated with the ring)
    int64_t pace_slot_stride = 0;
    int32_t rollout_form[12] = {};       // what the last rollout launch ran on (include/gu.h: gu_diag_rollout_form); zeros: none yet

    // transition-row tables of the latency-bound rollout (gu_rollout_rows.hip): [0] absorbing, [1] auto-reset folded in
    uint32_t *d_rows[2] = {nullptr, nullptr};
    int rows_shift[2] = {-1, -1};   // log2(16 * copies) the table was built for (-1: not built)
    uint32_t *d_rows2[2] = {nullptr, nullptr};  // pair tables (two steps per round trip) + the one-step table that goes with them
    bool rows2_built[2] = {false, false};
    // K-step tables of the statistics-only uniform rollout (gu_rollout_multi.hip) and the one-step tables that go with them
    uint32_t *d_mrows[2] = {nullptr, nullptr}, *d_mrows1[2] = {nullptr, nullptr};
    int mrows_K[2] = {0, 0}, mrows_shift[2] = {-1, -1};  // what they were built for (K = 0: not built)
    uint32_t *d_prow = nullptr;     // rows of the table policies (greedy: [S], sampled: [S][8]), rebuilt by every launch

    // rollout stats
    int32_t *d_ret = nullptr;
    int32_t *d_episodes_fin = nullptr;
    bool stats_valid = false;

    // done compaction: one ballot word per wave, written by every kernel that writes done[]
    uint64_t *d_done_bits = nullptr;
    bool entry_table_ok = false;    // the env state was left by a rollout (done flag == TERM bit of the cell, reward == the cell's): gu_rollout_rows.hip
    bool done_bits_valid = false;   // false only after the host installed done[] (gu_set_state)

    // scratch for masks / start choices / look_step_ahead
    void *d_scratch = nullptr;
    size_t scratch_bytes = 0;

    // pinned host staging (4*N int32)
    int32_t *h_pin = nullptr;
    double *h_tables = nullptr;     // page-locked copy of the DP tables [S] + [S][4]: the per-XCD launches of the tables alone write their results here too
    size_t h_tables_bytes = 0;      //   (gu_vi_xcd.hip), and a gu_vi_get behind such a call is two memcpys -- no launch, no wait
    bool h_tables_valid = false;    //   ... while nothing else has touched the tables since (every gu_vi_* call that may write them withdraws it)
    unsigned long long *h_ctl = nullptr;  // page-locked landing area of small results (gu_read_back): GU_CTL_WORDS 64-bit words
    char *h_up = nullptr;                 // page-locked staging of small uploads (GU_UP_BYTES): a copy from it is one DMA the stream orders,
                                          // a copy from the caller's pageable array is staged and waited for by the runtime
    uint32_t *h_seq = nullptr;      // page-locked control words (64 bytes): [0] completion word of gu_step's host-visible
                                    // paths, [GU_HOST_ERR_WORD] raised by a kernel that met an invalid action / state,
                                    // [GU_HOST_COUNT_WORD] number of done envs written by the compaction kernel
    uint32_t *d_blocks_done = nullptr;  // its device-side block counter
    uint32_t seq = 0, seq_since_sync = 0;

    // hipGraph cache for gu_step_graph
    hipGraphExec_t graph_exec = nullptr;
    int64_t graph_t0 = -1, graph_T = -1;
    uint32_t graph_flags = 0;

    // tabular DP
    double *d_v[2] = {nullptr, nullptr};
    double *d_pi[2] = {nullptr, nullptr};
    uint4 *d_pi_thr = nullptr;      // [S] inverse-CDF thresholds of d_pi[vi_cur], rebuilt by every GU_POLICY_SAMPLE rollout
    int vi_cur = 0;
    bool has_vi = false;
    double *d_delta = nullptr;      // per-block maxima + final
    uint8_t *d_greedy = nullptr;    // first-argmax action per state [cell_bytes]
    bool greedy_valid = false;
    int32_t vi_xcd_members[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // workgroups that registered per XCC in the last per-XCD launch of gu_vi_sweep_step_run
    int vi_run_form = 0;            // which form the last gu_vi_sweep_step_run took: 1 per XCD, 2 chip-wide cluster, 3 one launch per round
    void *d_vi_xcd_ctl = nullptr, *d_vi_xcd_work = nullptr;  // the per-XCD launches' own headers / keys / slots and granule buffers (gu_vi_xcd.hip)
    size_t vi_xcd_ctl_bytes = 0, vi_xcd_work_bytes = 0;
    uint32_t vi_xcd_epoch = 1;      // number of the next per-XCD launch (its tags carry it)
    int64_t vi_xcd_torn = 0;        // -DGU_VI_XCD_TORN builds: exchange words found with the right tag and the wrong payload, summed over the per-XCD launches
    int vi_dp_form = 0;             // ... and the last gu_vi_sweep / gu_vi_run / gu_vi_eval_run: 1 per XCD, 2 one workgroup, 3 chip-wide cluster, 4 one launch per round

    GuCarry carry;  // what the last call that touched the envs left for the next launch of the same learner (none: nothing carries)

    // batched tabular TD control (gu_td.hip): off until gu_td_init
    double *d_q = nullptr;        // [N][td_S][4] one float64 Q table per env
    int8_t *d_td_next = nullptr;  // [N] SARSA: the action a' carried from one launch to the next (-1: none)
    int32_t td_S = 0;             // states of the tables (0: none allocated); a grid of another size drops them
    // batched tabular n-step Q-learning / SARSA (gu_nstep.hip): learns into d_q; the window is allocated on first use
    int32_t *d_nstep_sa = nullptr;   // [N][GU_NSTEP_MAX] pending pairs s*4+a, oldest first
    int32_t *d_nstep_r = nullptr;    // [N][GU_NSTEP_MAX] their rewards
    int32_t *d_nstep_cnt = nullptr;  // [N] entries of the window
    // batched tabular SARSA(lambda) / Watkins's Q(lambda) (gu_lambda.hip): learns into d_q; the window is allocated on first use
    int32_t *d_lambda_w = nullptr;  // [N][GU_LAMBDA_MAX] the trace window, index = age (-1: none)
    // batched tabular softmax actor-critic (gu_ac.hip): off until gu_ac_init; tables of its own, not d_q
    double *d_ac_h = nullptr;  // [N][ac_S][4] preferences
    double *d_ac_v = nullptr;  // [N][ac_S] state values
    int32_t ac_S = 0;          // states of the tables (0: none allocated); a grid of another size drops them
    // batched tabular REINFORCE with baseline (gu_reinforce.hip): learns into d_ac_h / d_ac_v; the buffers are allocated on first use
    int32_t *d_rf_buf = nullptr;  // [rf_cap][N] the episode buffers, step-major, oldest first: 8-byte entries {s*4+a, r}
    int32_t *d_rf_cnt = nullptr;  // [N] their entries
    int32_t rf_cap = 0;           // entries per env the storage holds (0: none allocated)
    // batched off-policy Monte-Carlo control with weighted importance sampling (gu_is.hip): off until gu_is_init; learns into d_q
    double *d_is_c = nullptr;     // [N][is_S][4] cumulative weights
    int32_t is_S = 0;             // states of the weights (0: none allocated); a grid of another size drops them
    double *d_is_R = nullptr;     // [5][4] the ratio table of is_eps, R[c * 4 + m - 1]
    int64_t is_eps = -1;          // eps_q16 of the table on the device (-1: none yet)
    int32_t *d_is_buf = nullptr;  // [is_cap][N] the episode buffers, step-major, oldest first: 8-byte entries {s*4+a, r*8+c}
    int32_t *d_is_cnt = nullptr;  // [N] their entries
    int32_t is_cap = 0;           // entries per env the storage holds (0: none allocated)
    // batched semi-gradient SARSA / Q-learning on binary features (gu_fa.hip): off until gu_fa_init; weights of its own, not d_q
    double *d_fa_w = nullptr;         // [N][fa_F][4] one float64 weight table per env
    int32_t *d_fa_phi = nullptr;      // [fa_S][fa_K] the feature table, shared by all envs
    uint16_t *d_fa_phi16 = nullptr;   // ... as uint16 when fa_F <= 65536 (what the LDS kernels stage), padded to fa_phi16_bytes
    size_t fa_phi16_bytes = 0;        // fa_S * fa_K * 2 rounded up to 16
    int8_t *d_fa_next = nullptr;      // [N] SARSA: the action a' carried from one gu_fa_run to the next (-1: none)
    int32_t fa_S = 0, fa_K = 0, fa_F = 0;  // states, slots and features of the tables (fa_S 0: none); a grid of another size drops them
    // batched tabular Dyna-Q (gu_dyna.hip): off until gu_dyna_init; learns into d_q
    uint64_t *d_dyna_model = nullptr;  // [N][dyna_S*4] one packed word per (s, a): reward | (s' | done << 31) << 32; ~0 = unobserved
    int32_t *d_dyna_list = nullptr;    // [N][dyna_S*4] observed pairs s*4+a in the order of first observation (-1 beyond count)
    int32_t *d_dyna_count = nullptr;   // [N] entries of the list
    uint8_t *d_dyna_seen = nullptr;    // [N][dyna_S] bit a of byte s: (s, a) observed (the real step's test while dyna_exact)
    int32_t dyna_S = 0;                // states of the model (0: none allocated); a grid of another size drops it
    bool dyna_exact = false;           // every observed entry is what the current grid gives: no grid install since gu_dyna_init
    // batched prioritized sweeping (gu_sweep.hip): off until gu_sweep_init; learns into d_q from the Dyna-Q model above, with which
    // the queues are cleared (gu_dyna_init) and dropped (gu_dyna_free): they are sized by dyna_S
    uint64_t *d_sweep_heap = nullptr;  // [N][dyna_S*4+2] 1-based binary max-heap of keys (priority pattern | pair); slot 0: pops | inserts << 32
    int32_t *d_sweep_pos = nullptr;    // [N][dyna_S*4] the heap slot of each pair (-1: not queued)
    int32_t *d_sweep_size = nullptr;   // [N] keys in the heap
    // batched rollout search (gu_search.hip): decides and learns on d_q; allocated on first use, dropped with the tables
    double *d_search_score = nullptr;   // [N][4] the score row of each env's most recent searched iteration
    int64_t *d_search_steps = nullptr;  // [N] simulated moves of the last launch
    // batched count-based exploration (gu_explore.hip): off until gu_explore_init; chooses by and learns into d_q
    uint32_t *d_explore_n = nullptr;   // [N][explore_S][4] visit counts, saturating at GU_EXPLORE_COUNT_MAX
    int32_t explore_S = 0;             // states of the counts (0: none allocated); a grid of another size drops them
    double *d_explore_tab = nullptr;   // U[explore_C] | B[explore_C], shared by all envs (gu_explore_set_tables)
    int32_t explore_C = 0;             // entries of each (0: no tables yet)
    // batched Double Q-learning (gu_double.hip): off until gu_double_init; a pair of tables of its own, not d_q
    double *d_dq = nullptr;            // [N][dq_S][2][4] the A row and the B row of a state side by side: one aligned 64-byte piece
    int32_t dq_S = 0;                  // states of the pairs (0: none allocated); a grid of another size drops them
    // batched Monte-Carlo tree search (gu_mcts.hip): off until gu_mcts_init; decides and learns on d_q; dropped with the tables
    uint8_t *d_mcts_pool = nullptr;    // [N][mcts_P] nodes of 64 bytes: w[4] float64 | visits[4] uint32 | child[4] int32
    int32_t *d_mcts_meta = nullptr;    // [N][mcts_P][2] (state, parent * 4 + action; -1 for the root)
    int32_t *d_mcts_nodes = nullptr;   // [N] nodes of each env's most recent searched iteration (0: none yet)
    int64_t *d_mcts_steps = nullptr;   // [N] simulated moves of the last launch
    int32_t mcts_P = 0;                // nodes per env, max_sims + 1 (0: no pool)
    double *d_mcts_tab = nullptr;      // U[mcts_C] | B[mcts_C] | I[mcts_C], shared by all envs (gu_mcts_set_tables)
    int32_t mcts_C = 0;                // entries of each (0: no tables yet)

    // agent trail (gu_trail.hip): off unless gu_trail_enable was called
    int32_t trail_cap = 0;             // entries per env (0: off)
    int32_t *d_trail = nullptr;        // [N][trail_cap] ring of cells
    int32_t *d_trail_len = nullptr, *d_trail_head = nullptr;  // [N] each (one allocation)
    uint8_t *d_trail_done = nullptr;   // [N] done flag behind the last append
    uint32_t *d_trail_alpha = nullptr; // [trail_cap] alpha of the i-th newest entry, 16 fractional bits

    // RCCL
    void *comm = nullptr;  // ncclComm_t
    int32_t nranks = 0, rank = 0;
    int32_t *d_gather = nullptr;

    int32_t *pos() const { return d_out3; }
    int32_t *reward() const { return d_out3 + N; }
    int32_t *done() const { return d_out3 + 2 * N; }
};

// what the kernels need to find a lane's grid (by value in the kernel arguments)
struct GridSel {
    int64_t group;           // envs per grid
    int64_t grid_stride;     // bytes between consecutive grids' plane pairs (2 * cell_bytes)
    const int32_t *n_starts; // [n_grids]
    int32_t n_grids, max_starts;
    int32_t per_wave;        // LDS variants: every WAVE of a workgroup stages the planes of its own grid (groups of 64 .. 192 envs under
                             // workgroups of 256: the launch shape of the shared grid); 0: one grid per workgroup
};

inline GridSel gu_grid_sel(const gu_engine *h)
{
    return GridSel{h->group, 2 * (int64_t)h->cell_bytes, h->d_nstarts, h->n_grids, h->max_starts, 0};
}

// ---- error plumbing --------------------------------------------------------------
void gu_set_error(const char *fmt, ...);
int gu_fail(int code, const char *fmt, ...);

#define GU_HIP(expr)                                                                              \
    do {                                                                                          \
        hipError_t _e = (expr);                                                                   \
        if (_e != hipSuccess)                                                                     \
            return gu_fail(_e == hipErrorOutOfMemory ? GU_ERR_NOMEM : GU_ERR_HIP, "%s failed: %s", \
                           #expr, hipGetErrorString(_e));                                         \
    } while (0)

#define GU_REQUIRE(cond, code, ...) \
    do {                            \
        if (!(cond)) return gu_fail(code, __VA_ARGS__); \
    } while (0)

int gu_use_device(gu_engine *h);
int gu_ensure_scratch(gu_engine *h, size_t bytes);

#define GU_TRY(call)                                 \
    do {                                             \
        int _rc = (call);                            \
        if (_rc != GU_OK) return _rc;                \
    } while (0)

#define GU_ENTER(h) GU_TRY(gu_use_device(h))

#define GU_NEED_GRID(h) GU_REQUIRE((h)->has_grid, GU_ERR_STATE, "no grid set: call gu_set_grid first")

// What the messages call an overlay, and how they tell the caller that it is set and which call takes it away (index: GU_OVERLAY_*)
static const char *const GU_OVERLAY_NAME[6] = {"none", "wind", "fruit", "doors", "boxes", "errands"};
static const char *const GU_OVERLAY_IS_SET[6] = {"", "the engine has wind set (gu_set_wind; NULL calms it again)",
                                                 "the engine has fruit set (gu_set_fruit; NULL takes it away again)",
                                                 "the engine has doors set (gu_set_doors; NULL takes them away again)",
                                                 "the engine has boxes set (gu_set_boxes; NULL takes them away again)",
                                                 "the engine has errands set (gu_set_errands; NULL takes them away again)"};

// every call that moves envs or reads the move or reward rule and has no form for overlays refuses while one is set (include/gu.h:
// gu_set_wind, gu_set_fruit, gu_set_doors, gu_set_boxes, gu_set_errands)
#define GU_NO_OVERLAY(h, fn) \
    GU_REQUIRE(!(h)->overlay, GU_ERR_UNSUPPORTED, "%s knows no %s: %s", fn, GU_OVERLAY_NAME[(h)->overlay], GU_OVERLAY_IS_SET[(h)->overlay])

// frees device buffers and forgets them (hipFree's status is not looked at)
template <class... P>
static inline void gu_release(P *&...p)
{
    ((p ? (void)hipFree(p) : (void)0, p = nullptr), ...);
}

// ---- options (gu_options.hip) ----------------------------------------------------
// The value in force for `option`: the engine's own, else the process default, else the built-in one.  A few loads; called
// per launch.  (A -DGU_EXPERIMENTS build also consults the environment variable of the same name on every call, for the
// A/B tools.)
int64_t gu_opt(const gu_engine *h, int option);
int gu_debug();  // GU_DEBUG's level when the library was first asked (read once per process): 1 = one line per search / calibration, 2 = every candidate

// Raise the dynamic-LDS limit of one kernel instantiation once PER DEVICE (HIP keeps the attribute per device: a process
// that drives several GPUs must set it on each).  `mask` is a per-instantiation static.
template <typename K>
static inline void gu_allow_lds(K kern, std::atomic<uint64_t> &mask, int device, size_t bytes, size_t wanted)
{
    if (bytes <= 64 * 1024) return;
    const uint64_t bit = device < 64 ? (1ull << device) : 0;
    if (bit && (mask.load(std::memory_order_relaxed) & bit)) return;
    (void)hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)wanted);
    if (bit) mask.fetch_or(bit, std::memory_order_relaxed);
}

// ---- kernel launchers (gu_kernels.hip) -------------------------------------------
int gu_launch_reset(gu_engine *h, const uint8_t *d_mask, const int32_t *d_choice, bool only_done);
int gu_launch_step(gu_engine *h, const int32_t *d_actions_row, uint32_t flags, int32_t *host_obs = nullptr,
                   int32_t *host_reward = nullptr, int32_t *host_done = nullptr, uint32_t *host_seq = nullptr, uint32_t seq = 0,
                   uint32_t *host_err = nullptr);
int gu_launch_pack_actions(gu_engine *h, int64_t T);  // validates h->d_actions[0 .. T) and fills h->d_actions_packed
int gu_launch_rollout(gu_engine *h, int64_t T, int32_t policy, uint32_t flags);
int gu_launch_lookahead(gu_engine *h, int64_t n, const int32_t *d_states, const int32_t *d_actions, bool care,
                        int32_t *d_next, int32_t *d_reward, int32_t *d_done);
int gu_launch_done_compact(gu_engine *h);
int gu_launch_deinterleave(gu_engine *h, const int32_t *triples, int32_t *planes, int64_t count);  // [count][3] -> [3][count]
int gu_probe_trajectory_buffer(gu_engine *h, int32_t *buf, int64_t T, float *ms);  // one timed full write, rollout store shape
// Device-to-device copy by a kernel on the engine's stream (bytes a multiple of 4): the snapshots that the DP cluster launches take
// of the engine's state, and put back, stay on the kernel path (ordered with the launches around them, no copy-engine round trip
// for a few hundred KB).
int gu_device_copy(gu_engine *h, void *dst, const void *src, size_t bytes);
#define GU_MAX_SEGMENTS 8
struct GuSegments {  // gu_device_segments: copies (src != nullptr) and fills with zero (src == nullptr) of whole 32-bit words, one launch
    void *dst[GU_MAX_SEGMENTS];
    const void *src[GU_MAX_SEGMENTS];
    size_t words[GU_MAX_SEGMENTS];
    int n = 0;
    void add(void *d, const void *s, size_t bytes)
    {
        dst[n] = d, src[n] = s, words[n] = bytes / 4;
        ++n;
    }
};
int gu_device_segments(gu_engine *h, const GuSegments &s);
// Small results back to the host through the engine's page-locked landing area (a device-to-host copy into pageable memory is
// staged and waited for by the runtime; into pinned memory it is one DMA): copies `bytes` from `src` on the device to `dst`, behind
// everything queued on the engine's stream, and waits.  Larger than the area: the plain copy.
#define GU_CTL_WORDS (8 + 4096 + 20480)  /* ... and the tables of grids of up to 4096 states (v + pi: 40 bytes per state) in one go */
#define GU_UP_BYTES (40 * 4096)         /* page-locked staging of small uploads (gu_vi_set) */
int gu_read_back(gu_engine *h, void *dst, const void *src, size_t bytes);

// ---- tabular DP launchers (gu_vi.hip) --------------------------------------------
int gu_vi_alloc(gu_engine *h);
void gu_vi_free(gu_engine *h);
int gu_launch_greedy_table(gu_engine *h);

// ---- config 5 synchronised per XCD (gu_vi_xcd.hip) --------------------------------
struct GuXcdPlan {
    int block = 0, K = 0, NB = 1;  // threads per workgroup, states per thread at most, 16-byte exchange loads per thread (1 or 4)
    unsigned G = 0;            // workgroups
    uint32_t values = 0;       // doubles of a workgroup's value window in LDS
    size_t lds = 0, slots_bytes = 0, work_bytes = 0;  // dynamic LDS; the launches' own buffers: delta-key slots (all XCCs), granule buffers (per XCC)
};
#define GU_VI_FALLBACK 1  /* internal: a one-launch DP form did not apply or gave up, the tables are as they were -- take the next form */
bool gu_vi_xcd_plan(const gu_engine *h, bool agents, GuXcdPlan *plan);
void gu_vi_xcd_free(gu_engine *h);
int gu_vi_xcd_fused_run(gu_engine *h, const GuXcdPlan &xp, double gamma, int32_t iters, uint32_t flags, double *deltas);
int gu_vi_xcd_dp_run(gu_engine *h, double gamma, double threshold, bool use_threshold, bool greedy, int32_t max_rounds, int32_t *rounds_done,
                     double *deltas);

// ---- the batched learners ------------------------------------------------------------
// gu_td.hip (Q-learning, SARSA, Expected SARSA), gu_double.hip (Double Q-learning), gu_dyna.hip (Dyna-Q), gu_sweep.hip (prioritized
// sweeping), gu_nstep.hip, gu_lambda.hip, gu_search.hip (rollout search), gu_explore.hip (UCB / Thompson), gu_mcts.hip (tree search),
// gu_is.hip (off-policy Monte-Carlo), gu_ac.hip (actor-critic), gu_reinforce.hip and gu_fa.hip (semi-gradient learners on features)
// each hold their kernels, their launch code and their extern "C" functions (include/gu.h); the host helpers they share are in
// gu_tabular.hpp.  What they export to each other is their gu_*_free: the device buffers of the module and the fields that describe
// them, back to "none", and the carry slot with them when the module owns it.
void gu_dyna_free(gu_engine *h);        // (takes gu_sweep.hip's queues along)
int gu_sweep_clear(gu_engine *h);       // gu_sweep.hip: empty queues, queued on the stream (gu_dyna_init clears them with the model)
void gu_nstep_free(gu_engine *h);
void gu_lambda_free(gu_engine *h);
void gu_search_free(gu_engine *h);
void gu_explore_free(gu_engine *h);    // (the visit counts; the U and B tables stay)
void gu_mcts_free(gu_engine *h);       // (the node pools; the U, B and I tables stay)
void gu_double_free(gu_engine *h);
void gu_is_free(gu_engine *h);
void gu_ac_free(gu_engine *h);         // (takes gu_reinforce_free along: REINFORCE learns into the actor-critic tables)
void gu_reinforce_free(gu_engine *h);
void gu_fa_free(gu_engine *h);
// The one place that knows every learner's stores (gu_td.hip).  S > 0: a grid of S states is being installed -- Q tables of another
// state count go and take what hangs on them along (the SARSA actions, the n-step and lambda windows, the search scores, the node
// pools), and so does every other store sized by another state count.  S == 0: the engine is being destroyed -- everything goes.
void gu_learners_drop(gu_engine *h, int32_t S);
// Whether a store is there for the grid (and, for the Q tables of gu_td_run, the mask bits) the engine has now.  The GU_NEED_* guard
// of each module and the store's word of gu_get_stores (gu_api.hip) both ask these, so a caller that reads the word knows what the
// guard will say.
#define GU_TD_ROWS(h) ((int64_t)(h)->S << (h)->overlay_bits)  /* gu_td_run's rows: S << F under fruit, S << D under doors (64 bits: F runs to 32; gu_td_init keeps it below 2^31) */
#define GU_HAS_TD_Q(h) ((h)->d_q && (int64_t)(h)->td_S == GU_TD_ROWS(h))
#define GU_HAS_Q(h) ((h)->d_q && (h)->td_S == (h)->S)
#define GU_HAS_PAIRS(h) ((h)->d_dq && (h)->dq_S == (h)->S)
#define GU_HAS_DYNA(h) ((h)->d_dyna_model && (h)->dyna_S == (h)->S)
#define GU_HAS_SWEEP(h) ((h)->d_sweep_heap && GU_HAS_DYNA(h))
#define GU_HAS_COUNTS(h) ((h)->d_explore_n && (h)->explore_S == (h)->S)
#define GU_HAS_EXPLORE_TABLES(h) ((h)->d_explore_tab && (h)->explore_C >= 2)
#define GU_HAS_POOLS(h) ((h)->d_mcts_pool && (h)->mcts_P >= 2)
#define GU_HAS_MCTS_TABLES(h) ((h)->d_mcts_tab && (h)->mcts_C >= 2)
#define GU_HAS_AC(h) ((h)->d_ac_h && (h)->ac_S == (h)->S)
#define GU_HAS_WEIGHTS(h) ((h)->d_is_c && (h)->is_S == (h)->S)
#define GU_HAS_FA(h) ((h)->d_fa_w && (h)->fa_S == (h)->S)

// ---- what the engine carries between calls (DESIGN.md "What the engine carries between calls") ----
// Every call that touches the envs or a learner's tables ends what the learners carry from one launch to the next: gu_td_run's and
// gu_fa_run's SARSA actions, gu_nstep_run's window (its pending updates are discarded, not flushed), gu_lambda_run's window and the
// episode buffers of gu_reinforce_run and gu_is_run (their pending transitions are discarded, not learned from).  Only
// gu_tabular_after (gu_tabular.hpp) installs a carry.
static inline void gu_tabular_drop_carry(gu_engine *h) { h->carry = {}; }
static inline bool gu_carry_is(const gu_engine *h, int owner, int32_t key) { return h->carry.owner == owner && h->carry.key == key; }
// the key `owner` left if it owns the slot, else 0: its window or buffer was dropped and reads as empty
static inline int32_t gu_carry_key(const gu_engine *h, int owner) { return h->carry.owner == owner ? h->carry.key : 0; }
// a learner's gu_*_free: the slot goes with the stores only when they are what it points at
static inline void gu_carry_release(gu_engine *h, int owner)
{
    if (h->carry.owner == owner) h->carry = {};
}

// The envs were touched: `steps` lock-step steps were launched (0: a reset, an installed state, seed, grid or overlay).  Whatever the
// learners carried is gone, and only a rollout vouches for the state the entry table assumes (gu_launch_rollout says so behind this).
static inline void gu_envs_touched(gu_engine *h, uint64_t steps = 0)
{
    h->steps_taken += steps;
    gu_tabular_drop_carry(h);
    h->entry_table_ok = false;
}

// a captured step graph holds the seed, the arrays and the launches of the moment it was captured: whoever changes one of them drops it
static inline void gu_graph_drop(gu_engine *h)
{
    if (h->graph_exec) (void)hipGraphExecDestroy(h->graph_exec);
    h->graph_exec = nullptr;
}

// ---- overlays (gu_overlay.hip: the slot, its install path, getters, reset and launches; gu_overlay.hpp: what its kernels share) ----
struct RolloutArgs;
struct GuRolloutPlan;
struct OverlayStepArgs;
struct OverlayRolloutArgs;
struct TabArgs;
struct OverlayLaneArgs;
// GU_ERR_UNSUPPORTED unless the engine can take an overlay of `kind`: one grid, no trail, no overlay of another kind
int gu_overlay_admits(gu_engine *h, int kind);
// Puts `kind` into the slot: `plane` [S] is the feature's plane, validated by its entry point, `bits` the mask bits in use (0: no
// masks), `param` the kernels' parameter word, `init` the value every mask has now and after every reset, `param2` the second parameter word (errands).
// plane == nullptr takes the overlay away.  A refused call leaves the engine as it was.
int gu_overlay_install(gu_engine *h, int kind, const uint8_t *plane, int32_t bits, uint32_t param, uint32_t init = 0u, uint32_t param2 = 0u);
void gu_overlay_free(gu_engine *h);
int gu_overlay_grid_flags(gu_engine *h, std::vector<uint8_t> &flags);  // [S] the grid's flags plane, read back for a plane's validation
// fruit's and errands' plane format; at most `cap` fruits, counted into *n_fruit and, where of_kind is given, per kind into of_kind[4]
int gu_overlay_fruit_plane(gu_engine *h, int kind, const uint8_t *plane, int32_t cap, int32_t *n_fruit, int32_t *of_kind = nullptr);
int gu_overlay_get_plane(gu_engine *h, int kind, uint8_t *plane);  // [S]; zeros while `kind` is not set
int gu_overlay_get_masks(gu_engine *h, int kind, int64_t env0, int64_t n, uint32_t *masks, const char *what);
int gu_overlay_set_masks(gu_engine *h, int kind, int64_t env0, int64_t n, const uint32_t *masks, const char *what);
int gu_overlay_before_reset(gu_engine *h, const uint8_t *d_mask, bool only_done);  // sets the masks of the envs a reset is about to take to overlay_init; no-op without masks
// the launches that gu_launch_step / gu_launch_rollout hand over while an overlay is set
int gu_overlay_launch_step(gu_engine *h, const int32_t *d_actions_row, uint32_t flags, int32_t *host_obs, int32_t *host_reward, int32_t *host_done,
                           uint32_t *host_seq, uint32_t seq, uint32_t *host_err);
void gu_overlay_launch_rollout(gu_engine *h, const GuRolloutPlan &p, const RolloutArgs &r);  // (the launch alone: gu_launch_rollout checks and completes it)
void gu_overlay_lane_args(gu_engine *h, TabArgs &a, OverlayLaneArgs &o);  // (the overlay's part of gu_launch_td's arguments: gu_tabular.hpp)
// ... and what each feature keeps of them: the launch of its kernel's instantiation for the launch's shape (gu_wind.hip: its own ladder; gu_fruit.hip,
// gu_doors.hip, gu_boxes.hip, gu_errands.hip: one line each, gu_overlay.hpp's ladder around the kind's rule struct, so each kind compiles in its own object)
void gu_wind_step(gu_engine *h, bool lds, const OverlayStepArgs &a);
void gu_fruit_step(gu_engine *h, bool lds, const OverlayStepArgs &a);
void gu_doors_step(gu_engine *h, bool lds, const OverlayStepArgs &a);
void gu_boxes_step(gu_engine *h, bool lds, const OverlayStepArgs &a);
void gu_errands_step(gu_engine *h, bool lds, const OverlayStepArgs &a);
void gu_wind_rollout(gu_engine *h, const GuRolloutPlan &p, const OverlayRolloutArgs &a);
void gu_fruit_rollout(gu_engine *h, const GuRolloutPlan &p, const OverlayRolloutArgs &a);
void gu_doors_rollout(gu_engine *h, const GuRolloutPlan &p, const OverlayRolloutArgs &a);
void gu_boxes_rollout(gu_engine *h, const GuRolloutPlan &p, const OverlayRolloutArgs &a);
void gu_errands_rollout(gu_engine *h, const GuRolloutPlan &p, const OverlayRolloutArgs &a);
// errands: the reset of the words (eaten and progress cleared, the instruction drawn on stream 11 at the episode count BEFORE gu_reset_kernel increments it)
int gu_errands_before_reset(gu_engine *h, const uint8_t *d_mask, bool only_done);
// gu_td.hip: the mask bits in use become `bits` (0: none) -- Q tables whose row count is not S << bits go, with what hangs on them
void gu_td_rows_changed(gu_engine *h, int32_t bits);

// ---- agent trail (gu_trail.hip): no-ops while the trail is off ----------------------
int gu_trail_after_step(gu_engine *h, uint32_t flags);
int gu_trail_before_reset(gu_engine *h, const uint8_t *d_mask, bool only_done);
int gu_trail_after_rollout(gu_engine *h, int64_t T, int traj, bool auto_reset);
int gu_trail_after_set_state(gu_engine *h, bool moved, bool done_given);
void gu_trail_free(gu_engine *h);

// ---- grids (gu_api.hip / gu_maze.hip) ----------------------------------------------
int gu_install_grids(gu_engine *h, int32_t n_grids, int32_t W, int32_t H, const std::vector<uint8_t> &cell,
                     const std::vector<uint8_t> &raw, const std::vector<uint8_t> &kind, const std::vector<int32_t> &starts,
                     const std::vector<int32_t> &n_starts, int32_t max_starts);

// ---- RCCL (gu_comm.hip) ----------------------------------------------------------
void gu_comm_free(gu_engine *h);
