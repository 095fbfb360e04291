/* gu.h -- C ABI of libgu.so, the MI355X (gfx950) GridUniverse step/reset engine.
 *
 * The reference (TheMTank/GridUniverse) is pure Python and has no FFI layer; its
 * boundary for this path is the old-gym Env API of
 * core/envs/griduniverse_env.py:14-321.  Every entry point below names the
 * reference interface (file:line, `env:` = core/envs/griduniverse_env.py) whose
 * per-instance work it replaces for a whole batch of env instances.  The
 * reference-side binding (ctypes) is shown in INTEGRATION.md.
 *
 * Conventions
 *   - plain C, no C++/torch types; every function returns 0 (GU_OK) or a negative
 *     GU_ERR_* code and never throws; gu_last_error() gives the message of the last
 *     failure on the calling thread.
 *   - the caller owns every host buffer (C-contiguous, int32 unless noted);
 *     the library owns all device memory and frees it in gu_destroy().
 *   - a handle is bound to ONE device and ONE HIP stream and is not thread-safe;
 *     different handles may be driven from different threads / processes.
 *   - calls that take host buffers are synchronous; calls documented "async" only
 *     enqueue work on the handle's stream (gu_sync() waits for it).
 *   - env state is struct-of-arrays in HBM: pos[N] | reward[N] | done[N] (one
 *     contiguous int32[3N] block, so the gathered view is one collective),
 *     episode[N] (uint32), a 64-bit step count per env.  Actions are 0..3 =
 *     UP,RIGHT,DOWN,LEFT (env:56); -4..-1 are the same list addressed from its end, as
 *     in the reference (env:148: -1 is LEFT); anything else is
 *     rejected (the reference raises IndexError).  Caller-supplied actions and
 *     states are validated by the kernels that consume them (an error word in
 *     page-locked memory), not by host loops.
 */
#ifndef GU_H
#define GU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GU_ABI_VERSION 1

#define GU_OK 0
#define GU_ERR_INVALID (-1)     /* bad argument (NULL, out of range, wrong size)        */
#define GU_ERR_HIP (-2)         /* a HIP runtime call failed (no device, launch error)   */
#define GU_ERR_NOMEM (-3)       /* host or device allocation failed                      */
#define GU_ERR_STATE (-4)       /* call order: no grid set, no trajectory reserved, ...  */
#define GU_ERR_COMM (-5)        /* RCCL failure                                          */
#define GU_ERR_UNSUPPORTED (-6) /* grid too large for this build, etc.                   */

/* gu_rollout / gu_step_device flags */
#define GU_F_AUTO_RESET 1u  /* harness `if done: env.reset()` applied before the next step */
#define GU_F_TRAJECTORY 2u  /* write (obs,reward,done)[t][env] for every step              */
#define GU_F_STATS 4u       /* per-env sum of rewards and finished-episode count           */
#define GU_F_PACKED 16u     /* gu_rollout: write ONE packed uint32 per env-step instead of three int32 rows:
                               obs | (reward & 0xFF) << 16 | done << 24  (4 B per env-step; grids <= 65 536 cells);
                               read back with gu_read_trajectory_packed.  Excludes GU_F_TRAJECTORY. */
#define GU_F_PINNED_IO 8u   /* gu_step: the caller's buffers are page-locked (gu_host_alloc): the kernel reads and
                               writes them itself instead of going through the library's staging block */

/* gu_rollout policy kinds */
#define GU_POLICY_UNIFORM 0 /* a ~ U{0..3} from the per-env counter RNG (stream 0)           */
#define GU_POLICY_STREAM 1  /* a = actions[t][env] uploaded with gu_upload_actions           */
#define GU_POLICY_GREEDY 2  /* a = first argmax of pi[pos] (np.argmax; examples/griduniverse_alg_examples.py:76) */
#define GU_POLICY_SAMPLE 3  /* a ~ pi[pos]: inverse CDF on one 32-bit word of RNG stream 2 per step, the batched form of
                               np.random.choice(4, p=policy[obs]) in core/algorithms/monte_carlo.py:20.  The stream is the
                               build's own (oracle/gu_rng.py is its specification): one MurmurHash3 word per sixteen steps
                               of an env, the fifteen behind it by xorshift32 + a Weyl increment -- sampled sequences
                               differ from those of libraries built before ABI round 4, their distribution does not */

typedef struct gu_engine *gu_handle;

/* ---- library ----------------------------------------------------------------- */
int gu_version(void);                         /* GU_ABI_VERSION */
int gu_last_error(char *buf, size_t len);     /* copies the thread's last message, returns its length */
int gu_device_count(int *count);              /* hipGetDeviceCount */
int gu_source_hash(char *buf, size_t len);    /* 16 hex digits identifying the sources the library was built from
                                                 (sha256 over every .hip / .hpp under csrc and include/gu.h); returns the length */
/* "key=value;..." description of device `device_id` (name, arch, pci bus id, cus, lds_per_cu, sclk_khz, mclk_khz,
 * bus_bits, l2_bytes, hbm_bytes, hbm_free): what bench.py prints next to its numbers.  Returns the length. */
int gu_device_info(int device_id, char *buf, size_t len);

/* ---- options -------------------------------------------------------------------
 * Launch-shape and search parameters, per engine (h) or -- h == NULL -- as the process default every engine without a value
 * of its own uses.  GU_OPT_UNSET as value returns an option to the built-in default.  RESULTS NEVER DEPEND ON THEM (the
 * tests run every kernel path against the oracle by flipping them); they exist for tests and measurements.  The library
 * reads only two environment variables: GU_RCCL_LIB (which librccl to dlopen) and GU_DEBUG (reports on stderr).
 * Options 100+ select known-unsafe experiments and are refused (GU_ERR_UNSUPPORTED) unless the library was built with
 * -DGU_EXPERIMENTS (make exp -> libgu_exp.so, used by tools/ only). */
#define GU_OPT_UNSET INT64_MIN
#define GU_OPT_ROLLOUT_BLOCK 1        /* workgroup size of the general rollout kernel: 64 .. 1024 (256)                         */
#define GU_OPT_ROLLOUT_ROWS 2         /* transition-row kernel: 0 never, 1 wherever eligible, 2 = 1 without its pair tables
                                         (default: by launch shape)                                                           */
#define GU_OPT_ROWS_COPIES 3          /* copies of its table across the LDS banks: 1, 2, .. 32 (default: by policy)           */
#define GU_OPT_ROLLOUT_MULTI 4        /* K-step kernel: 0 never, 1 whenever the table fits (default: launches of >= 64 steps)  */
#define GU_OPT_ROLLOUT_MULTI_K 5      /* force K = 2 or 4                                                                     */
#define GU_OPT_ROLLOUT_MULTI_COPIES 6 /* 2 = replicate its table across the banks                                             */
#define GU_OPT_ROLLOUT_XCD 7          /* 1 = XCD-aware env-block order (measured slower; off)                                 */
#define GU_OPT_VI_PATH 8              /* DP: 1 = no workgroup-cluster kernel, 2 = one launch per round on every grid size,
                                         3 = chip-wide cluster kernel with an INJECTED grid-barrier timeout (tests of the
                                         fallback), 4 = no per-XCD form of gu_vi_sweep_step_run (the chip-wide cluster kernel
                                         instead), 5 = its per-XCD form gives up at once (INJECTED; tests of the fallback),
                                         6 = the per-XCD form of gu_vi_sweep_step_run for calls of ONE round too (by default
                                         those take the single fused launch, which starts ~10 us quicker; tests, measurements) */
#define GU_OPT_MC_SCRATCH_MB 9        /* scratch budget of gu_mc_evaluate (2048)                                              */
#define GU_OPT_MC_LANE_RETURNS 10     /* 1 = return sums by the per-lane kernel instead of the LDS-tiled one                  */
#define GU_OPT_MC_GLOBAL_WALK 11      /* 1 = history walk with its counters in global memory instead of LDS                   */
#define GU_OPT_STEP_SYNC 12           /* 1 = gu_step always waits with the stream synchronisation                             */
#define GU_OPT_TRAJ_CANDIDATES 13     /* back-to-back candidates of the trajectory placement search (4; 1 = take the first)   */
#define GU_OPT_TRAJ_FAR_CANDIDATES 14 /* candidates behind spacers (0 = none, the default)                                       */
#define GU_OPT_TRAJ_STRIDE_MIB 15     /* spacer size (3072)                                                                   */
#define GU_OPT_TRAJ_FAR_MIB 16        /* most memory the search may hold at once (49152)                                      */
#define GU_OPT_ROLLOUT_PACE 18        /* store pacing of launches that write rows: -1 = closed loop (default, see gu_rollout_pacing),
                                         0 = none, n = fixed period of n 10 ns ticks per 16 steps (-2: accepted, same as -1) */
#define GU_OPT_VI_XCD_BLOCK 19        /* workgroup size of the per-XCD form of gu_vi_sweep_step_run: 256, 512, 1024 (0 = by batch size) */
#define GU_OPT_TRAJ_LAYOUT 24         /* device layout of the int32 trajectory: 0 = three planes [T][N], 1 = one plane of (obs, reward,
                                         done) triples [T][N][3] written with one 12-byte store per lane and step, -1 (default) =
                                         triples where they are faster (small batches under the uniform policy); what
                                         gu_read_trajectory, gu_mc_evaluate and the host see does not change                   */
#define GU_OPT_ROLLOUT_HALF_WAVES 28   /* transition-row kernel, launches that write rows: 32 envs per wave and twice the waves; -1 = where
                                         measured faster (triples + pair tables at 8192 .. 16 384 envs; default), 0 never, 1 always   */
#define GU_OPT_ROLLOUT_ENTRY 29        /* transition-row kernel: 1 (default) = a launch that follows another rollout of the same engine takes
                                         its FIRST step on the staged table too (the state a rollout leaves behind always agrees with its cell);
                                         0 = always on the per-cell planes, as a launch behind gu_reset / gu_set_state / gu_step must       */
#define GU_OPT_SYNC_SPIN_US 30         /* gu_sync / gu_timer_end poll the event for up to this many microseconds (5000) before the runtime's
                                         blocking wait; 0 = blocking at once (ranks or engines that outnumber the host cores)             */
#define GU_OPT_COUNT 31
int gu_set_option(gu_handle h, int32_t option, int64_t value);
int gu_get_option(gu_handle h, int32_t option, int64_t *value);   /* the value in force (own, process default or built-in) */

/* ---- lifetime ----------------------------------------------------------------
 * One engine = `num_envs` lock-stepped instances of one grid on device `device_id`;
 * `env_id0` is the global index of its first env (RNG streams are keyed by global
 * id, so a sharded batch reproduces the single-device batch byte for byte).
 * Replaces num_envs x GridUniverseEnv.__init__ (env:17-107) state setup. */
int gu_create(int device_id, int64_t num_envs, int64_t env_id0, gu_handle *out);
int gu_destroy(gu_handle h);

/* ---- grid --------------------------------------------------------------------
 * Row bit-planes, `words_per_row` = ceil(W/32) uint32 words per row, bit (x & 31) of
 * word (x >> 5) of row y describes cell s = y*W + x (env:116-117).
 *   wall_rows  : wall_grid[s] == 1          (env:120-134, env:157-161)
 *   goal_rows  : s in goal_states           (env:173-174)
 *   lava_rows  : s in lava_states           (env:170-171)
 *   rplus_rows / rminus_rows : reward_matrix[s] == +10 / == -10 (env:80-90, 312-316),
 *       or both NULL to derive them as (lava ? -10 : goal ? +10 : -1).  They are
 *       separate planes because the reference's reward matrix and terminal test
 *       can disagree (negative indices wrap only in the former; quirk 5).
 *   starts     : starting_states (env:61-63), n_starts >= 1.
 * W * H <= 2^30 cells and W <= 8 388 607 columns (GU_ERR_UNSUPPORTED beyond: the move is a 24-bit multiply-add).
 * The library compiles the planes into two bytes per cell -- flags (per action: does the
 * move change the position, incl. the absorbing-terminal rule; terminal bit; reward code;
 * wall bit) and the int8 reward -- which the kernels stage in LDS (gu_get_cells reads
 * them back). */
int gu_set_grid(gu_handle h, int32_t W, int32_t H, int32_t words_per_row,
                const uint32_t *wall_rows, const uint32_t *goal_rows, const uint32_t *lava_rows,
                const uint32_t *rplus_rows, const uint32_t *rminus_rows,
                const int32_t *starts, int32_t n_starts);

/* Several DISTINCT grids of one shape in one engine (SURVEY.md 8(d) C3 variant, 8(f) rank 3): env e uses grid
 * e / (num_envs / n_grids) -- contiguous equal groups, n_grids must divide num_envs.  Planes are
 * [n_grids][H][words_per_row]; starts is [n_grids][max_starts] with n_starts[g] valid entries per grid.
 * The rollout kernels stage one grid per block in LDS when the group size is a multiple of 64, keep a private
 * copy of its grid per lane in LDS otherwise (e.g. one grid per env), and read L2 for grids too large for either.
 * Multi-grid engines do not support the DP / Monte-Carlo tables (one value table per engine). */
int gu_set_grids(gu_handle h, int32_t n_grids, int32_t W, int32_t H, int32_t words_per_row,
                 const uint32_t *wall_rows, const uint32_t *goal_rows, const uint32_t *lava_rows,
                 const uint32_t *rplus_rows, const uint32_t *rminus_rows,
                 const int32_t *starts, const int32_t *n_starts, int32_t max_starts);
/* Generate n_grids random mazes ON THE DEVICE (one lane carves one maze): the algorithm of
 * core/envs/maze_generation.py:41-149 (recursive backtracker, one 'x', one 'G'), draws from RNG stream 3 keyed
 * by (maze_seed, global grid id).  Replaces n_grids x GridUniverseEnv(random_maze=True) (env:318-321). */
int gu_generate_mazes(gu_handle h, int32_t n_grids, int32_t W, int32_t H, uint64_t maze_seed);
/* Read back grid `grid_index` as compiled: flags[S] (OPEN bits 0-3 = move changes the position, bit 4 terminal,
 * bits 5-6 reward code, bit 7 the cell is a wall),
 * reward[S] (int8), and its start table (any pointer may be NULL). */
int gu_get_cells(gu_handle h, int32_t grid_index, uint8_t *flags, int8_t *reward, int32_t *starts, int32_t *n_starts);

/* ---- wind: per-cell pushes with gusts (Sutton & Barto's windy gridworld, Example 6.5, and its stochastic form, Exercise 6.10) ----
 * Build-defined (the reference has no wind; restated on the CPU by tests/_wind_oracle.py).  Wind is a property of a SINGLE-GRID
 * engine: one byte per cell, wind[s] bits 0..1 the direction (the action codes UP, RIGHT, DOWN, LEFT), bits 2..3 the strength k
 * (0 .. 3), bits 4..7 zero, and an engine-wide gust probability gust_q16 in 0 .. 65536 (gust_q16 = round(gust * 65536); gust = 2/3,
 * 43691, is Exercise 6.10's one third each for k - 1, k and k + 1).
 * One step of env e at 64-bit step count t, from cell s (after the lazy reset, where there is one), with a valid action a:
 *   1. c = wind[s], the wind of the cell the agent LEAVES; k = (c >> 2) & 3, dir = c & 3.
 *   2. If k > 0 and gust_q16 > 0: w = the word of RNG stream 9 with counter t & 0xFFFFFFFF and epoch t >> 32 (keyed exactly like
 *      stream 4); if (w >> 16) < gust_q16 then k += (w & 1) ? +1 : -1.  So k ends in 0 .. 4.
 *   3. s1 = move(s, a); then k times s1 = move(s1, dir).
 *   4. move is the engine's rule as it stands: the OPEN bit of the cell's flags, with the absorbing terminal.  A wall or the border
 *      stops a push, and an agent blown ONTO a goal or lava cell stays there (its OPEN bits are zero).
 *   5. reward and done come from the final cell; then t += 1.
 * An action that gu_step rejects moves nothing and draws nothing; a launch with gust_q16 == 0 hashes no word; wind of strength 0
 * everywhere gives the bytes of the calm engine.  This differs from Sutton & Barto's vector-sum rule in one point -- an agent
 * cannot be blown ACROSS a terminal cell: on the book's 10 x 7 grid (column strengths 0 0 0 1 1 1 2 2 1 0 upward, start (0, 3), goal
 * (7, 3)) the shortest path has 10 moves (15 under the book's rule) and 62 of the 70 cells can be reached.
 * While wind is set, gu_step, gu_step_device, gu_rollout (all four policies; GU_F_PACKED is refused) and gu_td_run (both methods)
 * run their windy kernels (csrc/gu_wind.hip, csrc/gu_td.hip); every other call that moves envs or reads the move rule --
 * gu_step_graph, the other learners' gu_*_run, gu_look_step_ahead, gu_vi_sweep / _run / _eval_run / _greedy / _sweep_step /
 * _sweep_step_run, gu_mc_walk_lengths / _episodes, gu_shortest_paths -- returns GU_ERR_UNSUPPORTED.  Calls that read rows or state
 * only (gu_vi_set / _get, gu_mc_evaluate, sense, render, state, reset, seed, the tables' getters and setters) are unaffected.
 * gu_set_wind: wind[S], or NULL = calm again (the calm kernels run as before).  GU_ERR_STATE without a grid; GU_ERR_UNSUPPORTED on a
 *              multi-grid engine and while the agent trail is on (gu_trail_enable refuses while wind is set); GU_ERR_INVALID for a
 *              byte with bits 4..7 set or gust_q16 > 65536.  Ends what the learners carry from launch to launch (SARSA actions,
 *              windows, episode buffers); keeps tables, env state and step counts.  gu_set_grid, gu_set_grids and
 *              gu_generate_mazes drop the wind.
 * gu_get_wind: the plane (zeros when calm), the gust probability and whether wind is set; any pointer may be NULL. */
int gu_set_wind(gu_handle h, const uint8_t *wind /* [S], NULL = calm again */, uint32_t gust_q16);
int gu_get_wind(gu_handle h, uint8_t *wind /* [S], may be NULL */, uint32_t *gust_q16, int32_t *present);

/* ---- fruit: collectable rewards, each eaten once per episode ------------------------------------------------
 * Build-defined (the reference has no fruit; restated on the CPU by tests/_fruit_oracle.py).  Fruit is a property of a SINGLE-GRID
 * engine.  It consists of one byte per cell, fruit[s] -- bits 0..4 the slot (0 .. 31), bits 5..6 the kind (0 = no fruit, 1 / 2 / 3 =
 * the three kinds; the Python names are apple, lemon, melon), bit 7 zero, and kind 0 requires the whole byte to be 0 --, three
 * engine-wide values value[3], one per kind, each in -16 .. +16, and one uint32 eaten[e] per env.  F is the number of fruit cells,
 * 1 .. 32; their slots are exactly 0 .. F-1, each used once.  A fruit may not lie on a wall or on a goal or lava cell; it may lie on a
 * start cell.
 * One step of env e from cell s with a valid action:
 *   1. the lazy auto-reset, where the call has one, sets eaten[e] = 0 together with the position;
 *   2. s', r, d come from the engine's move rule exactly as without fruit: fruit never changes a move and never ends an episode;
 *   3. c = fruit[s'].  If (c >> 5) & 3 != 0 and bit c & 31 of eaten[e] is clear, then r += value[kind - 1] and that bit is set;
 *   4. t += 1.
 * So a reset does not eat the fruit of the start cell; a later step that ends there does, and so does a wall bump that leaves the
 * agent on it.  A rejected action (outside -4 .. 3) eats nothing.  No RNG stream is added and none is drawn differently: the obs and
 * done rows of gu_step and of a rollout (any policy) are byte for byte those of the engine without fruit, and the reward rows differ
 * by value[kind - 1] exactly at each fruit's first visit of an episode.
 * The bound on the values keeps a launch's int32 reward sum in range at the existing T <= 1e8: a step ends on one cell, so it eats
 * at most one fruit; a fruit is eaten at most once per episode and cannot lie on a terminal cell, so the step that eats it pays
 * the cell's -1 beside the value (|r| <= 17), and an episode that eats k fruits has at least k + 1 steps, the last one a terminal step
 * of |r| <= 10.  No step pays more than 17 in absolute value, and 1e8 * 17 < 2^31.  (Reward planes that put +-10 on a cell that is not
 * terminal can take such a step to 26; 8.2e7 steps are safe for those.)
 * Every path that resets an env clears its mask: gu_reset (masked envs only), gu_reset_done, and the lazy resets inside the kernels.
 * gu_set_fruit clears the masks of all envs; gu_set_state and gu_seed leave them alone.
 * While fruit is set, gu_step (pinned I/O and the completion word included), gu_step_device, gu_rollout (all four policies,
 * GU_F_TRAJECTORY / GU_F_STATS; GU_F_PACKED returns GU_ERR_UNSUPPORTED; rows are the three [T][N] planes, never triples) and gu_td_run
 * (both methods) run their fruit kernels (csrc/gu_fruit.hip, csrc/gu_td.hip); every other call that moves envs or reads the move or
 * reward rule -- gu_step_graph, the other learners' gu_*_run, gu_look_step_ahead, gu_vi_sweep / _run / _eval_run / _greedy /
 * _sweep_step / _sweep_step_run, gu_mc_walk_lengths / _episodes, gu_shortest_paths -- returns GU_ERR_UNSUPPORTED.  Calls that read
 * rows or state only (gu_mc_evaluate, sense, render, the getters, gu_read_*) are unaffected; they do not show fruit.
 * THE LEARNERS' TABLES: a problem with fruit is Markov only on (cell, eaten), so while fruit is set a gu_td_run table has S << F
 * rows and row eaten * S + s belongs to cell s with mask eaten.  Rules 1-4 of gu_td_run hold with "row of s" read as "row of
 * (s, eaten)": the action is drawn on the row of (s, eaten), the bootstrap uses the pre-update row of (s', eaten'), the update goes to
 * the row of (s, eaten); the arithmetic, the tie rule, the SARSA carry and the stream-4 words are as they are.  gu_td_init under
 * fruit returns GU_ERR_INVALID for F > 10, else allocates N * (S << F) * 32 bytes under its free-memory rule; gu_td_get_q / gu_td_set_q
 * move q[n][S << F][4].  No other learner ever sees such a table: they are refused while fruit is set.
 * gu_set_fruit: fruit[S] and value[3], or fruit = NULL = no fruit again (the kernels without fruit run as before).  GU_ERR_STATE without
 *              a grid; GU_ERR_UNSUPPORTED on a multi-grid engine, while wind is set (gu_set_wind refuses while fruit is set) and
 *              while the agent trail is on (gu_trail_enable refuses while fruit is set); GU_ERR_INVALID for a malformed byte, a
 *              repeated or missing slot, more than 32 fruits, a fruit on a wall or terminal cell, or a value outside -16 .. 16.
 *              Ends what the learners carry from launch to launch, destroys a captured step graph, and drops the Q tables (as a grid
 *              of another size does: gu_td_run returns GU_ERR_STATE until gu_td_init) whenever it changes their row count -- it keeps
 *              them when the row count stays; clearing fruit goes back to S rows the same way.  Keeps positions and step counts.
 *              gu_set_grid, gu_set_grids and gu_generate_mazes drop the fruit.
 * gu_get_fruit: the plane (zeros when none), the values and F (0 = none set); any pointer may be NULL.
 * gu_get_fruit_state / gu_set_fruit_state: the masks of envs env0 .. env0+n-1; GU_ERR_STATE while no fruit is set; setting a bit at or
 *              above F is GU_ERR_INVALID.  Setting masks ends the learners' carries (a carried SARSA action belongs to the old row). */
int gu_set_fruit(gu_handle h, const uint8_t *fruit /* [S], NULL = no fruit again */, const int32_t value[3]);
int gu_get_fruit(gu_handle h, uint8_t *fruit /* zeros when none */, int32_t value[3], int32_t *n_fruit /* 0 = none set */);
int gu_get_fruit_state(gu_handle h, int64_t env0, int64_t n, uint32_t *eaten);
int gu_set_fruit_state(gu_handle h, int64_t env0, int64_t n, const uint32_t *eaten);  /* a bit at or above F: GU_ERR_INVALID */

/* ---- doors, keys and levers: walls that an env opens for itself ----------------------------------------------
 * Build-defined (the reference has no doors; restated on the CPU by tests/_doors_oracle.py).  Doors are a property of a SINGLE-GRID
 * engine.  They consist of one byte per cell, door[s] -- bits 0..2 the slot (0 .. 7), bits 4..5 the kind (0 = nothing, 1 = door,
 * 2 = key, 3 = lever), bits 3, 6 and 7 zero, and kind 0 requires the whole byte to be 0 --, and one uint32 open[e] per env: bit k set
 * means the doors of slot k are open for env e.  D is the number of slots in use, 1 .. 8; the slots in use are exactly 0 .. D-1, and
 * every one of them has at least one door cell and at least one key or lever cell.  Several cells may share a slot (one key can open
 * two doors).  None of the three kinds may lie on a wall or on a goal or lava cell; they may lie on start cells.
 * One step of env e from cell s with a valid action a:
 *   1. the lazy auto-reset, where the call has one, sets open[e] = 0 together with the position: doors are shut again, keys are back;
 *   2. c is the candidate cell, from the engine's move rule exactly as without doors (door, key and lever cells are free cells for it);
 *   3. if door[c] is a door of slot k and bit k of open[e] is clear, the move is refused as a wall refuses it: s' = s; else s' = c.
 *      A closed door refuses ENTRY only: an agent standing on a door cell (at a start, or after gu_set_state) leaves it like any cell;
 *   4. r and d are the engine's for s': a bump on a closed door pays what a wall bump from s pays;
 *   5. if s' != s and door[s'] is a key of slot k, then open[e] |= 1 << k; if it is a lever of slot k, then open[e] ^= 1 << k.
 *      Standing still on a lever (wall bump, door bump) does not pull it again, and a reset onto a key or lever cell does not touch
 *      the mask;
 *   6. t += 1.
 * A rejected action (outside -4 .. 3) moves nothing and changes no mask.  No RNG stream is added and none is drawn differently.
 * Every path that resets an env clears its mask: gu_reset (masked envs only), gu_reset_done, and the lazy resets inside the kernels.
 * gu_set_doors clears the masks of all envs; gu_set_state and gu_seed leave them alone.
 * While doors are set, gu_step (pinned I/O and the completion word included), gu_step_device, gu_rollout (all four policies,
 * GU_F_TRAJECTORY / GU_F_STATS; GU_F_PACKED returns GU_ERR_UNSUPPORTED; rows are the three [T][N] planes, never triples) and gu_td_run
 * (both methods) run their door kernels (csrc/gu_doors.hip, csrc/gu_td.hip); every other call that moves envs or reads the move
 * rule -- gu_step_graph, the other learners' gu_*_run, gu_look_step_ahead, gu_vi_sweep / _run / _eval_run / _greedy / _sweep_step /
 * _sweep_step_run, gu_mc_walk_lengths / _episodes, gu_shortest_paths -- returns GU_ERR_UNSUPPORTED.  Calls that read rows or state only
 * (gu_mc_evaluate, sense, render, the getters, gu_read_*) are unaffected; they show door, key and lever cells as free cells.
 * THE LEARNERS' TABLES: a problem with doors is Markov only on (cell, open), so while doors are set a gu_td_run table has S << D rows
 * and row open * S + s belongs to cell s under the mask open.  Rules 1-4 of gu_td_run hold with "row of s" read as "row of (s, open)":
 * the action is drawn on the row of (s, open), the bootstrap uses the pre-update row of (s', open'), the update goes to the row of
 * (s, open); the arithmetic, the tie rule, the SARSA carry and the stream-4 words are as they are.  gu_td_init under doors allocates
 * N * (S << D) * 32 bytes under its free-memory rule (and its bound of 2^31 - 1 rows); gu_td_get_q / gu_td_set_q move q[n][S << D][4].
 * No other learner ever sees such a table: they are refused while doors are set.
 * gu_set_doors: door[S], or NULL = no doors again (the kernels without doors run as before).  GU_ERR_STATE without a grid;
 *              GU_ERR_UNSUPPORTED on a multi-grid engine, while wind or fruit is set (gu_set_wind and gu_set_fruit refuse while doors
 *              are set) and while the agent trail is on (gu_trail_enable refuses while doors are set); GU_ERR_INVALID for a malformed
 *              byte (a set bit 3 is a ninth slot), a missing slot, a slot without a door, a slot without a key or lever, or a door,
 *              key or lever on a wall or terminal cell.  A refused call leaves the engine as it was.  Ends what the learners carry
 *              from launch to launch, destroys a captured step graph, and drops the Q tables (gu_td_run returns GU_ERR_STATE until
 *              gu_td_init) whenever it changes their row count -- it keeps them when the row count stays; clearing the doors goes
 *              back to S rows the same way.  Keeps positions and step counts.  gu_set_grid, gu_set_grids and gu_generate_mazes drop
 *              the doors.
 * gu_get_doors: the plane (zeros when none) and D (0 = none set); either pointer may be NULL.
 * gu_get_doors_state / gu_set_doors_state: the masks of envs env0 .. env0+n-1; GU_ERR_STATE while no doors are set; setting a bit at
 *              or above D is GU_ERR_INVALID.  Setting masks ends the learners' carries (a carried SARSA action belongs to the old row). */
int gu_set_doors(gu_handle h, const uint8_t *door /* [S], NULL = no doors again */);
int gu_get_doors(gu_handle h, uint8_t *door /* zeros when none */, int32_t *n_slots /* 0 = none set */);
int gu_get_doors_state(gu_handle h, int64_t env0, int64_t n, uint32_t *open);
int gu_set_doors_state(gu_handle h, int64_t env0, int64_t n, const uint32_t *open);  /* a bit at or above D: GU_ERR_INVALID */

/* ---- boxes: Sokoban -- cells that refuse entry, and move ---------------------------------------------------------
 * Build-defined (the reference lists a Sokoban extension and has none; restated on the CPU by tests/_boxes_oracle.py).  Boxes are a
 * property of a SINGLE-GRID engine, and the fourth kind of overlay: they exclude wind, fruit, doors and the agent trail as those
 * exclude each other.  They consist of one byte per cell, box[s] -- bit 0 = the cell is a TARGET, bit 1 = a box stands here at every
 * reset, bits 2..7 zero; a cell may be both --, and one uint32 word per env.  Neither a target nor an initial box may lie on a wall, a
 * goal cell or a lava cell, and an initial box may not lie on a start cell.  B is the number of initial boxes, B >= 1; there must be
 * at least B targets, and at least one initial box must be off target (an env is never born solved).
 * THE WORD: b is the smallest width with S <= 1 << b.  Box k, numbered by ascending initial cell, keeps its identity for the whole
 * episode; its cell sits in bits [k * b, (k + 1) * b) of the env's word.  b * B must be <= 32 (5 boxes at S <= 64, 4 at S <= 256, 3
 * at S <= 1024, 2 up to S = 65536; b * B == 32 is legal).  `init` is the word of the initial boxes.
 * SOLVED means that every box stands on a target cell.
 * One step of env e from cell s under the word w with a valid action a:
 *   1. the lazy auto-reset, where the call has one, sets w = init together with the position: the boxes are back where they began;
 *   2. if w is solved already, nothing moves: s' = s, r = +10, d = 1.  This is absorbing, as a goal cell is, and a property of w, not
 *      of done[];
 *   3. c is the candidate cell, from the engine's move rule exactly as without boxes;
 *   4. if c != s and box k stands on c, then c2 is the engine's move from c with the same action (the OPEN bits of c itself: the
 *      border and walls refuse it).  The push is refused when c2 == c, when c2 is a goal or lava cell, or when another box stands on
 *      c2.  A refused push is a bump: s' = s, w unchanged.  Otherwise box k moves to c2 and s' = c.  Without a box on c, s' = c;
 *   5. a box refuses ENTRY only: an agent that stands on a box cell (after gu_set_state or gu_set_boxes_state) leaves it like any
 *      cell;
 *   6. if w' is solved, then r = +10 and d = 1, in place of everything else.  Otherwise r = R[s'] + v * (target[c2] - target[c]) on a
 *      push and R[s'] without one, and d is the engine's for s'.  v is on_target, 0 .. 16: pushing a box off a target takes back what
 *      pushing it on paid, so no cycle earns reward;
 *   7. t += 1.
 * A rejected action (outside -4 .. 3) moves nothing and changes no word.  No RNG stream is added and none is drawn differently.
 * Every path that resets an env sets its word to init: gu_reset (masked envs only), gu_reset_done, the lazy resets inside the
 * kernels, and gu_set_boxes itself, for every env.  gu_set_state and gu_seed leave the words alone.
 * DEADLOCK: a box that can never reach a target again (in a corner, say) ends no episode.  An auto-resetting env comes back only
 * through a goal or lava cell, so a grid for learners should have one.
 * While boxes are set, gu_step (pinned I/O and the completion word included), gu_step_device, gu_rollout (all four policies,
 * GU_F_TRAJECTORY / GU_F_STATS; GU_F_PACKED returns GU_ERR_UNSUPPORTED; rows are the three [T][N] planes) and gu_td_run (both methods)
 * run their box kernels (csrc/gu_boxes.hip, csrc/gu_td.hip); every call that is refused while doors are set (gu_set_doors above) is
 * refused in the same way, with GU_ERR_UNSUPPORTED.  Calls that read rows or state only are unaffected; sense and render show box and
 * target cells as free cells.
 * THE LEARNERS' TABLES: while boxes are set a gu_td_run table has S << (b * B) rows and row w * S + s belongs to cell s under the word
 * w, exactly as under doors.  gu_td_init takes at most 10 bits (b * B <= 10: one box up to S = 1024, two up to S = 32) and returns
 * GU_ERR_INVALID above.
 * gu_set_boxes: box[S] and on_target, or NULL = no boxes again.  GU_ERR_STATE without a grid; GU_ERR_UNSUPPORTED on a multi-grid
 *              engine, while wind, fruit or doors are set and while the agent trail is on (each of those refuses while boxes are
 *              set); GU_ERR_INVALID for a malformed byte, a box or target on a wall or terminal cell, an initial box on a start cell,
 *              no box, fewer targets than boxes, every box on a target, b * B > 32 or on_target outside 0 .. 16.  A refused call
 *              leaves the engine as it was.  Ends what the learners carry, destroys a captured step graph and drops the Q tables
 *              whenever it changes their row count, as gu_set_doors does.  Keeps positions and step counts.  gu_set_grid,
 *              gu_set_grids and gu_generate_mazes drop the boxes.
 * gu_get_boxes: the plane (zeros when none), on_target, B (0 = none set) and b; every pointer may be NULL.
 * gu_get_boxes_state / gu_set_boxes_state: the words of envs env0 .. env0+n-1; GU_ERR_STATE while no boxes are set; GU_ERR_INVALID for
 *              a word with a bit at or above b * B, a field >= S, two equal fields, or a field on a wall or terminal cell.  Setting
 *              words ends the learners' carries. */
int gu_set_boxes(gu_handle h, const uint8_t *box /* [S], NULL = no boxes again */, int32_t on_target /* 0 .. 16 */);
int gu_get_boxes(gu_handle h, uint8_t *box /* zeros when none */, int32_t *on_target, int32_t *n_boxes /* 0 = none set */, int32_t *bits_per_box);
int gu_get_boxes_state(gu_handle h, int64_t env0, int64_t n, uint32_t *words);
int gu_set_boxes_state(gu_handle h, int64_t env0, int64_t n, const uint32_t *words);

/* ---- errands: ordered fruit-collection instructions, one per episode ------------------------------------------------
 * Build-defined (the reference's roadmap lists natural language grounding -- "collect the lemon and then the apple" -- and a
 * multi-task interface, and has neither; restated on the CPU by tests/_errands_oracle.py).  Errands are a property of a SINGLE-GRID
 * engine, and the fifth kind of overlay: they exclude wind, fruit, doors, boxes and the agent trail as those exclude each other.
 * THE PLANE: one byte per cell, errand[s], in fruit's format exactly -- bits 0..4 the slot, bits 5..6 the kind (0 = no fruit, 1 / 2 / 3
 * = apple, lemon, melon), bit 7 zero, and kind 0 requires the whole byte to be 0.  F is the number of fruit cells, 1 .. 8; their slots
 * are exactly 0 .. F-1, each used once.  A fruit may not lie on a wall or on a goal or lava cell; it may lie on a start cell.
 * THE INSTRUCTIONS: I of them, 1 .. 4, each a list of L_j kinds, 1 <= L_j <= 4.  instr[j] holds instruction j: position p sits in bits
 * 2p .. 2p+1, kind 0 ends the list (nothing may follow it), a list of four has no end mark; instr[j] is zero for j >= I.  An instruction
 * may name a kind at most as often as the plane holds fruit of that kind, so a fresh episode can always carry it out.
 * THE PAY: pay[3] = right in 0 .. 16, wrong in -16 .. 0, finish in 0 .. 16.  A fruit cannot lie on a terminal cell, so the step that
 * eats one pays the cell's -1 beside right or wrong and the completing step pays finish alone: no step pays more than 17 in absolute
 * value, and fruit's bound on a launch's int32 reward sum holds (gu_set_fruit above).
 * THE WORD: one uint32 per env.  Bits [0, F): the fruit eaten (bit = slot).  Bits [F, F + pb): the progress p, pb = bit_length(max L_j).
 * Bits [F + pb, F + pb + ib): the index j of the env's instruction, ib = bit_length(I - 1).  F + pb + ib bits are in use (at most 13).
 * One step of env e from cell s under the word (eaten, p, j) with a valid action:
 *   1. the lazy auto-reset, where the call has one, sets eaten = 0 and p = 0 together with the position and draws j = (w * I) >> 32,
 *      w the word of RNG stream 11, keyed like stream 1 (seed, global env id, no epoch) with the value of episode[e] BEFORE this reset
 *      increments it as its counter.  With I = 1 no word need be hashed;
 *   2. if p == L_j, nothing moves: s' = s, r = finish, d = 1.  This is absorbing, and a property of the word, as "solved" is for boxes;
 *   3. otherwise s' comes from the engine's move rule exactly as without errands: an errand never changes a move;
 *   4. c = errand[s'].  If c holds a fruit whose bit of eaten is clear, the bit is set.  If its kind is entry p of instruction j, then
 *      p += 1; if now p == L_j, then r = finish and d = 1, in place of everything else, and otherwise r = R[s'] + right.  If its kind is
 *      not that entry, then r = R[s'] + wrong and p stays: the fruit is gone, and the instruction may now be impossible -- such an env
 *      comes back through a goal or lava cell only, as under a boxes deadlock;
 *   5. without a fresh fruit, r and d are the engine's for s';
 *   6. t += 1.
 * So a reset does not eat the fruit of the start cell; a later step that ends there does, and so does a wall bump that leaves the
 * agent on it.  A rejected action (outside -4 .. 3) moves nothing, eats nothing and draws nothing.  Streams 0, 1, 2 and 4 are drawn as
 * they are without errands.
 * Every path that resets an env clears eaten and p and draws j by rule 1: gu_reset (masked envs only, with or without start_choice),
 * gu_reset_done, and the lazy resets inside the kernels.  gu_set_errands itself sets every word to 0: instruction 0, nothing eaten.
 * gu_set_state and gu_seed leave the words alone.
 * While errands are set, gu_step (pinned I/O and the completion word included), gu_step_device, gu_rollout (all four policies,
 * GU_F_TRAJECTORY / GU_F_STATS; GU_F_PACKED returns GU_ERR_UNSUPPORTED; rows are the three [T][N] planes) and gu_td_run (both methods)
 * run their errand kernels (csrc/gu_errands.hip, csrc/gu_td.hip); every call that is refused while fruit is set (gu_set_fruit above) is
 * refused in the same way, with GU_ERR_UNSUPPORTED.  Calls that read rows or state only are unaffected; sense and render show fruit
 * cells as free cells.
 * THE LEARNERS' TABLES: the instruction is part of the learner's state.  While errands are set a gu_td_run table has
 * S << (F + pb + ib) rows and row word * S + s belongs to cell s under the word, exactly as under fruit.  gu_td_init takes at most 10
 * bits and returns GU_ERR_INVALID above.  No other learner has an errands form.
 * gu_set_errands: errand[S], n_instr = I, instr[4] and pay[3], or errand = NULL = no errands again.  GU_ERR_STATE without a grid;
 *              GU_ERR_UNSUPPORTED on a multi-grid engine, while wind, fruit, doors or boxes are set and while the agent trail is on
 *              (each of those refuses while errands are set); GU_ERR_INVALID for a malformed byte, a repeated or missing slot, more
 *              than 8 fruits, a fruit on a wall or terminal cell, I outside 1 .. 4, an empty or malformed instruction, a non-zero
 *              byte behind the I instructions, an instruction that names a kind more often than the plane holds it, or pay outside
 *              its ranges.  A refused call leaves the engine as it was.  Ends what the learners carry, destroys a captured step graph
 *              and drops the Q tables whenever it changes their row count, as gu_set_fruit does.  Keeps positions and step counts.
 *              gu_set_grid, gu_set_grids and gu_generate_mazes drop the errands.
 * gu_get_errands: the plane (zeros when none), I (0 = none set), the instruction bytes, the pay and F; every pointer may be NULL.
 * gu_get_errands_state / gu_set_errands_state: the words of envs env0 .. env0+n-1; GU_ERR_STATE while no errands are set;
 *              GU_ERR_INVALID for a word with a bit at or above F + pb + ib, with j >= I or with p > L_j, and the engine stays as it
 *              was.  Setting words ends the learners' carries. */
int gu_set_errands(gu_handle h, const uint8_t *errand /* [S], NULL = no errands again */, int32_t n_instr, const uint8_t instr[4] /* one byte each */, const int32_t pay[3]);
int gu_get_errands(gu_handle h, uint8_t *errand /* zeros when none */, int32_t *n_instr /* 0 = none set */, uint8_t instr[4], int32_t pay[3], int32_t *n_fruit);
int gu_get_errands_state(gu_handle h, int64_t env0, int64_t n, uint32_t *words);
int gu_set_errands_state(gu_handle h, int64_t env0, int64_t n, const uint32_t *words);

/* ---- RNG ---------------------------------------------------------------------
 * Keys the per-env counter RNG (MurmurHash3 of seed, global env id, stream,
 * counter -- 32-bit counters, no stream repeats before 2^32 draws; host view:
 * griduniverse_amd/rng.py, restated for the tests in oracle/gu_rng.py) and zeroes
 * episode[] and tcount[].
 * The reference has no per-env RNG (env:242-244 stores one and never uses it). */
int gu_seed(gu_handle h, uint64_t seed);

/* ---- reset: GridUniverseEnv._reset, env:187-193 --------------------------------
 * mask (N bytes, NULL = all): which envs to reset.  start_choice (N int32 indices
 * into starts[], NULL = draw from RNG stream 1 at the env's episode counter).
 * Sets done = 0, bumps episode[].  obs_out (N, optional) receives pos[]. */
int gu_reset(gu_handle h, const uint8_t *mask, const int32_t *start_choice, int32_t *obs_out);
/* Device-side: reset exactly the envs whose done flag is set (async). */
int gu_reset_done(gu_handle h);

/* ---- step: GridUniverseEnv._step, env:176-185 (+ look_step_ahead env:136-155) ---
 * Synchronous, host buffers: actions in, (obs, reward, done) out (each N int32,
 * outputs optional).  flags: GU_F_AUTO_RESET; GU_F_PINNED_IO when every buffer passed
 * is page-locked (gu_host_alloc): the kernel then reads / writes them directly over
 * PCIe and no copy command is issued (pageable buffers take the same route through the
 * library's own page-locked staging block, plus one memcpy each way).  Batches of up to
 * 8192 envs return as soon as the kernel has published a completion word in page-locked
 * memory -- the results are in place, the stream may still be draining; every later call on
 * the handle is ordered behind it as usual.
 * An action outside -4..3 is detected BY THE KERNEL (env:148 raises IndexError before it touches the
 * instance): that env does not step -- position, reward, done flag, pending lazy reset and step
 * count stay as they were, its outputs repeat its current state -- every env with a valid action
 * steps, and the call returns GU_ERR_INVALID naming the first offender.
 * With GU_F_PINNED_IO every pointer is checked (once per allocation) to be page-locked host memory;
 * pageable memory is GU_ERR_INVALID, not a GPU fault. */
int gu_step(gu_handle h, const int32_t *actions, uint32_t flags,
            int32_t *obs, int32_t *reward, int32_t *done);

/* Device-resident action stream [T][N] for gu_step_device / GU_POLICY_STREAM.  Values are validated on the
 * device after the copy; a stream holding anything outside -4..3 is rejected as a whole (GU_ERR_INVALID).
 * The upload REPLACES the stream: afterwards it holds exactly rows 0 .. T-1 (a rejected upload leaves none).
 * Besides the int32 rows (read by the single-step launches) the device keeps the stream packed to two bits
 * per action, 16 steps per word and env; gu_rollout(GU_POLICY_STREAM) reads that: 0.25 B, not 4 B, per env-step. */
int gu_upload_actions(gu_handle h, const int32_t *actions, int64_t T);
/* One step with actions row `t` of the uploaded stream; results stay in HBM (async). */
int gu_step_device(gu_handle h, int64_t t, uint32_t flags);
/* The same T single-step launches (rows t0 .. t0+T-1) replayed from one hipGraph (async). */
int gu_step_graph(gu_handle h, int64_t t0, int64_t T, uint32_t flags);
/* Copy the current (obs, reward, done) block to the host (any pointer may be NULL). */
int gu_read_outputs(gu_handle h, int32_t *obs, int32_t *reward, int32_t *done);

/* ---- rollout: the caller loop of core/algorithms/monte_carlo.py:7-26 fused -----
 * T env-steps per env in ONE launch (async).  GU_F_TRAJECTORY: the (obs, reward, done) of step i of this call land in row i of the
 * trajectory buffer (gu_reserve_trajectory(T) first; a buffer that is already large enough is kept).  GU_F_STATS: the per-env
 * reward sum and the number of episodes finished during this call are kept for gu_read_stats. */
/* Placement: where a buffer lands in HBM changes its write rate by a few per cent, so buffers of 64 MB and more are CHOSEN: up to
 * GU_OPT_TRAJ_CANDIDATES (4) allocations are written once in the rollout's store shape and the fastest is kept; never more than
 * a tenth of the free memory is held.  (what the search did: gu_trajectory_placement*, include/gu_diag.h.) */
int gu_reserve_trajectory(gu_handle h, int64_t T);
int gu_rollout(gu_handle h, int64_t T, int32_t policy_kind, uint32_t flags);
/* Store pacing: launches that write 128 MB of rows and more keep a schedule -- a wave begins its next 16 steps no earlier than
 * `period` ticks of 10 ns after the last ones were due.  The launches choose the period themselves, closed loop, on the device;
 * results never depend on it.  GU_OPT_ROLLOUT_PACE = 0: no limiter; n > 0: that period, fixed.  (where the
 * loop stands: gu_rollout_pacing, include/gu_diag.h.)  gu_rollout_calibrate is gu_rollout, kept for callers of rounds 3 and 4. */
int gu_rollout_calibrate(gu_handle h, int64_t T, int32_t policy_kind, uint32_t flags);
int gu_read_trajectory(gu_handle h, int64_t t0, int64_t T, int32_t *obs, int32_t *reward, int32_t *done);
int gu_read_trajectory_packed(gu_handle h, int64_t t0, int64_t T, uint32_t *packed);   /* [T][N] after GU_F_PACKED */
int gu_read_stats(gu_handle h, int64_t *reward_sum, int32_t *episodes);

/* ---- state (checkpoint / parity harness) --------------------------------------
 * Any pointer may be NULL.  pos/done int32[N], episode uint32[N], tcount uint64[N]: the steps every env has taken since gu_seed
 * (64 bits: at 4e7 steps per second and env a 32-bit count would wrap, and the action stream repeat, after 97 s; the step counts
 * of one engine must lie within 2^31 of each other -- envs step in lock step, apart only by gu_set_state and rejected actions). */
int gu_get_state(gu_handle h, int32_t *pos, int32_t *done, uint32_t *episode, uint64_t *tcount);
int gu_set_state(gu_handle h, const int32_t *pos, const int32_t *done, const uint32_t *episode, const uint64_t *tcount);

/* gu_get_stores : introspection -- what the engine holds right now, so that no caller has to keep count beside it.  *count =
 *                 GU_STORE_COUNT; with `values`, the first min(capacity, GU_STORE_COUNT) words, indexed by GU_STORE_*.  Host fields of
 *                 the handle only: nothing is synchronised, allocated or copied, nothing a learner carries from launch to launch is
 *                 dropped, and the call works before a grid is set.  A store's word is non-zero exactly when the entry points that
 *                 need the store would find it ("no ...: call gu_*_init first" otherwise): tables left over from a grid of another
 *                 state count read 0.  GU_STORE_TD_ROWS reports the rows of the Q tables only while they are the rows gu_td_run
 *                 learns on now, S << GU_STORE_OVERLAY_BITS; the learners that take no overlay need S rows, which is the same number
 *                 whenever they can run at all. */
enum {
    GU_STORE_S = 0,         /* states of the grid; 0 without a grid */
    GU_STORE_N_GRIDS,       /* grids installed (gu_set_grids, gu_generate_mazes) */
    GU_STORE_OVERLAY,       /* 0 none, 1 wind, 2 fruit, 3 doors, 4 boxes, 5 errands */
    GU_STORE_OVERLAY_BITS,  /* bits of an env's mask in use: F fruits, D door slots, b * B under boxes, F + pb + ib under errands, else 0 */
    GU_STORE_TD_ROWS,       /* rows per env of the Q tables (gu_td_init); 0 = none for the current rows */
    GU_STORE_DOUBLE,        /* states of the pairs of tables (gu_double_init); 0 = none */
    GU_STORE_DYNA,          /* states of the models (gu_dyna_init); 0 = none */
    GU_STORE_SWEEP,         /* 1 while the priority queues (gu_sweep_init) exist for the current models, else 0 */
    GU_STORE_EXPLORE,       /* states of the visit counts (gu_explore_init); 0 = none */
    GU_STORE_EXPLORE_C,     /* entries of the exploration schedule (gu_explore_set_tables); 0 = none */
    GU_STORE_MCTS_NODES,    /* nodes per env of the tree search's pools (gu_mcts_init: max_sims + 1); 0 = none */
    GU_STORE_MCTS_C,        /* entries of the tree search's schedule (gu_mcts_set_tables); 0 = none */
    GU_STORE_AC,            /* states of the actor-critic tables (gu_ac_init); 0 = none */
    GU_STORE_IS,            /* states of the cumulative importance weights (gu_is_init); 0 = none */
    GU_STORE_FA_F,          /* features of the weight tables (gu_fa_init); 0 = none */
    GU_STORE_FA_K,          /* slots per state of the feature table; 0 = none */
    GU_STORE_TRAIL_CAP,     /* trail entries per env (gu_trail_enable); 0 = off */
    GU_STORE_COUNT
};
int gu_get_stores(gu_handle h, int32_t capacity, int64_t *values, int32_t *count);

/* Ascending indices of envs whose done flag is set.  Every kernel that writes done[] (step, rollout, reset,
 * sweep-step) also writes its waves' 64-bit ballot of the new flags -- 8 KB at 65 536 envs -- so this call is ONE
 * launch: a single-workgroup scan + expansion of those words straight into page-locked memory (only a done[]
 * installed with gu_set_state needs a ballot pass first).  Batched form of the harness's `if done: env.reset()`
 * bookkeeping (core/algorithms/monte_carlo.py:19-25).  idx has room for N entries. */
int gu_done_indices(gu_handle h, int32_t *idx, int32_t *count);

/* ---- batched tabular TD control: N independent learners, learner e owns env e and its own float64 table Q_e[S][4] ----
 * (build-defined: the reference lists Q-learning and SARSA on its roadmap and ships no TD code; tests/_td_oracle.py is the CPU
 * restatement.)  One iteration of gu_td_run for env e at 64-bit step count t:
 *   1. if done: reset as gu_step under GU_F_AUTO_RESET does (start from RNG stream 1 at `episode`, then episode += 1) -- always on;
 *   2. w = the word of RNG stream 4 with counter t & 0xFFFFFFFF and epoch t >> 32 (keyed like streams 0 and 2).  Explore iff
 *      (w >> 16) < eps_q16 (0 .. 65536; 65536 = always): action w & 3.  Else greedy on Q_e[s]: of the m actions whose value equals
 *      the row maximum exactly, in ascending order, the one at index (((w >> 2) & 0x3FFF) * m) >> 14.  SARSA uses the carried
 *      action a' instead -- inside a launch always, and at its start when it directly follows a SARSA gu_td_run on this engine
 *      (no gu_seed, gu_reset*, gu_step*, gu_rollout, gu_set_state, gu_set_grid(s), gu_generate_mazes, gu_td_init, gu_td_set_q, gu_dyna_run,
 *      gu_sweep_run, gu_nstep_run, gu_search_run, gu_explore_run, gu_mcts_run, gu_esarsa_run, gu_double_run or sweep-step call in
 *      between);
 *   3. (s', r, d) by the engine's move rule (absorbing terminal); t += 1;
 *   4. float64, one rounding per operation: m = max Q_e[s'] (Q-learning) or Q_e[s'][a'] with a' drawn at s' by rule 2 from the word
 *      of the new t and the pre-update row (SARSA; not drawn when d); target = r if d else r + gamma * m;
 *      Q_e[s][a] += alpha * (target - Q_e[s][a]).
 * gu_td_init  : allocate the tables (N * S * 32 bytes; GU_ERR_NOMEM when free device memory cannot hold them with 1 GiB to
 *               spare) and set every entry to q0.  A grid of another size drops the tables (gu_td_init again).
 * gu_td_run   : T iterations per env in ONE launch (async).  method 0 = Q-learning, 1 = SARSA.  GU_F_TRAJECTORY writes the
 *               (obs, reward, done) rows as gu_rollout does (gu_read_trajectory), GU_F_STATS the per-env sums for gu_read_stats;
 *               no other flag.  GU_ERR_STATE before gu_td_init; GU_ERR_INVALID for a method other than 0 / 1, eps_q16 > 65536,
 *               non-finite alpha or gamma, T < 0.  The step counts advance by T.
 * gu_td_get_q / gu_td_set_q : tables of envs env0 .. env0+n-1 as q[n][S][4] on the host. */
int gu_td_init(gu_handle h, double q0);
int gu_td_run(gu_handle h, int64_t T, int32_t method, double alpha, double gamma, uint32_t eps_q16, uint32_t flags);
int gu_td_get_q(gu_handle h, int64_t env0, int64_t n, double *q);
int gu_td_set_q(gu_handle h, int64_t env0, int64_t n, const double *q);

/* ---- batched tabular Expected SARSA (Sutton & Barto 6.6): learner e owns env e and its table Q_e[S][4] (the gu_td_* tables) ----
 * (build-defined; tests/_double_oracle.py is the CPU restatement.)  One iteration of gu_esarsa_run for env e at step count t:
 *   1. reset and action as gu_td_run's rules 1 and 2 for Q-learning: one word of RNG stream 4 per step, no carried action, no
 *      second draw;
 *   2. (s', r, d) by the engine's move rule; t += 1; n = the pre-update row Q_e[s'] (not read when d);
 *   3. the mean of n under the epsilon-greedy policy of rule 1, float64 with one rounding per operation and no division: with
 *      pe = eps_q16 * 2^-18 and pg = (65536 - eps_q16) * 2^-16 (both exact), sum = ((n[0] + n[1]) + n[2]) + n[3] and mx = the row
 *      maximum, E = pe * sum + pg * mx.  (The m tied maxima all equal mx, so their mean is mx whatever m is.)
 *   4. target = r if d else r + gamma * E;  Q_e[s][a] += alpha * (target - Q_e[s][a]).
 * With eps_q16 = 0 (E = 0 * sum + 1 * mx) a launch gives the bytes of gu_td_run's Q-learning on finite tables without negative zeros.
 * Launches alternate freely with gu_td_run and the other learners on the same tables; a launch ends what they carry (SARSA actions,
 * windows, episode buffers).  Flags and errors as gu_td_run; GU_ERR_UNSUPPORTED while wind, fruit or doors are set. */
int gu_esarsa_run(gu_handle h, int64_t T, double alpha, double gamma, uint32_t eps_q16, uint32_t flags);

/* ---- batched greedy evaluation: env e walks K test episodes of at most L steps on its table Q_e (the gu_td_* tables, S << overlay_bits
 * rows), nothing learns and nothing of the engine moves ----
 * (build-defined; tests/_eval_oracle.py is the CPU restatement.)  Test episode k of env e:
 *   1. Start: what a reset at episode count k gives a freshly seeded env: the cell starts[gu_rng_start_index(stream 1, k, n_starts)] of
 *      the env's grid -- or first_state[k][e] where first_state is given (the cell only) --, and the overlay word that reset leaves: 0,
 *      the boxes' word at reset, or under errands the instruction drawn on stream 11 at count k.  The env's own pos, done, episode,
 *      tcount and word are neither read nor written.
 *   2. A start cell whose terminal bit is set ends the episode at once: len = 0, ret = 0, disc = 0, outcome by rule 6.
 *   3. Step i takes the FIRST of the actions whose value equals the row maximum exactly, in ascending order; the maximum is folded left
 *      to right with `>` as in gu_td_run.  Where no entry compares equal (a NaN in entry 0) the action is 0.  No RNG word is drawn.
 *      (np.argmax on finite rows.)
 *   4. (s', r, d) by the engine's move rule, or the overlay's, at step count k * L + i in epoch 0 (a gust is the stream-9 word at that
 *      counter).  Under fruit, doors, boxes and errands the row is word * S + s.
 *   5. ret += r (int32);  disc = disc + w * (double)r;  w = w * gamma, from w = 1.0 and disc = 0.0, float64 with one rounding per
 *      operation;  len += 1.  The episode ends when d is set or after L steps.
 *   6. outcome: 0 = L steps without an end; 1 = ended on a terminal cell whose reward is the positive one (goal); 2 = ended on any
 *      other terminal cell (lava); 3 = ended by the overlay while the cell's terminal bit is clear (boxes solved, errand completed, or
 *      an absorbing completed word).  end = the last cell; word = the last overlay word (0 under no overlay and under wind; under
 *      errands the instruction's index stays readable in it).
 * The outputs are host arrays [K][N]; any of them may be NULL.  The call is synchronous.
 * GU_ERR_STATE without a grid or before gu_td_init.  GU_ERR_INVALID for K < 1, L < 1, K * L > 1e8 (the learners' budget; it keeps the
 * step count below 2^32), K > 65535 or K * N > 2^24 (the launch's second dimension, and 32 bytes of scratch per test episode: 512 MiB),
 * a non-finite gamma, or a first_state outside 0 .. S-1 (the message names the first offender); nothing is written then.
 * The call has no other effect: what the learners carry (SARSA's next action, windows, episode buffers), the trajectory buffer, the
 * statistics, the done ballots, the step graph and gu_get_stores are as before, and the agent trail does not refuse it.  It serves
 * single-grid engines under every overlay and multi-grid engines in all their forms. */
int gu_td_evaluate(gu_handle h, int32_t K, int32_t L, double gamma, const int32_t *first_state, int32_t *ret, int32_t *len,
                   int32_t *outcome, int32_t *end, uint32_t *word, double *disc);

/* ---- batched tabular Double Q-learning (Sutton & Barto 6.7): learner e owns env e and a PAIR of tables A_e[S][4], B_e[S][4] ----
 * (build-defined; tests/_double_oracle.py is the CPU restatement.)  The pair is storage of its own, q[N][S][2][4] float64 -- the A
 * row and the B row of a state side by side --, not the gu_td_* tables.  One iteration of gu_double_run for env e at step count t,
 * after the lazy reset of gu_td_run's rule 1:
 *   1. the action by gu_td_run's rule 2 (without a carried action) on the row A_e[s][.] + B_e[s][.] (one rounded add per entry), with
 *      the word of RNG stream 4 at t;
 *   2. the coin c = bit 0 of the word of RNG stream 10 with counter t & 0xFFFFFFFF and epoch t >> 32 (keyed exactly like stream 4),
 *      at the same t: c = 0 updates A from B's estimate (X = A, Y = B), c = 1 updates B from A's (X = B, Y = A);
 *   3. (s', r, d) by the engine's move rule; t += 1; the pre-update pair of s' (not read when d);
 *   4. a* = the lowest action with X[s'][a*] equal to the maximum of row X[s'] (action 0 if none compares equal); est = Y[s'][a*];
 *      target = r if d else r + gamma * est;  X[s][a] += alpha * (target - X[s][a]), float64, one rounding per operation;
 *   5. that entry is the step's one store (8 bytes).
 * gu_double_init  : allocate the pairs (N * S * 64 bytes; GU_ERR_NOMEM when free device memory cannot hold them with 1 GiB to spare)
 *                   and set every entry of both tables to q0.  A grid of another state count drops them (gu_double_init again).
 * gu_double_run   : T iterations per env in ONE launch (async); flags and argument errors as gu_td_run.  GU_ERR_STATE before
 *                   gu_double_init, GU_ERR_UNSUPPORTED while wind, fruit or doors are set.  A launch ends what the other learners
 *                   carry (SARSA actions, windows, episode buffers).  The step counts advance by T.
 * gu_double_get_q / gu_double_set_q : pairs of envs env0 .. env0+n-1 as q[n][S][2][4] on the host. */
int gu_double_init(gu_handle h, double q0);
int gu_double_run(gu_handle h, int64_t T, double alpha, double gamma, uint32_t eps_q16, uint32_t flags);
int gu_double_get_q(gu_handle h, int64_t env0, int64_t n, double *q);
int gu_double_set_q(gu_handle h, int64_t env0, int64_t n, const double *q);

/* ---- batched tabular Dyna-Q: learner e owns env e, its table Q_e[S][4] (the gu_td_* tables) and a learned model ----
 * (build-defined: the reference lists "Integrating learning and planning (Dyna, ...)" on its roadmap and ships no code; Sutton &
 * Barto 8.2; tests/_dyna_oracle.py is the CPU restatement.)  The model of learner e: next_e[S][4] (int32, -1 = never observed),
 * reward_e[S][4] (int32), done_e[S][4] (0/1); list_e[4S], the observed pairs s*4+a in the order they were FIRST observed; count_e,
 * its entries.  The env is deterministic, so one stored outcome per (s, a) is the whole model.
 * One iteration of gu_dyna_run for env e at 64-bit step count t:
 *   1. real step: rules 1-4 of gu_td_run, method 0 (Q-learning), unchanged (lazy auto-reset, the stream-4 word at count t,
 *      epsilon-greedy with its tie rule, the move, t += 1, the float64 update of Q_e[s][a]);
 *   2. model: next/reward/done[s][a] = (s', r, d) as observed; if (s, a) had never been observed, list_e[count_e++] = s*4+a;
 *   3. planning: for j = 0 .. P-1, c = t_old * P + j (64-bit; t_old = the count before rule 1's increment): w = the word of RNG
 *      stream 5 with counter c & 0xFFFFFFFF and epoch c >> 32 (keyed like stream 4); k = (uint64(w) * count_e) >> 32;
 *      p = list_e[k], s_p = p >> 2, a_p = p & 3, (s'_p, r_p, d_p) from the model; target = r_p if d_p, else
 *      r_p + gamma * max Q_e[s'_p] (folded left to right with `>` over the row as it is now, earlier planning updates of this
 *      iteration included); Q_e[s_p][a_p] += alpha * (target - Q_e[s_p][a_p]), float64, one rounding per operation;
 *   4. the next iteration chooses its action from the table after planning.
 * Trajectory rows and GU_F_STATS cover the real steps only.  The step counts advance by T.
 * gu_dyna_init      : allocate the model of every env (N * S * 49 bytes; GU_ERR_NOMEM under gu_td_init's free-memory rule) and
 *                     clear it (count 0, all pairs unobserved).  gu_td_init and gu_td_set_q leave the model alone; a grid of another
 *                     size drops it with the Q tables.
 * gu_dyna_run       : T iterations per env with P planning updates each, in ONE launch (async).  GU_ERR_STATE without Q tables
 *                     (gu_td_init) or without a model; GU_ERR_INVALID for P < 0 or P > 256, T * (P + 1) > 1e8, and everything
 *                     gu_td_run rejects.  T = 0 changes nothing.  Flags as gu_td_run.  Ends the SARSA carry.
 * gu_dyna_get_model : the model of envs env0 .. env0+n-1 on the host: next, reward, done as [n][S][4] (unobserved pairs: -1, 0, 0),
 *                     list as [n][4S] (-1 beyond count), count as [n]; any output pointer may be NULL. */
int gu_dyna_init(gu_handle h);
int gu_dyna_run(gu_handle h, int64_t T, int32_t P, double alpha, double gamma, uint32_t eps_q16, uint32_t flags);
int gu_dyna_get_model(gu_handle h, int64_t env0, int64_t n, int32_t *next, int32_t *reward, int32_t *done, int32_t *list, int32_t *count);

/* ---- batched prioritized sweeping: learner e owns env e, its table Q_e[S][4] (the gu_td_* tables), its Dyna-Q model and a queue ----
 * (build-defined: the reference ships no code for it; Sutton & Barto 8.4; tests/_sweep_oracle.py is the CPU restatement.)  The model
 * is the one gu_dyna_run fills (next / reward / done / list / count above, the same buffers).  The queue of learner e is a set of
 * observed pairs p = s*4+a, each under a 64-bit key:
 *   key(p, x) = ((bits(x) >> 16) << 16) | p for a float64 priority x > 0, bits(x) its pattern: the priority truncated to 36 mantissa
 *   bits, ties broken by the larger pair index.  The pair index has 16 bits, so the queue needs 4 * S <= 65 536 (S <= 16 384: a
 *   128 x 128 grid fits).  Key 0 = not queued.  Keys are ordered as uint64, a total order: what a pop returns does not depend on how
 *   the device stores the queue.
 *   insert(p, x): only if x > theta and (bits(x) >> 16) != 0 (a NaN x fails the first test); then key_e[p] = max(key_e[p], key(p, x)) --
 *   a pair that is queued keeps the larger priority.
 * One iteration of gu_sweep_run for env e at 64-bit step count t:
 *   1. real step: rules 1-3 of gu_td_run, method 0 (lazy auto-reset, the stream-4 word at count t, epsilon-greedy with its tie rule, the
 *      move, t += 1) -- and NO update of Q_e[s][a]: all learning goes through the queue;
 *   2. model: rule 2 of gu_dyna_run, unchanged;
 *   3. priority of the real pair: target = r if d, else r + gamma * max Q_e[s'] (folded left to right with `>`); x = |target -
 *      Q_e[s][a]|, float64, one rounding per operation; insert(s*4+a, x);
 *   4. planning: up to P times, ending early when the queue is empty: remove the pair p with the largest key, S = p >> 2, A = p & 3,
 *      (S', R, D) from the model; tgt = R if D, else R + gamma * max Q_e[S'] over the row as it is now; Q_e[S][A] += alpha * (tgt -
 *      Q_e[S][A]); then for every candidate cell c of {S, S - W, S + 1, S + W, S - 1} with 0 <= c < S_cells (W = the current grid's
 *      width) and every action b of 0 .. 3 whose pair (c, b) is observed with next_e[c][b] == S: with (R', D') of that pair,
 *      x' = |(R' if D' else R' + gamma * max Q_e[S]) - Q_e[c][b]|, insert(c*4+b, x').  (Inserts commute and Q is only read, so the
 *      order of the candidates does not matter.  A move displaces the agent by at most one cell and nothing wraps, so on a model
 *      recorded under the current grid these 20 candidates are ALL predecessors of S; the rule is geometric so that it stays
 *      defined on a model kept across a grid install of equal S and another W.)
 *   5. the next iteration chooses its action from the table after planning.
 * Trajectory rows and GU_F_STATS cover the real steps only.  The step counts advance by T.  Planning draws nothing: no RNG stream.
 * gu_sweep_init      : gu_dyna_init (allocate the model if need be, clear it), plus the queue: allocated if need be (N * (S * 48 + 20)
 *                      bytes under gu_td_init's free-memory rule) and emptied.  GU_ERR_INVALID if 4 * S > 65 536.  gu_dyna_init
 *                      empties an existing queue with the model (a queued pair never outlives its model entry); a grid of another
 *                      size drops the queue with the model.
 * gu_sweep_run       : T iterations per env with up to P planning updates each, in ONE launch (async).  GU_ERR_STATE without Q tables
 *                      (gu_td_init) or without a queue for the current S; GU_ERR_INVALID for P < 0 or P > 256, theta negative or not
 *                      finite, T * (P + 1) > 1e8, and everything gu_dyna_run rejects.  T = 0 changes nothing.  Flags as gu_td_run.
 *                      Refused while wind is set, as gu_dyna_run; ends the other learners' carries as gu_dyna_run does.
 * gu_sweep_get_queue : the queues of envs env0 .. env0+n-1 on the host: key as [n][S][4] (0 = not queued), size as [n]; either
 *                      pointer may be NULL.
 * gu_diag_sweep_heap : introspection -- the device's raw form of those queues, one binary max-heap per env: heap as [n][4S+2]
 *                      (slots 1 .. size hold the keys, every parent i >= its children 2i and 2i+1; slot 0 holds two counters since
 *                      gu_sweep_init, pops in the low half and inserts that changed the queue in the high half, each modulo 2^32; the
 *                      other slots are stale), pos as [n][4S] (the slot of each queued pair, -1 elsewhere); either may be NULL. */
int gu_sweep_init(gu_handle h);
int gu_sweep_run(gu_handle h, int64_t T, int32_t P, double theta, double alpha, double gamma, uint32_t eps_q16, uint32_t flags);
int gu_sweep_get_queue(gu_handle h, int64_t env0, int64_t n, uint64_t *key, int32_t *size);
int gu_diag_sweep_heap(gu_handle h, int64_t env0, int64_t n, uint64_t *heap, int32_t *pos);
/* gu_diag_rollout_form : introspection -- what the last gu_rollout of this engine ran on, as the launcher planned it
 *                      (csrc/gu_rollout_plan.hpp; DESIGN.md "Rollout dispatch").  *count = 12 words; with `form`, capacity >= 12:
 *                      kernel family (1 general, 2 transition-row, 3 K-step, 4 windy, 5 fruit, 6 doors, 7 boxes, 8 errands); row layout (0 none, 1 planes, 2 packed, 3 triples);
 *                      MAP of the general kernel (0 / 1 / 3 / 5), else -1; workgroup size; workgroups; dynamic LDS bytes; flag bits (1 pair
 *                      tables, 2 half waves, 4 per-wave grids, 8 thresholds in LDS, 16 straddles a 2^32-step boundary, 32 first step on the
 *                      table, 64 XCD-aware block order); K of the K-step kernel; log2 of the table's row pitch; staged action words per lane;
 *                      the store-pacing slot (-1 none); 0 unpaced / 1 closed loop / 2 fixed period.  All zeros before the first rollout. */
int gu_diag_rollout_form(gu_handle h, int32_t *form, int32_t capacity, int32_t *count);

/* ---- batched simulation-based search: learner e owns env e and its table Q_e[S][4] (the gu_td_* tables) and plans at decision time ----
 * (build-defined: the second half of the reference's roadmap entry "Integrating learning and planning (Dyna, MC/TD Tree search,
 * Forward and Simulation-based search)", for which it ships no code; the "rollout algorithm" of Sutton & Barto 8.10, "simple
 * Monte-Carlo search" of Silver's lecture 8; tests/_search_oracle.py is the CPU restatement.)  gu_dyna_run plans in the background
 * from a LEARNED model; this learner plans before each real move, from the current state, with the TRUE model: the engine's move
 * rule.  It chooses each non-exploring real action by M simulated rollouts per action, of depth D, under an epsilon-greedy rollout
 * policy on Q_e; a truncated rollout bootstraps on max Q_e at its leaf; the real transition is learned from by Q-learning.
 * One iteration of gu_search_run for env e at 64-bit step count t:
 *   1. reset: lazy auto-reset, exactly as rule 1 of gu_td_run;
 *   2. w = the stream-4 word at t (as rule 2 of gu_td_run);
 *   3. action.  If (w >> 16) < eps_q16: a = w & 3 and NO simulation is run.  Else if M = 0: a by rule 2 of gu_td_run on Q_e[s].
 *      Else search: for each action b = 0 .. 3 in order, (s1, r1, d1) is the move rule from (s, b) -- the env itself does not
 *      move --, and for j = 0 .. M-1:
 *        G = (double)r1, disc = gamma, x = s1, dn = d1;
 *        for i = 0 .. D-1, while not dn: c = ((t * 4 + b) * M + j) * D + i (uint64, wrapping); w' = the word of RNG stream 6
 *          with counter c & 0xFFFFFFFF and epoch c >> 32 (keyed like streams 4 and 5); u = rule 2 of gu_td_run applied to the
 *          row Q_e[x] with w' and eps_sim_q16; (x', r', dn) = the move rule from (x, u); G = G + disc * r', then
 *          disc = disc * gamma, then x = x';
 *        after the loop, if not dn: G = G + disc * max Q_e[x], folded left to right with `>`;
 *      score_b = ((G_0 + G_1) + ...) + G_{M-1} -- sums, not means: no division.  a = the tie rule of rule 2 applied to the score
 *      row with w: the k-th (ascending) of the m exactly-maximal actions, k = (((w >> 2) & 0x3FFF) * m) >> 14.  No table entry is
 *      written during a search;
 *   4. (s', r, d) by the engine's move rule (absorbing terminal); t += 1;
 *   5. the Q-learning update of rule 4 of gu_td_run, method 0, on Q_e[s][a];
 *   6. the next iteration sees the updated table.
 * All float64, one rounding per operation, multiply / add / subtract only.  With M = 0 this is gu_td_run, method 0, byte for byte,
 * for any D and eps_sim_q16.  There is no carry; gu_search_run ends every other learner's carry, window and episode buffer.
 * gu_search_run : T iterations per env in ONE launch (async).  GU_ERR_STATE before gu_td_init; GU_ERR_INVALID for M outside
 *                 0 .. GU_SEARCH_MAX_M, D outside 0 .. GU_SEARCH_MAX_D, either epsilon above 65536, T * (1 + 4 M D) > 1e8
 *                 (gu_dyna_run's launch bound) and everything gu_td_run rejects.  T = 0 changes nothing.  Flags, rows, statistics,
 *                 the agent trail and the step counts as gu_td_run: the T real steps only.
 * gu_search_get : of envs env0 .. env0+n-1 on the host: score as [n][4], the score row of each env's most recent SEARCHED
 *                 iteration (zeros until there is one); sim_steps as [n], the simulated moves of the last launch (the inner i
 *                 steps only, not the four first moves).  Either pointer may be NULL.  The storage (N * 40 bytes) is allocated on
 *                 first use (GU_ERR_NOMEM under gu_td_init's free-memory rule); a grid of another size drops it with the tables. */
#define GU_SEARCH_MAX_M 64
#define GU_SEARCH_MAX_D 256
int gu_search_run(gu_handle h, int64_t T, int32_t M, int32_t D, double alpha, double gamma, uint32_t eps_q16, uint32_t eps_sim_q16,
                  uint32_t flags);
int gu_search_get(gu_handle h, int64_t env0, int64_t n, double *score, int64_t *sim_steps);

/* ---- batched count-based exploration: learner e owns env e, its table Q_e[S][4] (the gu_td_* tables) and visit counts N_e[S][4] ----
 * (build-defined: the last entry of the reference's roadmap, "Exploration vs Exploitation (Optimistic policy, optimistic policy
 * with uncertainty, Thompson sampling, UCB)", for which it ships no code; Sutton & Barto 2.7 (UCB action selection), Silver's
 * lecture 9; tests/_explore_oracle.py is the CPU restatement.  "Optimistic policy" is gu_td_init's q0.)  Tabular Q-learning whose
 * ACTION CHOICE is driven by the learner's own counts: N_e[S][4], uint32, learner-major [N][S][4], saturating at
 * GU_EXPLORE_COUNT_MAX.  Two float64 tables shared by all learners, U[C] and B[C], supplied by the host, turn counts into a bonus:
 * the exploration schedule is data, and the kernel computes no log, sqrt or division.
 * One iteration of gu_explore_run for env e at 64-bit step count t:
 *   1. reset: lazy auto-reset, exactly as rule 1 of gu_td_run;
 *   2. w = the stream-4 word at t (as rule 2 of gu_td_run).  If (w >> 16) < eps_q16: a = w & 3;
 *   3. else: n_b = N_e[s][b], n_s = n_0 + n_1 + n_2 + n_3 (fits 32 bits: the counts saturate); u = U[min(n_s, C-1)];
 *      p_b = u * B[min(n_b, C-1)];
 *        mode 0 (UCB)      : score_b = Q_e[s][b] + p_b;
 *        mode 1 (Thompson) : score_b = Q_e[s][b] + (p_b * z_b), z_b = the integer-valued double (byte0 + byte1 + byte2 + byte3 of
 *                            x_b) - 510, where x_0 = the word of RNG stream 7 with counter t & 0xFFFFFFFF and epoch t >> 32 (keyed
 *                            exactly like stream 4) and x_{b+1} = next(x_b), the bijection of stream 2 (gu_rng.hpp:
 *                            gu_rng_sample_next).  z_b is an Irwin-Hall approximate normal of variance 21845: the host folds
 *                            1 / sqrt(21845) into B;
 *      a = the greedy branch of rule 2 of gu_td_run applied to the score row: the maximum folded left to right with `>`, of the m
 *      actions whose score equals it exactly the one at index (((w >> 2) & 0x3FFF) * m) >> 14;
 *   4. N_e[s][a] = min(N_e[s][a] + 1, GU_EXPLORE_COUNT_MAX) -- on exploring steps too, after the choice;
 *   5. (s', r, d) by the engine's move rule; t += 1; the Q-learning update of rule 4 of gu_td_run, method 0, on Q_e[s][a].  The bonus
 *      never enters the table.
 * All float64, one rounding per operation, multiply and add only.  With U or B all zero either mode is gu_td_run, method 0, byte for
 * byte (tables, rows, statistics, env state, step counts); the counts are an extra.  There is no carry; gu_explore_run ends every
 * other learner's carry, window and episode buffer, as gu_search_run does.
 * gu_explore_init       : allocate the counts (N * S * 16 bytes; GU_ERR_NOMEM under gu_td_init's free-memory rule) and zero them.
 *                         GU_ERR_STATE before gu_td_init.  gu_td_init and gu_td_set_q leave the counts alone; a grid of another
 *                         size drops them (gu_explore_init again).
 * gu_explore_set_tables : copy U[C] and B[C] (they stay until the next call, across grids).  GU_ERR_INVALID unless
 *                         2 <= C <= GU_EXPLORE_MAX_C and every entry is finite and >= 0.
 * gu_explore_run        : T iterations per env in ONE launch (async).  mode 0 = UCB, 1 = Thompson.  GU_ERR_STATE before
 *                         gu_td_init, gu_explore_init or gu_explore_set_tables; GU_ERR_INVALID for another mode and everything
 *                         gu_td_run rejects.  T = 0 changes nothing.  Flags, rows, statistics, the agent trail and the step counts
 *                         as gu_td_run.
 * gu_explore_get_counts / gu_explore_set_counts : counts of envs env0 .. env0+n-1 as counts[n][S][4] on the host; set rejects a
 *                         value above GU_EXPLORE_COUNT_MAX (GU_ERR_INVALID) before it writes anything. */
#define GU_EXPLORE_MAX_C 4096
#define GU_EXPLORE_COUNT_MAX 0x3FFFFFFFu
int gu_explore_init(gu_handle h);
int gu_explore_set_tables(gu_handle h, int32_t C, const double *U, const double *B);
int gu_explore_run(gu_handle h, int64_t T, int32_t mode, double alpha, double gamma, uint32_t eps_q16, uint32_t flags);
int gu_explore_get_counts(gu_handle h, int64_t env0, int64_t n, uint32_t *counts);
int gu_explore_set_counts(gu_handle h, int64_t env0, int64_t n, const uint32_t *counts);

/* ---- batched Monte-Carlo tree search (UCT): learner e owns env e, its table Q_e[S][4] (the gu_td_* tables) and a pool of tree nodes ----
 * (build-defined: the "MC/TD Tree search" half of the reference's roadmap entry "Integrating learning and planning (Dyna, MC/TD Tree
 * search, Forward and Simulation-based search)", for which it ships no code; Kocsis & Szepesvari's UCT, Sutton & Barto 8.11;
 * tests/_mcts_oracle.py is the CPU restatement.)  gu_search_run spends a fixed budget of rollouts on every action; this learner
 * builds a TREE at the state it stands in, before each non-exploring real move, with the TRUE model (the engine's move rule), and
 * spends its M simulations where the tree's own statistics point.  Node 0 is the root; nodes are numbered in order of creation;
 * node v holds its state x_v, its parent link (parent * 4 + action; -1 for the root), child_v[4] (node index, -1 = none), visit
 * counts n_v[4] (uint32) and return sums w_v[4] (float64).  Three float64 tables shared by all learners, U[C], B[C] and I[C],
 * supplied by the host, every index clamped to C - 1, turn counts into the UCB1 bonus and sums into means: the kernel computes no
 * log, sqrt or division.
 * One iteration of gu_mcts_run for env e at 64-bit step count t:
 *   1. reset: lazy auto-reset, exactly as rule 1 of gu_td_run;
 *   2. w = the stream-4 word at t (as rule 2 of gu_td_run);
 *   3. action.  If (w >> 16) < eps_q16: a = w & 3 and NO simulation is run.  Else if M = 0: a by rule 2 of gu_td_run on Q_e[s].
 *      Else the tree is rebuilt from scratch -- node 0 = s without children, counts 0, sums 0.0; one node -- and for j = 0 .. M-1
 *      one simulation runs.  Its draws are the words of RNG stream 8 with counter c & 0xFFFFFFFF and epoch c >> 32 (keyed like
 *      streams 4 - 7), c = (t * M + j) * (H + D) + i (uint64, wrapping), i = the draws the simulation has made so far:
 *        selection: v = 0, depth = 0.  At node v: n_s = n_v[0] + n_v[1] + n_v[2] + n_v[3]; score_b = +infinity if n_v[b] == 0, else
 *          (w_v[b] * I[n_v[b]]) + (U[n_s] * B[n_v[b]]); u = the greedy branch of rule 2 of gu_td_run applied to the score row with
 *          the next stream-8 word (the maximum folded left to right with `>`, of the m exactly-maximal actions the one at index
 *          (((w' >> 2) & 0x3FFF) * m) >> 14); (x', r', dn) = the move rule from (x_v, u); depth += 1.  If dn: tail = 0.0 and the
 *          simulation goes to its backup.  Else if child_v[u] >= 0 and depth < H: v = child_v[u], again.  Else: if child_v[u] < 0
 *          a node for x' is created (no children, counts 0, sums 0.0, parent link v * 4 + u, child_v[u] = its index) -- at the
 *          depth cap too --, and in either case a rollout starts at x';
 *        rollout (gu_search_run's): G = 0.0, disc = 1.0, x = x'; up to D times, while not terminal: u = rule 2 of gu_td_run
 *          applied to the row Q_e[x] with the next stream-8 word and eps_sim_q16; (x, r, dn) = the move rule from (x, u);
 *          G = G + disc * r, then disc = disc * gamma.  After the loop, if not dn: G = G + disc * max Q_e[x], folded left to right
 *          with `>`.  tail = G.  (D = 0: tail = 0.0 + 1.0 * max Q_e[x'], the TD-tree-search case.);
 *        backup: G = tail; for each edge of the path, from the last one (v, u) -- its reward r' -- up to the root's:
 *          G = r_edge + gamma * G, then w[edge] = w[edge] + G and n[edge] += 1.
 *      After the M simulations the final row is -infinity where n_0[b] == 0, else w_0[b] * I[n_0[b]] -- the MEAN return of the root
 *      action, not its visit count --, and a = the tie rule of rule 2 applied to that row with w.  No Q_e entry is written during
 *      a search;
 *   4. (s', r, d) by the engine's move rule (absorbing terminal); t += 1;
 *   5. the Q-learning update of rule 4 of gu_td_run, method 0, on Q_e[s][a]; the next iteration sees the updated table.
 * All float64, one rounding per operation, multiply / add / subtract only.  With M = 0 this is gu_td_run, method 0, byte for byte,
 * for any H, D, tables and eps_sim_q16.  There is no carry; gu_mcts_run ends every other learner's carry, window and episode
 * buffer, as gu_search_run does.  A tree lives for one decision: nothing is reused between decisions and states met twice in one
 * tree are two nodes.
 * gu_mcts_init       : allocate a pool of max_sims + 1 nodes per env (1 <= max_sims <= GU_MCTS_MAX_SIMS; N * (max_sims + 1) * 72
 *                      bytes; GU_ERR_NOMEM under gu_td_init's free-memory rule) and empty it.  GU_ERR_STATE before gu_td_init.  A
 *                      grid of another size drops the pool with the Q tables (gu_mcts_init again).
 * gu_mcts_set_tables : copy U[C], B[C] and I[C] (they stay until the next call, across grids).  GU_ERR_INVALID unless
 *                      2 <= C <= GU_EXPLORE_MAX_C and every entry is finite and >= 0.  UCB1 with constant k: U[n] = k sqrt(ln(n + 1)),
 *                      B[n] = 1 / sqrt(n), I[n] = 1 / n, B[0] = I[0] = 0 (index 0 is never read: an untried action scores infinity).
 * gu_mcts_run        : T iterations per env in ONE launch (async).  GU_ERR_STATE before gu_td_init or gu_mcts_init, and, when M > 0,
 *                      before gu_mcts_set_tables; GU_ERR_INVALID for M outside 0 .. max_sims, H outside 1 .. GU_MCTS_MAX_DEPTH, D
 *                      outside 0 .. GU_SEARCH_MAX_D, either epsilon above 65536, T * (1 + M (H + D)) > 1e8 (gu_dyna_run's launch
 *                      bound) and everything gu_td_run rejects.  T = 0 changes nothing.  Flags, rows, statistics, the agent trail
 *                      and the step counts as gu_td_run: the T real steps only.
 * gu_mcts_get        : of envs env0 .. env0+n-1 on the host, from each env's most recent SEARCHED iteration: w as [n][4] and visits
 *                      as [n][4], the root's rows (zeros until there is one); nodes as [n], the nodes of that tree; sim_steps as
 *                      int64 [n], the simulated moves of the last launch, selection and rollout moves alike.  Any pointer may be NULL.
 * gu_mcts_get_tree   : the whole tree of that iteration: state, parent as [n][max_sims + 1], child, visits, w as
 *                      [n][max_sims + 1][4], count as [n]; entries of nodes beyond count are -1, -1, -1, 0, 0.0.  Any pointer may
 *                      be NULL. */
#define GU_MCTS_MAX_SIMS 255
#define GU_MCTS_MAX_DEPTH 64
int gu_mcts_init(gu_handle h, int32_t max_sims);
int gu_mcts_set_tables(gu_handle h, int32_t C, const double *U, const double *B, const double *I);
int gu_mcts_run(gu_handle h, int64_t T, int32_t M, int32_t H, int32_t D, double alpha, double gamma, uint32_t eps_q16, uint32_t eps_sim_q16,
                uint32_t flags);
int gu_mcts_get(gu_handle h, int64_t env0, int64_t n, double *w, uint32_t *visits, int32_t *nodes, int64_t *sim_steps);
int gu_mcts_get_tree(gu_handle h, int64_t env0, int64_t n, int32_t *state, int32_t *parent, int32_t *child, uint32_t *visits, double *w,
                     int32_t *count);

/* ---- batched tabular n-step Q-learning and n-step SARSA: learner e owns env e and its table Q_e[S][4] (the gu_td_* tables) ----
 * (build-defined: the reference lists "Temporal Difference (TD) Learning with variations" on its roadmap and ships no code;
 * Sutton & Barto ch. 7; method 0 is the uncorrected n-step Q-learning of asynchronous n-step Q-learning, Mnih et al. 2016;
 * tests/_nstep_oracle.py is the CPU restatement.)  Learner e keeps a WINDOW: the pending transitions (s_k, a_k, r_k), oldest
 * first, at most n - 1 of them between iterations.  One iteration of gu_nstep_run for env e at 64-bit step count t:
 *   1. lazy auto-reset, exactly as rule 1 of gu_td_run (the window is empty here: see 5);
 *   2. action: as rule 2 of gu_td_run (the stream-4 word at t, epsilon, the tie rule).  SARSA takes its carried a' instead,
 *      under the same conditions as gu_td_run's SARSA (the carry across launches is the window's, below);
 *   3. (s', r, d) by the engine's move rule; t += 1; append (s, a, r) to the window;
 *   4. if not d: B from the row of s' BEFORE this iteration's update: max Q_e[s'] folded left to right with `>` (Q-learning), or
 *      Q_e[s'][a'] with a' drawn at s' by rule 2 from the word of the new t (SARSA).  If the window now holds n entries:
 *      G = B, then for k from newest to oldest G = r_k + gamma * G; Q_e[s_0][a_0] += alpha * (G - Q_e[s_0][a_0]); drop entry 0;
 *   5. if d: flush.  For each entry, oldest first, G = the Horner sum of its reward and the rewards of the entries after it,
 *      without bootstrap (G = r for the newest); the updates apply in that order, each reading Q_e as the ones before it left it
 *      (a repeated (s, a) compounds).  The window ends empty; SARSA draws no a';
 *   6. the next iteration chooses from the table after this iteration's updates.
 * All float64, one rounding per operation (multiply, then add).  With n = 1 this is gu_td_run, byte for byte, for both methods.
 * CARRY: the window and SARSA's a' persist from one gu_nstep_run to the next when the later call directly follows the earlier one
 * with the same method and n.  Any other call in between -- everything that ends gu_td_run's SARSA carry, gu_td_run,
 * gu_dyna_run, gu_sweep_run, gu_search_run, a gu_nstep_run with another method or n -- drops both; the pending updates are discarded, not flushed.
 * gu_nstep_run ends gu_td_run's SARSA carry.
 * gu_nstep_run        : T iterations per env in ONE launch (async).  method 0 = n-step Q-learning, 1 = n-step SARSA; 1 <= n <=
 *                       GU_NSTEP_MAX.  GU_ERR_STATE before gu_td_init; GU_ERR_INVALID for a bad method or n and everything
 *                       gu_td_run rejects.  The window storage (N * 132 bytes) is allocated on first use (GU_ERR_NOMEM under
 *                       gu_td_init's free-memory rule); a grid of another size drops it with the tables.  T = 0 changes
 *                       nothing.  Flags, rows and statistics as gu_td_run.  The step counts advance by T.
 * gu_nstep_get_window : the windows of envs env0 .. env0+n-1 on the host: sa (s*4+a) and reward as [n][GU_NSTEP_MAX], oldest
 *                       first, (-1, 0) beyond count; count as [n], 0 when the window has been dropped.  Any pointer may be NULL. */
#define GU_NSTEP_MAX 16
int gu_nstep_run(gu_handle h, int64_t T, int32_t method, int32_t n, double alpha, double gamma, uint32_t eps_q16, uint32_t flags);
int gu_nstep_get_window(gu_handle h, int64_t env0, int64_t n, int32_t *sa, int32_t *reward, int32_t *count);

/* ---- batched tabular SARSA(lambda) and Watkins's Q(lambda): learner e owns env e and its table Q_e[S][4] (the gu_td_* tables) ----
 * (build-defined: the reference lists "Temporal Difference (TD) Learning with variations" on its roadmap and ships no code;
 * Sutton & Barto ch. 12, backward view with REPLACING traces truncated after K steps; tests/_lambda_oracle.py is the CPU
 * restatement.)  Learner e keeps a TRACE WINDOW W_e[j], j = 0 .. GU_LAMBDA_MAX-1: the pair s*4+a whose trace has age j, or -1.
 * The pairs of a window are distinct; between iterations W_e[0] = -1 and W_e[j] = -1 for every j >= K.
 * Coefficients, float64, one rounding per operation: c = gamma * lambda, P_0 = 1.0, P_j = P_{j-1} * c.
 * One iteration of gu_lambda_run for env e at 64-bit step count t:
 *   1. lazy auto-reset, exactly as rule 1 of gu_td_run (the window is empty here: see 6);
 *   2. action: as rule 2 of gu_td_run.  SARSA(lambda) takes its carried a' instead, under the same conditions as gu_td_run's SARSA
 *      (the carry across launches is the window's, below).  Watkins's Q(lambda) only: if Q_e[s][a] == max Q_e[s] (folded left to
 *      right with `>`, over the row the action was chosen from) is false, the window is emptied first;
 *   3. (s', r, d) by the engine's move rule; t += 1;
 *   4. m = max Q_e[s'] (Q(lambda)) or Q_e[s'][a'] with a' drawn at s' by rule 2 from the word of the new t and the pre-update row
 *      (SARSA(lambda); not drawn when d); target = r if d else r + gamma * m; delta = target - Q_e[s][a]; g = alpha * delta;
 *   5. if (s, a) is in the window, that entry is removed; W_e[0] = s*4+a.  For every j < K with W_e[j] >= 0 and P_j != 0:
 *      Q_e[p] = Q_e[p] + g * P_j, p = W_e[j] (distinct pairs: the order does not matter);
 *   6. if d the window is emptied; else every entry ages by one (W_e[j+1] = W_e[j], j = K-2 .. 0; W_e[0] = -1; age K-1 drops out);
 *   7. the next iteration chooses from the table after this iteration's updates (a wall bump and window pairs in the row of s'
 *      included).
 * With K = 1 (any lambda) or lambda = 0 (any K) this is gu_td_run, byte for byte: method 0 is Q-learning, 1 is SARSA.
 * CARRY: the window and SARSA's a' persist from one gu_lambda_run to the next when the later call directly follows the earlier one
 * with the same method and K (alpha, gamma and lambda may change: the ages carry, the new c applies).  Any other call in between --
 * everything that ends gu_td_run's SARSA carry, gu_td_run, gu_dyna_run, gu_sweep_run, gu_nstep_run, gu_ac_run, gu_search_run, a gu_lambda_run with another
 * method or K -- drops both.  gu_lambda_run ends gu_td_run's SARSA carry and gu_nstep_run's window.
 * gu_lambda_run        : T iterations per env in ONE launch (async).  method 0 = Watkins's Q(lambda), 1 = SARSA(lambda); 1 <= K
 *                        <= GU_LAMBDA_MAX; 0 <= lambda <= 1.  GU_ERR_STATE before gu_td_init; GU_ERR_INVALID for a bad method,
 *                        K or lambda (NaN included) and everything gu_td_run rejects.  The window storage (N * 256 bytes) is
 *                        allocated on first use (GU_ERR_NOMEM under gu_td_init's free-memory rule); a grid of another size drops
 *                        it with the tables.  T = 0 changes nothing.  Flags, rows and statistics as gu_td_run.  The step counts
 *                        advance by T.
 * gu_lambda_get_window : the windows of envs env0 .. env0+n-1 on the host as sa[n][GU_LAMBDA_MAX], index = age; -1 everywhere once
 *                        the window has been dropped. */
#define GU_LAMBDA_MAX 64
int gu_lambda_run(gu_handle h, int64_t T, int32_t method, int32_t K, double alpha, double gamma, double lambda, uint32_t eps_q16,
                  uint32_t flags);
int gu_lambda_get_window(gu_handle h, int64_t env0, int64_t n, int32_t *sa);

/* ---- batched tabular one-step actor-critic with a softmax policy: learner e owns env e, preferences H_e[S][4] and values V_e[S] ----
 * (build-defined: the reference lists "Policy Gradients (MC Policy Gradients and Actor-critic)" on its roadmap and ships no code;
 * Sutton & Barto 13.5; tests/_ac_oracle.py is the CPU restatement.)  The tables are float64 and the learner's own, not the
 * gu_td_* Q tables.  All arithmetic is float64 with one rounding per operation (multiply, add, subtract, divide).
 * THE BUILD'S EXP, gu_exp(x) for x <= 0 (NaN: unspecified):
 *   x < -700: 0.0, and so gu_exp(-inf) = 0.0 -- finite preferences can produce it: -1e308 - 1e308 in rule 2.  Otherwise k = rint(x * 1.4426950408889634) (half to even);
 *   r = (x - k * 6.93147180369123816490e-01) - k * 1.90821492927058770002e-10;
 *   p = 1/13!, then p = p * r + c for c = 1/12!, 1/11!, ..., 1/2!, 1, 1 in that order (multiply and add rounded separately;
 *   each 1/n! is the double nearest to it); result = ldexp(p, k) (k >= -1010 here, so the result is normal and exact).
 * One iteration of gu_ac_run for env e at 64-bit step count t:
 *   1. reset: lazy auto-reset, exactly as rule 1 of gu_td_run;
 *   2. policy: h = H_e[s], m = its maximum folded left to right with `>`; e_b = gu_exp(h_b - m); Z = ((e_0 + e_1) + e_2) + e_3;
 *      iz = 1 / Z; pi_b = e_b * iz;
 *   3. action: w = the stream-4 word at t (as rule 2 of gu_td_run); x = (w * 2^-32) * Z; a = the first b with x < c_b,
 *      c_0 = e_0, c_b = c_{b-1} + e_b, c_3 = Z; 3 if none.  No epsilon: the softmax explores;
 *   4. (s', r, d) by the engine's move rule (absorbing terminal); t += 1;
 *   5. TD error: delta = (r + gamma * V_e[s']) - V_e[s], V_e[s'] read before this iteration's writes; delta = r - V_e[s] when d
 *      (H_e[s'] and V_e[s'] are not read then);
 *   6. critic: V_e[s] = V_e[s] + alpha_critic * delta;
 *   7. actor: g = alpha_actor * delta; H_e[s][b] = H_e[s][b] + g * ([b == a] - pi_b) for b = 0..3.  There is no gamma^t factor
 *      ("I" of the textbook's pseudo-code): a deliberate choice, the common form of the continuing, auto-resetting learner;
 *   8. the next iteration sees the updated row and value (a wall bump, s' == s, included).
 * gu_ac_run ends gu_td_run's SARSA carry and gu_nstep_run's window and has no carry of its own.
 * gu_ac_init : allocate both tables (N * S * 40 bytes; GU_ERR_NOMEM under gu_td_init's free-memory rule) and fill every
 *              preference with h0 and every value with v0; GU_ERR_INVALID for a non-finite h0 or v0.  A grid of another size
 *              drops the tables (gu_ac_init again).  gu_td_init and gu_td_set_q leave them alone.
 * gu_ac_run  : T iterations per env in ONE launch (async).  GU_ERR_STATE before gu_ac_init; GU_ERR_INVALID for non-finite rates
 *              or gamma, T < 0 or T > 1e8, flags other than GU_F_TRAJECTORY | GU_F_STATS.  Rows, statistics, the trajectory
 *              reservation and the agent trail as gu_td_run.  T = 0 changes nothing.  The step counts advance by T.
 * gu_ac_get / gu_ac_set : the tables of envs env0 .. env0+n-1 on the host, pref as [n][S][4] and v as [n][S]; either pointer
 *              may be NULL, not both.  gu_ac_set rejects non-finite entries (GU_ERR_INVALID) before it writes anything. */
int gu_ac_init(gu_handle h, double h0, double v0);
int gu_ac_run(gu_handle h, int64_t T, double alpha_actor, double alpha_critic, double gamma, uint32_t flags);
int gu_ac_get(gu_handle h, int64_t env0, int64_t n, double *pref, double *v);
int gu_ac_set(gu_handle h, int64_t env0, int64_t n, const double *pref, const double *v);

/* ---- batched tabular REINFORCE with baseline (Monte-Carlo policy gradient): learner e owns env e and the gu_ac_* tables ----
 * (build-defined: the first half of the reference's roadmap entry "Policy Gradients (MC Policy Gradients and Actor-critic)", for
 * which it ships no code; Sutton & Barto 13.3/13.4; tests/_reinforce_oracle.py is the CPU restatement.)  The preferences H_e are
 * the actor, the values V_e the baseline.  Learner e also keeps an EPISODE BUFFER E_e: the transitions (s_k, a_k, r_k) of its
 * current segment, oldest first, at most L-1 of them between iterations.  All arithmetic is float64 with one rounding per
 * operation; gu_exp and the softmax exactly as rule 2 of gu_ac_run.
 * One iteration of gu_reinforce_run for env e at 64-bit step count t:
 *   1. reset: lazy auto-reset, exactly as rule 1 of gu_td_run (the buffer is empty here: see 5);
 *   2. policy and action: rules 2 and 3 of gu_ac_run on H_e[s] as it is now (the stream-4 word at t).  The tables change only in
 *      rule 5, so inside a segment the policy is fixed;
 *   3. (s', r, d) by the engine's move rule (absorbing terminal); t += 1; append (s, a, r) to E_e;
 *   4. if not d and E_e holds fewer than L entries: the iteration ends here;
 *   5. segment end (d, or E_e holds L entries): G = 0.0 if d, else V_e[s'] read before any write of this pass (a truncated
 *      segment bootstraps on the baseline; the env is NOT reset and goes on from s').  Then for every entry, newest to oldest:
 *        G = r_k + gamma * G; delta = G - V_e[s_k]; V_e[s_k] = V_e[s_k] + alpha_baseline * delta;
 *        pi = the softmax (rule 2 of gu_ac_run) of H_e[s_k] as it is now -- earlier updates of this pass included: a repeated
 *        state compounds; g = alpha_actor * delta; H_e[s_k][b] = H_e[s_k][b] + g * ([b == a_k] - pi_b) for b = 0..3.
 *      There is no gamma^k factor, as in rule 7 of gu_ac_run.  E_e ends empty;
 *   6. the next iteration sees the tables after the pass.
 * With alpha_baseline = 0 and V = 0 this is plain REINFORCE.  With L = 1 it is gu_ac_run, byte for byte.
 * CARRY: the buffer persists from one gu_reinforce_run to the next when the later call directly follows the earlier one with the
 * same L (the rates and gamma may change).  Any other call in between -- everything that drops gu_lambda_run's window, and
 * gu_td_run, gu_dyna_run, gu_sweep_run, gu_nstep_run, gu_lambda_run, gu_ac_run, gu_search_run, gu_ac_init, gu_ac_set, a gu_reinforce_run with another L --
 * drops it: the pending transitions are discarded, not learned from.  gu_reinforce_run ends gu_td_run's SARSA carry and the
 * windows of gu_nstep_run and gu_lambda_run.
 * gu_reinforce_run         : T iterations per env in ONE launch (async).  1 <= L <= GU_REINFORCE_MAX.  GU_ERR_STATE before
 *                            gu_ac_init; GU_ERR_INVALID for a bad L, non-finite rates or gamma, T < 0 or T > 1e8, flags other
 *                            than GU_F_TRAJECTORY | GU_F_STATS.  The buffer storage (N * (8 L + 4) bytes) is allocated on first
 *                            use for the L of the call, and again for a larger one (GU_ERR_NOMEM under gu_td_init's free-memory
 *                            rule); a grid of another size drops it with the tables.  T = 0 changes nothing.  Rows, statistics,
 *                            the trajectory reservation and the agent trail as gu_ac_run: the T real steps only.  The step
 *                            counts advance by T.
 * gu_reinforce_get_episode : the buffers of envs env0 .. env0+n-1 on the host: sa (s*4+a) and reward as [n][GU_REINFORCE_MAX],
 *                            oldest first, (-1, 0) beyond count; count as [n], 0 when the buffer has been dropped.  Any pointer
 *                            may be NULL. */
#define GU_REINFORCE_MAX 1024
int gu_reinforce_run(gu_handle h, int64_t T, int32_t L, double alpha_actor, double alpha_baseline, double gamma, uint32_t flags);
int gu_reinforce_get_episode(gu_handle h, int64_t env0, int64_t n, int32_t *sa, int32_t *reward, int32_t *count);

/* ---- batched off-policy Monte-Carlo control with weighted importance sampling: learner e owns env e and its table Q_e[S][4] ----
 * (build-defined: the second half of the reference's roadmap entry "Off-policy control (Q-Learning, Importance Sampling)", for
 * which it ships no code -- gu_td_run is the first half; Sutton & Barto 5.7, every-visit, WEIGHTED importance sampling;
 * tests/_is_oracle.py is the CPU restatement.)  The target policy is greedy on Q_e with ties shared equally, the behaviour policy is
 * gu_td_run's epsilon-greedy on the same table.  Learner e owns env e, its gu_td_* table Q_e[S][4], a float64 table C_e[S][4] of
 * CUMULATIVE WEIGHTS, initially 0, and an EPISODE BUFFER E_e: the entries (s_k, a_k, r_k, c_k) of its current segment, oldest
 * first, at most L-1 of them between iterations.  All arithmetic is float64 with one rounding per operation and no contraction.
 * THE RATIO TABLE R[m][c], m = 1..4, c = 0..4: pi(a|s) / b(a|s) for an action that is one of m maxima of its row now and was, when
 * it was taken, one of c maxima (c = 0: none of them).  Computed on the host from eps_q16: eps = eps_q16 / 65536.0;
 * b_0 = eps * 0.25; b_c = (1.0 - eps) / c + eps * 0.25; R[m][c] = (1.0 / m) / b_c, and 0.0 where b_c == 0 (only c = 0 at epsilon 0,
 * a class that cannot occur).  The kernel holds these 20 doubles and computes no division for the ratio.  The tie rule's
 * (x * m) >> 14 is exactly uniform only for m = 1, 2, 4: for m = 3 the three actions have probabilities 5462, 5461, 5461 / 16384,
 * and the ratios are the nominal ones.
 * RECIP(x), the correctly rounded 1 / x of a positive normal x: x = f * 2^p with f in [1, 2); the build's correctly rounded
 * reciprocal of f (csrc/gu_softmax.hpp, gu_recip14) scaled by 2^-p, which is exact.  The restatement writes 1.0 / x.
 * One iteration of gu_is_run for env e at 64-bit step count t:
 *   1. reset: lazy auto-reset, exactly as rule 1 of gu_td_run (the buffer is empty here: see 5);
 *   2. behaviour action: rule 2 of gu_td_run unchanged (the stream-4 word at t, epsilon-greedy on Q_e[s] with its tie rule; no
 *      other RNG stream).  Its CLASS c: m, the number of entries of Q_e[s] equal to the row maximum (folded left to right with
 *      `>`), if Q_e[s][a] equals that maximum -- an exploring draw that happens to be greedy included --, else 0;
 *   3. (s', r, d) by the engine's move rule (absorbing terminal); t += 1; append (s, a, r, c) to E_e;
 *   4. if not d and E_e holds fewer than L entries: the iteration ends here;
 *   5. segment end (d, or E_e holds L entries): G = 0.0 if d, else max Q_e[s'], folded left to right with `>` and read before any
 *      write of this pass (a truncated segment bootstraps; the env is NOT reset and goes on from s').  W = 1.0.  Then for every
 *      entry, newest to oldest, in this order:
 *        G = r_k + gamma * G;
 *        C_e[s_k][a_k] = C_e[s_k][a_k] + W;
 *        Q_e[s_k][a_k] = Q_e[s_k][a_k] + (W * RECIP(C_e[s_k][a_k])) * (G - Q_e[s_k][a_k]);
 *        with the row Q_e[s_k] as it is now: if Q_e[s_k][a_k] is not equal to the row maximum, the pass ends and the older
 *        entries are discarded unlearned (the target policy would not have taken a_k: their weight is 0);
 *        otherwise W = W * R[m_now][c_k], m_now the number of maxima of the row now;
 *        if not 2^-256 <= W < w_cap, the pass ends likewise.
 *      E_e ends empty;
 *   6. the next iteration sees the tables after the pass.
 * W stays inside [2^-256, w_cap) wherever it is added to C, so a nonzero entry of C that the learner made lies in
 * [2^-256, 2^320) and RECIP never sees a subnormal, zero or infinity (entries installed by gu_is_set above 2^320 are outside that
 * guarantee).  w_cap, 1 <= w_cap <= 2^256, is also the knob of "truncated importance sampling": a small value ends passes early.
 * Ordinary (unweighted) importance sampling is not offered: its estimates overflow.  With L long and few greedy actions the learner
 * learns from the tails of its episodes only: on large open grids it is slower than gu_td_run (the textbook weakness).
 * CARRY: as gu_reinforce_run's.  The buffer persists from one gu_is_run to the next when the later call directly follows the
 * earlier one with the same L (gamma, epsilon and w_cap may change).  Any other call in between -- everything that drops
 * gu_reinforce_run's buffer, gu_reinforce_run itself, gu_is_init, gu_is_set, a gu_is_run with another L -- drops it: the pending
 * transitions are discarded, not learned from; and gu_is_run drops gu_reinforce_run's buffer, ends gu_td_run's SARSA carry and the
 * windows of gu_nstep_run and gu_lambda_run.  C_e lives until gu_is_init or a grid of another size; gu_td_init and gu_td_set_q
 * leave it alone (new Q tables under old weights learn slowly: call gu_is_init too).
 * gu_is_init        : allocate the cumulative weights (N * S * 32 bytes; GU_ERR_NOMEM under gu_td_init's free-memory rule) and set
 *                     them to 0.  GU_ERR_STATE before gu_td_init.
 * gu_is_run         : T iterations per env in ONE launch (async).  1 <= L <= GU_IS_MAX.  GU_ERR_STATE before gu_td_init or
 *                     gu_is_init; GU_ERR_INVALID for a bad L, w_cap outside [1, 2^256] (NaN included), eps_q16 above 65536, a
 *                     non-finite gamma, T < 0 or T > 1e8, flags other than GU_F_TRAJECTORY | GU_F_STATS.  The buffer storage
 *                     (N * (8 L + 4) bytes) is allocated on first use for the L of the call, and again for a larger one
 *                     (GU_ERR_NOMEM as above); a grid of another size drops it with the weights.  T = 0 changes nothing.  Rows,
 *                     statistics, the trajectory reservation and the agent trail as gu_td_run: the T real steps only.  The step
 *                     counts advance by T.
 * gu_is_get / gu_is_set : the cumulative weights of envs env0 .. env0+n-1 as c[n][S][4] on the host; set rejects a negative or
 *                     non-finite entry (GU_ERR_INVALID) before it writes anything.
 * gu_is_get_episode : the buffers of envs env0 .. env0+n-1 on the host: sa (s*4+a), reward and cls as [n][GU_IS_MAX], oldest
 *                     first, (-1, 0, 0) beyond count; count as [n], 0 when the buffer has been dropped.  Any pointer may be NULL. */
#define GU_IS_MAX 1024
int gu_is_init(gu_handle h);
int gu_is_run(gu_handle h, int64_t T, int32_t L, double gamma, uint32_t eps_q16, double w_cap, uint32_t flags);
int gu_is_get(gu_handle h, int64_t env0, int64_t n, double *c);
int gu_is_set(gu_handle h, int64_t env0, int64_t n, const double *c);
int gu_is_get_episode(gu_handle h, int64_t env0, int64_t n, int32_t *sa, int32_t *reward, int32_t *cls, int32_t *count);

/* ---- batched semi-gradient SARSA and Q-learning on binary features: learner e owns env e and a weight table w_e[F][4] ----
 * (build-defined: the reference's roadmap entry "Value Approximation", for which it ships no code; Sutton & Barto 10.1;
 * tests/_fa_oracle.py is the CPU restatement.)  The action values are computed, not stored.  The engine holds ONE feature table
 * phi[S][K] (int32, 0 <= phi < F, 1 <= K <= GU_FA_MAX_K) shared by all envs: it depends on the state index only, so it also serves
 * one-grid-per-env batches, whose grids share W x H.  Column k is a slot (a tiling of tile coding): no feature index occurs in two
 * columns; one index many times in one column is aggregation.
 *   Q_e(s)[b] = w_e[phi[s][0]][b], then + w_e[phi[s][k]][b] for k = 1 .. K-1 in this order, one rounded add each.
 * One iteration of gu_fa_run for env e at 64-bit step count t:
 *   1. lazy auto-reset, exactly as rule 1 of gu_td_run;
 *   2. action: rule 2 of gu_td_run (the stream-4 word at t, eps_q16, the tie rule) applied to the row Q_e(s).  SARSA takes its
 *      carried a' instead, under the conditions of gu_td_run's SARSA (the carry across launches is gu_fa_run's own, below);
 *   3. (s', r, d) by the engine's move rule (absorbing terminal); t += 1;
 *   4. n = Q_e(s') from the weights as they are before this step's update; m = max n, folded with `>` as in gu_td_run (method 0,
 *      Q-learning) or n[a'] with a' drawn at s' by rule 2 from the word of the new t (method 1, SARSA; not drawn when d);
 *      target = r if d else r + gamma * m; g = alpha * (target - Q_e(s)[a]); then for k = 0 .. K-1:
 *      w_e[phi[s][k]][a] = w_e[phi[s][k]][a] + g.
 * All float64, one rounding per operation, multiply / add / subtract only.  alpha is applied as given: dividing a step size by K
 * is the caller's business.  With K = 1, F = S, phi[s][0] = s this is gu_td_run byte for byte, both methods, across launches.
 * CARRY: SARSA's a' survives from one gu_fa_run to the next under the conditions of gu_td_run's carry; gu_fa_init, gu_fa_set_w and
 * a run of any other learner end it as well, and gu_fa_run ends every other learner's carry, window and episode buffer.  A SARSA
 * gu_td_run does not hand its action to gu_fa_run, nor the other way round.
 * gu_fa_init  : copy phi, allocate the weights (N * F * 32 bytes; GU_ERR_NOMEM under gu_td_init's free-memory rule) and set every
 *               entry to w0.  GU_ERR_INVALID for K outside 1 .. GU_FA_MAX_K, F outside 1 .. GU_FA_MAX_F, an index outside [0, F), an index that occurs
 *               in two columns, a non-finite w0.  The weights are separate from the gu_td_* tables; both may exist.  A grid of
 *               another size drops features and weights (gu_fa_init again).
 * gu_fa_run   : T iterations per env in ONE launch (async).  method 0 = Q-learning, 1 = SARSA.  Flags, rows, statistics, the
 *               agent trail, T = 0, the argument checks and the step counts as gu_td_run.  GU_ERR_STATE before gu_fa_init.
 * gu_fa_get_w / gu_fa_set_w : weights of envs env0 .. env0+n-1 as w[n][F][4] on the host.
 * gu_fa_get_q : their action values q[n][S][4], folded on the device by the rule above. */
#define GU_FA_MAX_K 8
#define GU_FA_MAX_F (1 << 26) /* 2 GiB of weights per learner */
int gu_fa_init(gu_handle h, int32_t K, int32_t F, const int32_t *phi, double w0);
int gu_fa_run(gu_handle h, int64_t T, int32_t method, double alpha, double gamma, uint32_t eps_q16, uint32_t flags);
int gu_fa_get_w(gu_handle h, int64_t env0, int64_t n, double *w);
int gu_fa_set_w(gu_handle h, int64_t env0, int64_t n, const double *w);
int gu_fa_get_q(gu_handle h, int64_t env0, int64_t n, double *q);

/* ---- look_step_ahead table queries: env:136-155 for n (state, action) pairs (grid 0 of a multi-grid engine) ---- */
int gu_look_step_ahead(gu_handle h, int64_t n, const int32_t *states, const int32_t *actions,
                       int32_t care_about_terminal, int32_t *next, int32_t *reward, int32_t *done);

/* ---- tabular DP on the engine's grid (float64, bit-exact, no FMA contraction) ----
 * gu_vi_set   : upload v[S] and pi[S][4]                (dynamic_programming.py:12-13)
 * gu_vi_sweep : `iters` x { V1 policy-evaluation sweep  core/algorithms/utils.py:15-27;
 *               optionally V2 greedy improvement        core/algorithms/utils.py:55-72 }
 *               deltas[i] = max(v - v') of sweep i      dynamic_programming.py:17 (may be NULL)
 * gu_vi_run   : the whole value_iteration loop (dynamic_programming.py:14-27) queued in one call: up to
 *               max_steps rounds {V1, delta, V2}; the stopping rule `delta < threshold` is evaluated ON THE
 *               DEVICE after each round and turns the launches queued behind it into no-ops, so the host
 *               synchronises once.  steps_done = rounds executed; deltas[0..steps_done) optional.
 * gu_vi_eval_run : policy_iteration's evaluation loop (dynamic_programming.py:40-42): V1 sweeps with the policy
 *               fixed until `delta < threshold` or max_steps sweeps; steps_done / deltas as for gu_vi_run.
 *               (Grids of up to 4096 states run gu_vi_run / gu_vi_eval_run / gu_vi_sweep as ONE launch of one
 *               workgroup with v in LDS; larger grids take one launch per round.)
 * gu_vi_greedy: V2 alone on the current v (policy improvement without an evaluation sweep)
 * gu_vi_get   : download v / pi (either may be NULL).  Behind a gu_vi_run / gu_vi_sweep / gu_vi_eval_run that ran as the one
 *               launch of one XCD's workgroups this is two memcpys: that launch leaves its final tables in a page-locked copy
 *               on the host, valid until the next call that may write a table.
 * gu_vi_sweep_step : config 5 -- ONE launch that performs one V1+V2 sweep AND one env
 *               step in which every agent acts greedily on the updated policy.
 * gu_vi_sweep_step_run : `iters` such rounds.  Three forms, fastest first: (1) ONE launch synchronised per XCD -- every XCD
 *               sweeps the whole table with its own workgroups and steps its share of the agents, nothing a round needs
 *               leaves the XCD's L2 (table + planes within one workgroup's LDS, one workgroup per CU at most); (2) ONE launch
 *               of a workgroup cluster with a chip-wide barrier per round (max(S, N) <= 1024 x the device's CUs,
 *               S <= 32 767); (3) one launch per round.  A form that cannot hold its workgroups resident together gives up
 *               (bounded spins), the state is put back, the next form runs.  deltas[iters] optional.
 * gu_vi_last_form : which of the three the last gu_vi_sweep_step_run of this engine took (1, 2, 3; 0 = none yet).
 * gu_vi_last_clusters : members[8] = how many workgroups of its last per-XCD launch read each HW_REG_XCC_ID (the clusters as the
 *               hardware reported them; equal under the round-robin placement observed on MI355X -- speed only, any split is correct). */
int gu_vi_set(gu_handle h, const double *v, const double *pi);
int gu_vi_sweep(gu_handle h, double gamma, int32_t iters, int32_t greedy_update, double *deltas);
int gu_vi_run(gu_handle h, double gamma, double threshold, int32_t max_steps, int32_t *steps_done, double *deltas);
int gu_vi_eval_run(gu_handle h, double gamma, double threshold, int32_t max_steps, int32_t *steps_done, double *deltas);
int gu_vi_greedy(gu_handle h, double gamma);
int gu_vi_get(gu_handle h, double *v, double *pi);
int gu_vi_sweep_step(gu_handle h, double gamma, uint32_t flags, double *delta);
int gu_vi_sweep_step_run(gu_handle h, double gamma, int32_t iters, uint32_t flags, double *deltas);

/* ---- Monte-Carlo policy evaluation: core/algorithms/monte_carlo.py:29-99 ----------------
 * Consumes the trajectory rows 0..T-1 of the last gu_rollout (run WITHOUT auto-reset: env e is
 * episode e; its episode ends at its first done row, or after T steps -- run_episode, :7-26) and
 * applies the reference's arithmetic in the reference's order (episode 0, 1, ... N-1):
 *   per episode  : visit counts and summed returns per state, first-visit or every-visit (:54-71);
 *                  return from step idx = sum_i discount_pow[i] * r[idx+i] over the i with keep[i]
 *                  (the caller passes discount_factor**i and (discount_factor**i > threshold) so
 *                  that pow is evaluated by the host language exactly like the reference, :69-70)
 *   across episodes, per state: incremental mean / running mean with alpha / batch mean (:73-97)
 * first_state[N]: the state each episode started in (what reset() returned).  value[S] in/out is
 * NOT read: evaluation starts from zeros like the reference; value_out[S] and visits_out[S]
 * (total_visit_counter, optional) are written.  float64, bit-exact. */
int gu_mc_evaluate(gu_handle h, int64_t T, const int32_t *first_state, int32_t every_visit, int32_t incremental_mean,
                   int32_t stationary_env, double alpha, const double *discount_pow, const uint8_t *keep,
                   double *value_out, double *visits_out);
/* The REFERENCE'S OWN episodes for gu_mc_evaluate: run_episode (core/algorithms/monte_carlo.py:7-26) draws one
 * np.random.choice(4, p=policy[obs]) -- one uniform of numpy's global stream -- per step, episode after episode.  The host
 * pre-draws the uniforms u[K] in bulk; the episode that begins at uniform i in start cell c is a pure function of (i, c), so
 *   gu_mc_walk_lengths  walks it for EVERY offset i < n_offsets and every start cell start_states[n_starts], one lane each:
 *                       lengths[c][i] = steps until done or `cap` (run_episode's max_steps_per_episode; 0xFFFF: the uniforms ran
 *                       out first); cdf[S][4] = the rows np.random.choice builds (p.cumsum() / p.sum()).  The caller follows the chain
 *                       offset -> offset + length through the table, one look-up per episode;
 *   gu_mc_walk_episodes walks episode e (env e of the engine) from uniform offsets[e] and cell first_state[e] and writes its
 *                       (obs, reward, done) rows 0 .. T-1 into the trajectory buffer (rows past its end: the absorbing state, as a
 *                       rollout without auto-reset leaves them), for gu_mc_evaluate.  The engine's env state is not touched. */
int gu_mc_walk_lengths(gu_handle h, int64_t K, const double *u, int64_t n_offsets, int32_t n_starts, const int32_t *start_states,
                       int32_t cap, const double *cdf, uint16_t *lengths);
int gu_mc_walk_episodes(gu_handle h, int64_t K, const double *u, const double *cdf, const int64_t *offsets, const int32_t *first_state,
                        int32_t cap, int64_t T);

/* ---- shortest paths: the breadth-first search of core/algorithms/maze_solving.py:43-50, 123-193 for EVERY grid ----
 * One lane per grid searches from the grid's first start cell over the care_about_terminal=False move graph
 * (children in action order, FIFO), stops at the first terminal state (goal or lava) it dequeues and writes the
 * action list.  path[n_grids][max_path] int8, path_len[n_grids] (-1 no terminal reachable, -2 longer than
 * max_path), terminal[n_grids] (optional) the state reached. */
int gu_shortest_paths(gu_handle h, int32_t max_path, int8_t *path, int32_t *path_len, int32_t *terminal);

/* ---- headless RGB frames (stands in for the pyglet window of core/envs/rendering.py:236-343) -----------------
 * rgb[n_envs][H*cell_px][W*cell_px][3] uint8 for envs env0 .. env0+n_envs-1: ground / wall / goal / lava tiles -- which of
 * the four a cell gets follows the viewer's rule (rendering.py:119-133: goal, else lava, else wall, else ground); the flat
 * colours that stand in for its textures are build-defined -- a grid line on the top and left edge of each cell
 * (cell_px >= 4), the agent as an inset square on its cell. */
int gu_render_rgb(gu_handle h, int64_t env0, int64_t n_envs, int32_t cell_px, uint8_t *rgb);
/* The agent trail: core/envs/griduniverse_env.py:92-93, 182-184, 190 (`last_n_states`: the cell the agent is on after every
 * step, newest 500 kept, emptied by reset) + core/envs/rendering.py:287-311 (every frame: newest first, a quad over the entry's
 * tile with alpha 0.3 * 0.96^(i + 1), entries on the agent's current cell skipped).  OFF by default; gu_trail_enable(capacity
 * 1 .. 500; 0 = off again) makes the step / reset / rollout launches keep a ring per env -- small kernels of their own behind the
 * launch; a rollout must then write rows (GU_F_TRAJECTORY or GU_F_PACKED), the fused sweep + step launches are refused --
 * and gu_render_rgb blend it over the tiles: corner colours red, yellow, green, blue (bottom-left, counter-clockwise) interpolated
 * bilinearly at the pixel centre, c = (c * (65536 - A) + colour * A + 32768) >> 16 per entry with A = round(alpha * 65536).
 * gu_trail_read: cells[n_envs][capacity] oldest first (-1 beyond length[k]), like the reference's list of states. */
int gu_trail_enable(gu_handle h, int32_t capacity);
int gu_trail_read(gu_handle h, int64_t env0, int64_t n_envs, int32_t *cells, int32_t *length);
/* The policy-arrow figure of Viewer.render_policy_arrows (core/envs/rendering.py:159-212) for the current policy table
 * (gu_vi_set / gu_vi_run ...): rgb[H*cell_px][W*cell_px][3], the tiles of grid 0 plus, on every state that is neither
 * terminal nor a wall, one arrow per action with probability >= 0.1: shaft from the tile centre, round(p*20) long
 * (half to even), head a triangle of half-width 5 and height 5 on its end, on the reference's 52-pixel tile.
 * Rasterisation (the reference leaves it to OpenGL): coordinates scale by cell_px / 52 about the tile centre; a pixel is
 * painted when its centre lies within max(1, cell_px / 26) / 2 of the shaft segment, or inside the head triangle (edges
 * included, the base edge excluded).  Probabilities are expected in [0, 1] (an arrow never leaves its tile then). */
int gu_render_policy_rgb(gu_handle h, int32_t cell_px, uint8_t *rgb);

/* ---- agent sensors: what every env SEES, as small uint8 views ------------------------------------------------
 * The reference ships no sensor; its roadmap asks for "different sensor configurations for the agent so it can be defined
 * whether the agent field of view is constrained to the current state, surrounding states or the complete grid".  The rule
 * is build-defined:
 *   class of a cell: the viewer's tile rule (core/envs/rendering.py:119-133, pinned by tests/golden/arrows.json "tiles"):
 *     goal -> 3, else lava -> 2, else wall -> 1, else ground -> 0 (so goal+lava and goal+wall are goal, lava+wall is lava);
 *     a cell outside the grid has class 4.  Device-generated mazes: the class follows from the cell's flags.
 *   GU_SENSE_EGO, radius r in 0 .. GU_SENSE_MAX_R, K = 2r + 1: for an agent on cell s = y*W + x,
 *     view[dy][dx] = class of cell (y + dy - r, x + dx - r), 4 where that lies outside the grid; r = 0 is the class of the
 *     agent's own cell.  The agent is always at the centre and is not marked.
 *   GU_SENSE_GRID: view[y][x] = class of cell y*W + x, plus 8 on the agent's cell; H x W, the radius is ignored.
 * gu_sense: the position is the env's current one (under lazy auto-reset a finished env still stands on its terminal cell);
 *   view[n][K][K] or [n][H][W] for envs env0 .. env0+n-1.
 * gu_sense_trajectory: the position is the obs value of the row and env; view[T][N][K][K] or [T][N][H][W] for rows t0 .. t0+T-1
 *   of the trajectory buffer, in either int32 layout (GU_OPT_TRAJ_LAYOUT).
 * view == NULL: the kernel runs into the engine's scratch memory and nothing is copied (timing: gu_timer_begin / gu_timer_end).
 * GU_ERR_STATE: no grid; rows not in the trajectory buffer or nothing written there yet; a packed buffer (GU_F_PACKED).
 * GU_ERR_INVALID: unknown mode; radius outside 0 .. GU_SENSE_MAX_R in GU_SENSE_EGO; env range outside the batch; more than 2^32
 *   bytes of views in one call.  Neither call touches env state, RNG streams, what the learners carry from launch to launch,
 *   their windows and buffers, or the trajectory buffer. */
#define GU_SENSE_EGO 0
#define GU_SENSE_GRID 1
#define GU_SENSE_MAX_R 7
int gu_sense(gu_handle h, int64_t env0, int64_t n, int32_t mode, int32_t radius, uint8_t *view);
int gu_sense_trajectory(gu_handle h, int64_t t0, int64_t T, int32_t mode, int32_t radius, uint8_t *view);

/* ---- page-locked host memory -----------------------------------------------------
 * Buffers from gu_host_alloc make gu_step (with GU_F_PINNED_IO), gu_read_outputs and gu_read_trajectory copy at
 * the full PCIe rate; numpy arrays can be built on them (np.ctypeslib / np.frombuffer). */
int gu_host_alloc(size_t bytes, void **ptr);
int gu_host_free(void *ptr);

/* ---- stream ---------------------------------------------------------------------
 * (HIP-event timers on the handle's own stream -- torch.cuda.Event cannot see it --: gu_timer_*, include/gu_diag.h.) */
int gu_sync(gu_handle h);

/* ---- multi-GPU gathered view (RCCL over xGMI) ----------------------------------
 * One process per GPU.  Rank 0 calls gu_comm_unique_id and ships the 128 bytes to
 * the other ranks by any host channel; every rank then calls gu_comm_init.  The
 * data path (step / rollout) never communicates; only gu_allgather_view does:
 * one ncclAllGather of the packed int32[3N] (obs|reward|done) block per rank, then
 * a D2H copy into three host arrays of nranks*N.  All ranks must hold the same N. */
#define GU_COMM_ID_BYTES 128
int gu_comm_unique_id(uint8_t id[GU_COMM_ID_BYTES]);
int gu_comm_init(gu_handle h, int32_t nranks, int32_t rank, const uint8_t id[GU_COMM_ID_BYTES]);
int gu_comm_destroy(gu_handle h);
int gu_allgather_view(gu_handle h, int32_t *obs_all, int32_t *reward_all, int32_t *done_all);
/* The same for ONE process that holds one handle per device (handles[i] on a distinct device, equal N):
 * ncclCommInitAll, then one grouped ncclAllGather; the view is copied out of handles[0]'s device. */
int gu_comm_init_all(gu_handle *handles, int32_t n);
int gu_allgather_view_all(gu_handle *handles, int32_t n, int32_t *obs_all, int32_t *reward_all, int32_t *done_all);

#ifdef __cplusplus
}
#endif
#endif /* GU_H */
