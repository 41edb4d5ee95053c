/*
 * ctf_env.h — C ABI of the batched GridworldCtf hot path on MI355X (gfx950).
 *
 * This header is the drop-in boundary.  The reference (g-nightingale/marl-ctf-development) is
 * pure Python and has no FFI of its own: its boundary is the class `GridworldCtf`
 * (gridworld_ctf.py:13).  Every entry point below names the reference method(s) whose work it
 * replaces; the Python facade in `marl-ctf-development_amd/gridworld_ctf.py` binds them with
 * ctypes (see INTEGRATION.md for the stub a reference maintainer would add).
 *
 * Conventions
 *   - plain C, plain pointers and sizes; no torch / C++ types cross this ABI;
 *   - every `*_dev` pointer is a caller-owned DEVICE pointer (e.g. torch tensor .data_ptr());
 *     the library never allocates or frees I/O buffers;
 *   - `stream` is a `hipStream_t` passed as `void*` (NULL = the null stream); calls that take a
 *     stream only enqueue work on it and return;
 *   - ctf_step, ctf_observe, ctf_observe_codes, ctf_step_observe, ctf_reset, ctf_harvest_episodes, ctf_harvest_visitation,
 *     ctf_export_visitation, ctf_export_states, ctf_import_states, ctf_scripted_actions, ctf_scripted_roles, ctf_scripted_abilities, ctf_scripted_costs, ctf_action_effects, ctf_random_effective_actions and ctf_reset_scattered are kernel launches and nothing else (no
 *     allocation, no copy, no synchronisation, no host-side state that moves from call to call), so a caller may capture them
 *     into a hipGraph on `stream` and replay it: every replay is the next step (tests/test_gpu_hipgraph.py);
 *   - return value 0 = OK, negative = error (see CTF_E_*); `ctf_last_error()` has the text;
 *   - a handle is not thread-safe; distinct handles are independent (one per GPU / shard).
 */
#ifndef CTF_ENV_H
#define CTF_ENV_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CTF_ABI_VERSION 2

#define CTF_MAX_AGENTS 16   /* N  <= 16                                   */
#define CTF_MAX_GRID 32     /* G  <= 32 (G*G <= 1024 cells)               */
#define CTF_MAX_CELLS (CTF_MAX_GRID * CTF_MAX_GRID)
#define CTF_MAX_CHANNELS 16 /* C  <= 16 (tiles 1..13 + own-position plane) */
#define CTF_N_ACTIONS 9     /* gridworld_ctf.py:100-145: actions 0..8      */
#define CTF_N_METRICS 13    /* per-agent counters, gridworld_ctf.py:456-468 */
#define CTF_MT_N 624        /* MT19937 state words                         */

/* error codes */
#define CTF_OK 0
#define CTF_E_INVALID (-1) /* bad argument / config                        */
#define CTF_E_HIP (-2)     /* a HIP runtime call failed                    */
#define CTF_E_NOMEM (-3)
#define CTF_E_RANGE (-4)   /* env index out of range                       */

/* sticky per-handle device status bits (ctf_status) — situations in which the reference raises */
#define CTF_ST_BAD_ACTION 1u   /* action outside 0..8: reference raises KeyError (gridworld_ctf.py:710) */
#define CTF_ST_NO_RESPAWN 2u   /* no open cell round the spawn: np.random.randint(0) ValueError (:771)  */
#define CTF_ST_SPAWN_EDGE 4u   /* respawn offset went negative (spawn on row/col 0, the WARNING at :773) */
#define CTF_ST_RNG_OVERRUN 8u  /* one step drew more than ~624 words from one generator: its rejection loops cannot be
                                  followed further (a run of > 500 rejected draws: does not happen)                  */
#define CTF_ST_SYNC_TIMEOUT 16u /* ctf_step_observe's single launch: a render tile waited longer than its bound (10 ms) for
                                   the step of its envs and went on (the launch's blocks did not run in index order)  */
#define CTF_ST_BAD_SNAPSHOT 32u /* ctf_load_states: a record's header or destination index was wrong; that env is untouched
                                   (ctf_save_states: a source index outside [0, E); that record's header is left invalid)      */
#define CTF_ST_BAD_GROUP 64u    /* ctf_harvest_episodes / ctf_harvest_visitation: a group id outside [0, n_groups); that env is skipped
                                   (ctf_export_visitation: an env index outside [0, E); that record is not written)             */

#define CTF_ST_BAD_STATE 128u   /* ctf_import_states: a record broke one of ctf_set_state's rules, or its index was outside [0, E);
                                   that env is untouched */

/* ctf_config.rng_mode */
#define CTF_RNG_MT19937 0 /* the reference's two MT19937 generators, bit for bit (default)                          */
#define CTF_RNG_COUNTER 1 /* opt-in: counter-based streams — word n of a stream = Philox4x32-10(key = the stream's
                             seed, counter = (n / 4, stream, "CTF1"))[n % 4]; the draws are made from those words by the
                             reference's own rules (random.shuffle, np.random.rand, np.random.randint): a reference run
                             whose three functions read the same tape gives the same trajectory                     */
#define CTF_RNG_COUNTER_DIRECT 2 /* the same tape and the same three draw rules as CTF_RNG_COUNTER, so the same trajectory for
                             the same seeds — but no generator words are stored; per env the state is the two seeds and the
                             two counts of words consumed (32 bytes), and the step computes the Philox blocks it draws from */

/* ctf_step flags */
#define CTF_STEP_AUTO_RESET 1u /* an env whose `done` is set is reset before it is stepped (not in the
                                  reference, which never auto-resets; off by default)               */

/* indices of the per-agent counters in ctf_state_view.metrics (gridworld_ctf.py:456-468) */
enum {
    CTF_M_TAG_COUNT = 0,
    CTF_M_RESPAWN_TAG_COUNT = 1,
    CTF_M_FLAG_PICKUPS = 2,
    CTF_M_FLAG_CAPTURES = 3,
    CTF_M_FLAG_DISPOSSESSIONS = 4,
    CTF_M_BLOCKS_LAID = 5,
    CTF_M_BLOCKS_MINED = 6,
    CTF_M_BLOCKS_LAID_DIST_OWN_FLAG = 7,
    CTF_M_BLOCKS_LAID_DIST_OPP_FLAG = 8,
    CTF_M_STEPS_DEFENDING_ZONE = 9,
    CTF_M_STEPS_ATTACKING_ZONE = 10,
    CTF_M_STEPS_ADJ_TEAMMATE = 11,
    CTF_M_STEPS_ADJ_OPPONENT = 12
};

/*
 * Flat description of one GridworldCtf configuration.  Built in Python by the facade from the
 * reference's constructor kwargs (gridworld_ctf.py:19-52) and scenario dict (scenarios.py), so the
 * numpy-slice painting of load_scenario (:352-381) and the set-ordering of get_tiles_used (:488-499)
 * stay on the host side of the boundary.
 */
typedef struct ctf_config {
    int32_t abi_version;          /* = CTF_ABI_VERSION                                          */
    int32_t n_agents;             /* N_AGENTS (:68)                                             */
    int32_t grid_size;            /* GRID_SIZE after load_scenario (:359)                        */
    int32_t n_channels;           /* len(TILES_USED)+1 (:997)                                   */
    int32_t game_steps;           /* GAME_STEPS (:60)                                           */
    int32_t flip_axis;            /* FLIP_AXIS (:358): -1 = None (both axes), 0, 1, 2           */
    int32_t home_flag_capture;    /* HOME_FLAG_CAPTURE (:65)                                    */
    int32_t use_adjusted_rewards; /* USE_ADJUSTED_REWARDS (:82)                                 */
    int32_t drop_flag_when_no_hp; /* DROP_FLAG_WHEN_NO_HP (:64)                                 */
    int32_t log_metrics;          /* 1 = keep counters + visitation maps (always on in the reference) */
    int32_t n_opponents[2];       /* len(OPPONENTS[t]) (:392-395)                               */
    int32_t rng_mode;             /* CTF_RNG_MT19937 (the reference's generators), CTF_RNG_COUNTER or CTF_RNG_COUNTER_DIRECT */
    int32_t reserved0[5];         /* keeps the doubles 8-byte aligned without implicit padding */

    double heal_per_step;         /* AGENT_HP_HEALING_PER_STEP (:212)                           */
    double tag_probability;       /* TAG_PROBABILITY (:231)                                     */
    double guardian_damage_multiplier; /* (:228)                                                */
    double vault_hp_cost;         /* (:234)                                                     */
    double vault_min_hp;          /* (:235)                                                     */
    double reward_capture;        /* REWARD_CAPTURE = 1 (:77)                                   */
    double reward_step;           /* REWARD_STEP = 0 (:78)                                      */
    double reward_tag;            /* REWARD_TAG = 0.0 (:79)                                     */
    double win_margin_scalar;     /* 0.1 (:75)                                                  */
    double loss_margin_scalar;    /* 0.0 (:76)                                                  */
    double opp_capture_punishment;/* OPP_FLAG_CAPTURE_PUNISHMENT_SCALAR = 0.5 (:80)             */
    double type_hp[4];            /* AGENT_TYPE_HP (:209)                                       */
    double type_damage[4];        /* AGENT_TYPE_DAMAGE (:215)                                   */

    int8_t agent_team[CTF_MAX_AGENTS];     /* AGENT_TEAMS (:203)                                */
    int8_t agent_type[CTF_MAX_AGENTS];     /* AGENT_TYPES (:206): 0 scout 1 guardian 2 vaulter 3 miner */
    int8_t opponents[2][CTF_MAX_AGENTS];   /* OPPONENTS[t][k] (:392-395), ascending agent idx   */
    int8_t flag_pos[2][2];                 /* FLAG_POSITIONS[t] = (row, col) (:360)             */
    int8_t capture_pos[2][2];              /* CAPTURE_POSITIONS[t] (:361)                       */
    int8_t spawn_pos[2][2];                /* SPAWN_POSITIONS[t] (:362)                         */
    int8_t start_pos[CTF_MAX_AGENTS][2];   /* AGENT_STARTING_POSITIONS[i] (:363)                */
    uint8_t tile_of_channel[CTF_MAX_CHANNELS]; /* [k] = TILES_USED[k-1] for k>=1; [0] unused    */
    uint8_t init_grid[CTF_MAX_CELLS];      /* grid painted by load_scenario, row-major G*G      */
} ctf_config;

/* Host-side copy of ONE env's state (attributes the reference exposes: grid, agent_positions,
 * agent_hp, has_flag, block_inventory, _arr, env_step_count, done, metrics). */
typedef struct ctf_state_view {
    uint8_t grid[CTF_MAX_CELLS];           /* self.grid, row-major G*G                          */
    int8_t pos[CTF_MAX_AGENTS][2];         /* self.agent_positions[i] = (row, col)              */
    double hp[CTF_MAX_AGENTS];             /* self.agent_hp[i]                                  */
    uint8_t has_flag[CTF_MAX_AGENTS];      /* self.has_flag[i]                                  */
    int32_t inventory[CTF_MAX_AGENTS];     /* self.block_inventory[i]                           */
    uint8_t perm[CTF_MAX_AGENTS];          /* self._arr (persists across reset, :244)           */
    int32_t step_count;                    /* self.env_step_count                               */
    int32_t done;                          /* self.done                                         */
    int32_t team_captures[2];              /* metrics['team_flag_captures'][t]                  */
    int32_t metrics[CTF_N_METRICS][CTF_MAX_AGENTS]; /* agent-level counters; team / type sums are derived */
    uint8_t visitation[CTF_MAX_AGENTS][CTF_MAX_CELLS]; /* metrics['agent_visitation_maps'][i], u8 wraps */
} ctf_state_view;

typedef struct ctf_env ctf_env; /* opaque; owns all device-side SoA state of n_envs envs */

/* GridworldCtf.__init__ + first reset() (gridworld_ctf.py:19-350, :383-477) for n_envs envs on
 * HIP device `device_id`.  RNG streams start as seeds 0 (see ctf_seed). */
int ctf_create(const ctf_config* cfg, int32_t n_envs, int32_t device_id, ctf_env** out);
void ctf_destroy(ctf_env* env);

int32_t ctf_n_envs(const ctf_env* env);
/* bytes of one env's observation block u8[N][C][G][G], elements of one env's metadata f16[N][M] */
int64_t ctf_obs_bytes_per_env(const ctf_env* env);
int64_t ctf_meta_elems_per_env(const ctf_env* env);

/* Per-env twin MT19937 streams.  Env e behaves as a reference process after
 * `random.seed(py_seeds[e]); np.random.seed(np_seeds[e])` (CPython init_by_array / NumPy legacy
 * init_genrand).  Host arrays of n_envs seeds; np seeds must be < 2^32.
 * (On the device a stream is kept as the ring of its NEXT 624 outputs, so that a step finds its random words in memory
 * and regenerates behind itself; the hand-over functions below convert to and from the standard form, exactly.)
 * In counter mode the seeds are the keys of the env's two counter streams (any 64-bit values), both at word 0. */
int ctf_seed(ctf_env* env, const uint64_t* py_seeds, const uint64_t* np_seeds, void* stream);
/* Exact state hand-over for one env: 624 words + position, i.e. random.getstate()[1] and
 * np.random.get_state()[1:3].  Either pointer may be NULL.  Synchronous. */
int ctf_set_rng_state(ctf_env* env, int32_t env_index, const uint32_t* py_mt625, const uint32_t* np_mt625);
int ctf_get_rng_state(ctf_env* env, int32_t env_index, uint32_t* py_mt625, uint32_t* np_mt625);

/* The same for ALL envs at once, stream-ordered and without a device synchronisation: py_dev / np_dev are DEVICE arrays
 * uint32 [E][625] (624 state words + position per env, either may be NULL).  ctf_get_rng_states returns the standard
 * form.  What the facade's global-RNG contract uses per step
 * (random.getstate() / np.random.get_state() in, the advanced states out) and what a checkpoint of a batch needs. */
int ctf_set_rng_states(ctf_env* env, const uint32_t* py_dev, const uint32_t* np_dev, void* stream);
int ctf_get_rng_states(ctf_env* env, uint32_t* py_dev, uint32_t* np_dev, void* stream);
/* Counter mode only (the four functions above return CTF_E_INVALID there, these two in MT19937 mode): the whole RNG state
 * of an env is how many words it has consumed from each stream.  counters_dev: DEVICE array uint64 [E][2] = (random,
 * np.random).  Stream-ordered.  ctf_set_rng_counters is what a checkpoint restore calls after ctf_seed. */
int ctf_get_rng_counters(ctf_env* env, uint64_t* counters_dev, void* stream);
int ctf_set_rng_counters(ctf_env* env, const uint64_t* counters_dev, void* stream);

/* GridworldCtf.reset() (gridworld_ctf.py:383-477) for the envs whose mask byte is non-zero
 * (NULL = all).  Draws no random numbers and keeps `_arr`, like the reference. */
int ctf_reset(ctf_env* env, const uint8_t* env_mask_dev, void* stream);

/* GridworldCtf.step(actions) (gridworld_ctf.py:849-918) for every env.
 *   actions_dev      int8 [E][N]
 *   rewards_f32_dev  float  [E][N] or NULL   (what ppo.py:107 stores)
 *   rewards_f64_dev  double [E][N] or NULL   (the reference's Python floats, bit-exact)
 *   done_dev         uint8 [E] or NULL */
int ctf_step(ctf_env* env, const int8_t* actions_dev, float* rewards_f32_dev, double* rewards_f64_dev,
             uint8_t* done_dev, uint32_t flags, void* stream);

/* standardise_state(i, reverse_grid) + get_env_metadata(i) for every agent of every env
 * (gridworld_ctf.py:975-1009, :1027-1069).
 *   obs_dev      uint8 [E][N][C][G][G] or NULL
 *   meta_dev     IEEE binary16 bits [E][N][M], M = 2N+6, or NULL.  Must be 8-byte aligned (the rows leave as 8-byte stores; an env's
 *                N * M * 2 bytes are a multiple of 8): ctf_observe, ctf_observe_codes and ctf_step_observe refuse any other
 *                pointer with CTF_E_INVALID before anything is launched
 *   reverse_mask bit i = reverse_grid for agent i; CTF_REVERSE_DEFAULT = (team(i) == 1), the value
 *                every caller in the reference passes (ppo.py:69,87; utils.py:535)
 * One launch: k_observe_tiles (one wave per 8 KiB of the flat buffer) when an env's block is a multiple of 16 bytes and at
 * least 8 KiB and obs_dev is 16-byte aligned, k_observe (one wave per env) otherwise; identical bytes either way.  When the
 * observations of all live handles of this process on the device together exceed 320 MB (more than the caches absorb) the tile
 * kernel's stores carry the nontemporal hint: the observations pass by the caches, which keep the env state for the next step
 * (CTF_OBS_NT=0 / 1 at ctf_create forces plain / hinted stores; other PROCESSES' handles on the device are not seen); smaller
 * batches' observations are left in the memory-side cache for their consumer.
 *
 * PLACEMENT of obs_dev (the caller's buffer, so the caller's business): on MI355X roughly one hipMalloc allocation
 * of > 1 GiB in ten is of a kind this launch streams into at 0.87 of the HBM peak, the others cost it 15-20 % — a property of the
 * allocation's physical backing, independent from one allocation to the next even after a free.  A caller that cares allocates a
 * candidate, times ctf_observe into it against a plain fill of the same bytes (the fill does not depend on the kind: render / fill
 * <= 1.08 is the fast kind, >= 1.15 the slow one), frees it if it is slow and tries again.  The Python facade does exactly that on first use of its
 * observation buffer: knobs placement_tries (default 256 candidates, CTF_PLACEMENT_TRIES), CTF_PLACEMENT_SECONDS (default 3.0: once a
 * buffer of the fast kind is in hand the search for a better one ends after this long; ten seconds while none has turned up) and placement_gib (default 16: the cap
 * on what the search may HOLD — it holds two buffers, the candidate and the best so far; CTF_PLACEMENT_GIB), tune_placement=False
 * to switch it off; VecGridworldCtf.placement reports kind, ratio, candidates tried, bytes held and the time it took.
 *
 * INVALIDATION RULE.  ctf_observe and ctf_step_observe write EVERY byte of obs_dev — except into the one buffer the caller has
 * handed over with ctf_obs_retain (below): there they rewrite only the 128-byte lines whose bytes differ from what this handle
 * last rendered into it.  Whoever else writes into a retained buffer (a fill, a copy, another handle, another library) must call
 * ctf_obs_invalidate before the next render; changes of the env STATE (ctf_reset, auto-reset, ctf_set_state, ctf_import_states,
 * ctf_load_states) and of reverse_mask need no notice. */
#define CTF_REVERSE_DEFAULT 0xFFFFFFFFu
int ctf_observe(ctf_env* env, uint8_t* obs_dev, uint16_t* meta_dev, uint32_t reverse_mask, void* stream);
/* which of the two a ctf_observe into obs_dev launches: 1 = k_observe_tiles, 0 = k_observe (profiling: attributing a measured
 * duration to the right kernel) */
int32_t ctf_observe_kernel(const ctf_env* env, const uint8_t* obs_dev);
/* 1 when that launch stores the observation with the nontemporal hint (the tile kernel while the live handles' observations on
 * the device exceed 320 MB, or CTF_OBS_NT=1), 0 for plain stores */
int32_t ctf_observe_stores_hinted(const ctf_env* env, const uint8_t* obs_dev);

/* RETAINED observations: rewrite only what changed.  Per env-step about 15 % of the 128-byte lines of an arena env's block differ
 * from the step before; a buffer that only this handle writes need not be rewritten whole.
 * Retention is opted into, never inferred: the address of a buffer proves nothing about its contents (an allocator hands the same
 * address out again; a caller fills its buffer), so every pointer that has not been retained keeps the meaning above.
 * ctf_obs_retain: the caller promises that from now on only this handle writes obs_dev, a full [E][N][C][G][G] block.  One retained
 *   buffer per handle; a second call replaces the first; obs_dev = NULL releases it.  Retaining invalidates: the next render
 *   into the buffer writes everything.  The first call allocates the handle's SHADOW on the device — per env the grid and the
 *   position bytes the buffer's block was last rendered from, and one key word that names the reverse mask of that render or
 *   says "unknown", and the four slot images of that grid (CGG bits each: what a view shows apart from the viewer's own cell),
 *   which a render carries forward from the cells that changed instead of rebuilding them; about 1 900 bytes per arena env,
 *   1 600 of them the images: 123 MB at 65 536 envs against 18 MB before the images — and the call waits for `stream` once (everything after it is capturable;
 *   on a stream that is being captured the call retains nothing and renders stay full).  Renders into the retained buffer are then k_observe_delta: one wave per env compares the state with the shadow, and
 *   rewrites the dirty lines (all of them where the key is not the expected one) and the metadata rows.  Validity is device
 *   state only, so a hipGraph captured before the shadow was ever written replays correctly.  The delta render applies when
 *   an env's block is a multiple of 16 bytes, at most 261 904 of them (a span of 2 048 lines), and obs_dev is 16-byte aligned; otherwise, and with
 *   CTF_OBS_RETAIN=0 in the environment (read at the call), ctf_obs_retain is a no-op and renders stay full.
 *   CTF_STEP_OBSERVE_ONE_LAUNCH=1 wins over retention: that launch renders in full and invalidates.  The delta render's
 *   stores carry the nontemporal hint by the full render's rule (above); CTF_OBS_DELTA_NT=0 / 1 at the call forces it off / on.
 *   Also read at the call and constant until the next one (so graph replays are unaffected): CTF_OBS_DELTA_REBUILD=1 (the slot
 *   images are rebuilt from the grid at every render and the shadow's are never touched) and, for tests and soaks,
 *   CTF_OBS_DELTA_ALL_DIRTY=1 (every line is rewritten at every render, the images still carried forward).
 * ctf_obs_invalidate: everything about the retained buffer is unknown again.  Stream-ordered, one small launch, capturable.
 * ctf_observe_retained: 1 if a ctf_observe into obs_dev would take the delta path now, else 0.
 * A render with obs_dev = NULL (metadata only) or into any other pointer leaves the shadow alone. */
int ctf_obs_retain(ctf_env* env, uint8_t* obs_dev, void* stream);
int ctf_obs_invalidate(ctf_env* env, void* stream);
int32_t ctf_observe_retained(const ctf_env* env, const uint8_t* obs_dev);

/* The same observation in compact form: the tile planes 1..C-1 of standardise_state are one-hot per cell
 * (plane k+1 = (relabelled grid == TILES_USED[k]), gridworld_ctf.py:990-1001) and plane 0 holds the single
 * own-position bit, so
 *   codes_dev    uint8 [E][N][G][G] or NULL: low 7 bits = index of the plane that is 1 at this cell (0 = none of
 *                1..C-1), bit 7 = plane 0;  obs[e][i][k][r][c] == (k ? (codes & 127) == k : codes >> 7)
 *   meta_dev     as ctf_observe
 *   selfcell_dev uint16 [E][N] or NULL: the cell index (row-major over G x G, after the flip) at which agent i's row has
 *                bit 7 set — redundant with codes_dev, for consumers that treat a team's agents together
 * 1/C of the bytes of ctf_observe; what a GPU policy (include/ctf_policy.h) and a rollout buffer consume. */
int ctf_observe_codes(ctf_env* env, uint8_t* codes_dev, uint16_t* meta_dev, uint16_t* selfcell_dev, uint32_t reverse_mask,
                      void* stream);

/* ctf_step immediately followed by ctf_observe (the rollout inner loop, ppo.py:59-98): the two launches enqueued by one
 * call.  With CTF_STEP_OBSERVE_ONE_LAUNCH=1, where the tile render applies (ctf_observe_kernel == 1), ONE launch instead,
 * k_step_observe: the step's blocks, its ring regeneration, then the render's tiles, each of which waits only for the step
 * blocks of its own (one or two) envs — the same results bit for bit, but 9 % slower at 65 536 arena envs, so not the
 * default (profiles/r06_one_launch_step_observe.md).  (Step and render fused per env group, one wave doing
 * both, was measured in round 2 — 25 % slower: profiles/r02_fused_step_observe_ablation.md.)
 * In the two-launch form the metadata rows are written by the step kernel, which holds every env's final record, and the render
 * runs without them (the same bits; meta_dev with obs_dev == NULL is one launch); CTF_STEP_META=0, read at every call, leaves them
 * to the render as before (profiles/r15_step_meta.md). */
int ctf_step_observe(ctf_env* env, const int8_t* actions_dev, float* rewards_f32_dev,
                     double* rewards_f64_dev, uint8_t* done_dev, uint8_t* obs_dev, uint16_t* meta_dev,
                     uint32_t reverse_mask, uint32_t flags, void* stream);
/* how many launches a ctf_step_observe into obs_dev makes now: 1 (k_step_observe) or 2 (k_step, then ctf_observe's kernel) */
int32_t ctf_step_observe_launches(const ctf_env* env, const uint8_t* obs_dev);

/* AGENT_TYPE_ACTION_MASK expanded as agent_network.py:66-75 does: mask_host[i][a] = 1 if action a is
 * legal for agent i (flag 1 => actions 0..4 only).  Host buffer uint8 [N][9]. */
int ctf_action_mask(const ctf_env* env, uint8_t* mask_host);

/* Host views of one env (synchronous; parity tests and the facade's attribute access). */
int ctf_get_state(ctf_env* env, int32_t env_index, ctf_state_view* host_out);
int ctf_set_state(ctf_env* env, int32_t env_index, const ctf_state_view* host_in);

/* ONE env step for a caller that lives in HOST memory: the batch-of-one mode behind the reference's own class API, i.e. what a
 * rollout loop over GridworldCtf does per step (ppo.py:59-98): step(actions) (gridworld_ctf.py:849-918), then standardise_state(i) +
 * get_env_metadata(i) for every agent (:975-1069), with the process-global generators handed in and back (random.getstate() /
 * np.random.get_state(); the reference draws from them inside step).  For a handle of n_envs == 1 (CTF_E_INVALID otherwise).
 * Everything — the hand-over of both generator states, the step, the render, the state read-back — is enqueued on `stream` as kernels
 * that read their inputs from, and write their outputs into, ONE pinned, device-mapped host block the handle owns (no copy operations),
 * and the call waits for the stream once: round 5 measured 408 us per env step for the same work through ctf_set_rng_states + ctf_step
 * + ctf_get_rng_states + ctf_observe + ctf_get_state + ctf_status with a wait behind each.
 * All pointers are HOST pointers; any OUT pointer may be NULL (not wanted).
 *   actions_host    int8 [N], or NULL: no step is made (state, observation and generator states are still returned: reset())
 *   py_mt625_in / np_mt625_in   uint32 [625] (624 words + position) to install BEFORE the step, or NULL (keep the device's)
 *   reverse_mask, flags         as ctf_observe / ctf_step
 *   rewards_host    double [N] (the reference's Python floats, bit-exact)      done_host    int32
 *   status_host     the sticky CTF_ST_* bits raised since the last read (cleared, like ctf_status)
 *   view_host       the env's state after the step (ctf_get_state's view)
 *   py_mt625_out / np_mt625_out uint32 [625]: the generators AFTER the step, standard form
 *   obs_host        uint8 [N][C][G][G]      meta_host   IEEE binary16 bits [N][M] */
int ctf_host_step(ctf_env* env, const int8_t* actions_host, const uint32_t* py_mt625_in, const uint32_t* np_mt625_in,
                  uint32_t reverse_mask, uint32_t flags, double* rewards_host, int32_t* done_host, uint32_t* status_host,
                  ctf_state_view* view_host, uint32_t* py_mt625_out, uint32_t* np_mt625_out, uint8_t* obs_host, uint16_t* meta_host,
                  void* stream);

/* Bulk export of the counters the duel / evaluation harness reads (utils.py:557-571, metrics_logger.py:137-159):
 *   metrics_dev   int32 [E][13][N] agent-level counters (CTF_M_* order) or NULL (zeros when log_metrics == 0)
 *   captures_dev  int32 [E][2]     metrics['team_flag_captures'] or NULL
 *   steps_dev     int32 [E]        env_step_count or NULL */
int ctf_export_counters(ctf_env* env, int32_t* metrics_dev, int32_t* captures_dev, int32_t* steps_dev, void* stream);

/* Batched snapshot, restore and clone of whole env states on the device (ctf_snapshot.h has the layout).
 * One env's state is one opaque RECORD of S = ctf_snapshot_bytes(env) bytes (a multiple of 256; it depends on the config only):
 * a 64-byte header (magic 'CTFS', layout version 1, the handle's config fingerprint) and the env's device form copied as it is —
 * record, grid, both streams' rings and digests with their positions, ready flags and ages, the counter-mode stream indices, and
 * with log_metrics the counters, the visitation base maps and the env's 512-entry visitation log.  Nothing is converted, so a
 * restored env continues bit for bit as the saved one would have.  Observations are not part of the state.
 * Records are valid across handles and processes whose fingerprints are equal, for the same layout version; a library version
 * that changes the layout version does not read older records.  The FINGERPRINT is a 64-bit FNV-1a over every rule and constant
 * of the config, the init grid, N, G, C, the strides of the device form, rng_mode and log_metrics — not n_envs, the device, the
 * seeds or the CTF_* environment switches: two handles built from the same kwargs agree.
 * Both calls are stream-ordered kernel launches (no synchronisation, no allocation) and can be captured into a hipGraph.  Buffers
 * are DEVICE pointers, 16-byte aligned; the index lists are DEVICE int32 arrays of n entries. */
int64_t ctf_snapshot_bytes(const ctf_env* env);        /* S: bytes of one env's record (multiple of 256) */
uint64_t ctf_snapshot_fingerprint(const ctf_env* env);
/* dst_dev[k] = record of env src_idx_dev[k], k < n.  src_idx_dev NULL = envs 0..n-1 (n <= E).  Repeats allowed. */
int ctf_save_states(ctf_env* env, const int32_t* src_idx_dev, int32_t n, uint8_t* dst_dev, void* stream);
/* env dst_idx_dev[k] := record src_dev[k], k < n <= E.  dst_idx_dev NULL = envs 0..n-1.  Indices must be distinct
 * (repeats: undefined).  A record whose header does not match this handle, or an index outside [0, E), writes nothing for that
 * record and raises CTF_ST_BAD_SNAPSHOT.  Observations are not part of the state: call ctf_observe afterwards. */
int ctf_load_states(ctf_env* env, const uint8_t* src_dev, const int32_t* dst_idx_dev, int32_t n, void* stream);

/* Harvest of finished episodes into per-group results, on the device (ctf_harvest.h has the row; the batched form of what
 * utils.duel's result sign, utils.py:562-569, and MetricsLogger.harvest_metrics, metrics_logger.py:137-159, read from one env).
 * acc_dev is a caller-owned table int64 [n_groups][H], H = ctf_harvest_words(env) = 8 + 13 * N, that the call ADDS to (the caller
 * zeroes it).  Row g sums over the taken envs e with group_dev[e] == g:
 *   [0] episodes   [1] team-0 wins   [2] draws   [3] team-1 wins (the sign of team_flag_captures[0] - [1])
 *   [4] [5] team_flag_captures of team 0 / 1   [6] env_step_count   [7] reserved (never written)
 *   [8 + m * N + i] agent-level counter m (CTF_M_* order) of agent i; with log_metrics == 0 these words are left untouched and the
 *   first seven are still counted.
 * Which envs are taken: those whose episode ended in the most recent step — `done` set AND env_step_count == GAME_STEPS.  That
 * holds for exactly one step per episode in both stepping modes: with CTF_STEP_AUTO_RESET the next step resets the env (count 1),
 * without it the env runs on past GAME_STEPS (`done` stays set, the count moves on).  So ONE call after EVERY step neither drops
 * nor double-counts an episode.  Two calls without a step in between count the same episodes twice; two steps without a call in
 * between lose the episodes of the envs that auto-reset in the second one.  CTF_HARVEST_ALL takes every env as it stands, ended
 * or not: the cut of a truncated duel (utils.py:559, step_count > max_steps).
 *   group_dev     int32 [E], or NULL: every env is group 0.  An id outside [0, n_groups) skips that env and raises CTF_ST_BAD_GROUP
 *   env_mask_dev  uint8 [E], or NULL: only envs whose byte is non-zero are looked at
 * One kernel launch and nothing else (capturable behind ctf_step_observe); env state is only read; the sums are integer sums, so
 * the table does not depend on the order in which envs are added.  acc_dev must be 8-byte aligned. */
#define CTF_HARVEST_ALL 1u
int32_t ctf_harvest_words(const ctf_env* env);
int ctf_harvest_episodes(ctf_env* env, const int32_t* group_dev, int32_t n_groups, const uint8_t* env_mask_dev, uint32_t flags,
                         int64_t* acc_dev, void* stream);

/* Visitation maps in bulk, on the device (ctf_visitation.h has the definition): metrics['agent_visitation_maps'] of many envs
 * without a ctf_get_state round trip per env.  THE MAP OF ONE ENV is what ctf_get_state's view holds before its u8 wrap: the base
 * maps (zeros + 1 at the start cells after a reset, or what ctf_set_state handed in / the env folded) plus 1 at the logged cell of
 * every step since; N * G * G = ctf_visitation_words(env) true counts [N][G * G], nothing wraps at 256 (callers that want the
 * reference's uint8 maps take `& 0xFF`: its `+=` on uint8 arrays wraps, and the sum of wrapped counts is congruent to the wrapped
 * sum of true counts).  Both calls fail with CTF_E_INVALID on a handle created with log_metrics == 0 (it keeps no maps); both are one
 * kernel launch and nothing else (stream-ordered, no allocation, no synchronisation, capturable behind ctf_step_observe); env state
 * is only read.
 * ctf_harvest_visitation: the per-group form.  acc_dev is a caller-owned table int64 [n_groups][N][G * G], 8-byte aligned, that the
 *   call ADDS to.  It takes the same envs under the same rules as ctf_harvest_episodes (`done` set and env_step_count ==
 *   GAME_STEPS, or every env with CTF_HARVEST_ALL; group_dev, NULL = group 0; env_mask_dev; an id outside [0, n_groups) skips the
 *   env and raises CTF_ST_BAD_GROUP): a call behind the same step with the same arguments covers exactly the same episodes, so row
 *   g sums to N * (steps + episodes) of the episode harvest's row g.  Integer sums: the table does not depend on the order of additions.
 * ctf_export_visitation: the per-env form.  out_dev[k] = the map of env idx_dev[k], uint32 [n][N][G * G], k < n; idx_dev NULL = envs
 *   0..n-1 (n <= E).  Repeats allowed.  An index outside [0, E) writes nothing for that record and raises CTF_ST_BAD_GROUP (the
 *   bit of "an id named no row of this handle": no new bit is needed). */
int32_t ctf_visitation_words(const ctf_env* env); /* N * G * G; 0 for a null handle */
int ctf_harvest_visitation(ctf_env* env, const int32_t* group_dev, int32_t n_groups, const uint8_t* env_mask_dev, uint32_t flags,
                           int64_t* acc_dev, void* stream);
int ctf_export_visitation(ctf_env* env, const int32_t* idx_dev, int32_t n, uint32_t* out_dev, void* stream);

/* Env states as plain arrays, in bulk and on the device: ctf_get_state / ctf_set_state for many envs in ONE stream-ordered kernel
 * launch each (no allocation, no copy, no synchronisation: capturable behind ctf_step_observe), without the host decode.
 * ctf_state_arrays holds DEVICE pointers.  Every member may be NULL (export: not wanted; import: see below), every pointer is
 * 16-byte aligned, and record k's row is dense: [n][...] with no padding to the device form's strides. */
typedef struct ctf_state_arrays {
    uint8_t* grid;          /* u8  [n][G*G]    self.grid, row-major                          */
    int8_t*  pos;           /* i8  [n][N][2]   agent_positions (row, col)                    */
    double*  hp;            /* f64 [n][N]                                                    */
    uint8_t* has_flag;      /* u8  [n][N]                                                    */
    int32_t* inventory;     /* i32 [n][N]      block_inventory (as ctf_state_view)           */
    uint8_t* perm;          /* u8  [n][N]      _arr                                          */
    int32_t* step_count;    /* i32 [n]                                                       */
    int32_t* team_captures; /* i32 [n][2]                                                    */
    uint8_t* done;          /* u8  [n]                                                       */
    int32_t* metrics;       /* i32 [n][13][N]  CTF_M_* order                                 */
    uint8_t* visitation;    /* IMPORT ONLY: u8 [n][N][G*G] base maps (ctf_set_state's)       */
} ctf_state_arrays;
/* ctf_export_states: record k of every non-NULL array = what ctf_get_state of env idx_dev[k] would show, bit for bit (hp too).
 *   idx_dev NULL = envs 0..n-1 (n <= E).  Repeats allowed.  An index outside [0, E) writes nothing for that record in any array
 *   and raises CTF_ST_BAD_GROUP (ctf_export_visitation's rule).  out->visitation must be NULL (ctf_export_visitation is the export
 *   of the maps) and out->metrics must be NULL on a handle with log_metrics == 0: CTF_E_INVALID.  Env state is only read.
 * ctf_import_states: ctf_set_state for many envs — env idx_dev[k] := record k, k < n <= E; idx_dev NULL = envs 0..n-1.  Indices must
 *   be distinct (repeats: undefined).  grid, pos, hp, has_flag, inventory, perm, step_count, team_captures and done are required
 *   (CTF_E_INVALID).  metrics NULL = zeros.  visitation NULL = the maps restart as after reset() (+1 at the config's start cells);
 *   non-NULL = the given u8 maps become the base maps.  Either way the visitation log is empty (folded up to step_count), exactly
 *   as ctf_set_state leaves it.  Either optional array on a log_metrics == 0 handle: CTF_E_INVALID.  The kernel applies
 *   ctf_set_state's checks per record — pos inside the grid, perm[i] < N, inventory in 0..1000, grid codes <= 13, 0 <= step_count
 *   < 2^28, index in [0, E) — and a record that fails writes NOTHING for that env and raises CTF_ST_BAD_STATE.  An env set by
 *   either call holds the same device bytes.  The generators are not touched; observations are not state. */
int ctf_export_states(ctf_env* env, const int32_t* idx_dev, int32_t n, const ctf_state_arrays* out, void* stream);
int ctf_import_states(ctf_env* env, const ctf_state_arrays* in, const int32_t* idx_dev, int32_t n, void* stream);

/* Sticky status bits raised by any env since the last call (synchronises `stream`, clears them). */
int ctf_status(ctf_env* env, uint32_t* out_bits, void* stream);

/* Synthetic workload helper for bench/tests: actions_dev[e][i] uniform on 0..8 from Philox4x32-10,
 * key = (seed lo, seed hi), counter = (global env index = env_offset + e, step, 0, 0). */
int ctf_random_actions(ctf_env* env, int8_t* actions_dev, uint64_t seed, uint32_t step,
                       uint32_t env_offset, void* stream);

/* Scripted opponents: a baseline policy computed on the device from the env STATE (not from an observation), so that an evaluation
 * or a league has a fixed anchor that plays at the env's speed and is reproducible bit for bit.  kind:
 *   CTF_SCRIPT_RUNNER  a flag runner.  Agent a of team t heads for T = flag_pos[t] if has_flag[a], else flag_pos[1 - t]: standing next
 *     to T is what the pickup and capture rules test (gridworld_ctf.py:583-600).  Goal cells: the cells inside the grid within
 *     Chebyshev distance 1 of T whose tile is OPEN (0).  d = breadth-first distance to the goal cells (d = 0) over OPEN cells with
 *     4-neighbour unit moves; every other tile is a wall: blocks, destructibles, flags and every agent (the asking one included).
 *     The action is the lowest-numbered of 0..3 (deltas (-1,0), (1,0), (0,1), (0,-1)) whose neighbour is inside the grid and has the
 *     minimum finite d; if there is none, 4 (stay).  Actions 5..8 are never chosen, so every agent type's action mask is respected.
 *     Exploration: w = Philox4x32-10(key = (seed lo, seed hi), counter = (env_offset + e, step, a, 0x424F5431)), ctf_random_actions'
 *     Philox; if w[0] < epsilon_q32 the action is (w[1] * 5) >> 32, uniform on 0..4.  epsilon_q32 = 0 is the deterministic bot.
 * The actions are ENV actions: they go to ctf_step as they are (a caller that maps its networks' team-1 actions through
 * REVERSED_ACTION_MAP must not map these).
 *   actions_dev  int8 [E][N]: written only for the agents whose bit is set in agent_mask; every other byte is left alone, so a caller
 *                fills in its own agents' actions and the bot the rest, in place
 * One kernel launch and nothing else (none for an empty mask): stream-ordered, no allocation, no synchronisation, capturable behind
 * ctf_step.  Works in every rng_mode and with log_metrics == 0; env state is only read and the env's generators are not touched.
 * CTF_E_INVALID, before anything is launched: an unknown kind, a mask bit at or above N, a NULL actions_dev. */
#define CTF_SCRIPT_RUNNER 0u
int ctf_scripted_actions(ctf_env* env, int8_t* actions_dev /* int8 [E][N] */, uint32_t agent_mask, uint32_t kind, uint32_t epsilon_q32,
                         uint64_t seed, uint32_t step, uint32_t env_offset, void* stream);

/* Scripted opponents with a ROLE per agent: nibble i of role_pack is agent i's role, so one team can mix them.  With opp(t) = every
 * agent of the other team that stands inside the grid (by the team bits, whatever agent_mask says) and dil(S) = the cells inside the
 * grid within Chebyshev distance 1 of a member of S, agent a of team t plays
 *   CTF_ROLE_RUNNER  as CTF_SCRIPT_RUNNER above.
 *   CTF_ROLE_CHASER  Tagging is automatic: an agent with damage > 0 hits every opponent within Chebyshev distance 1 at the end of its
 *     turn (gridworld_ctf.py:796-837).  S = opp(t).  If a's own cell is in dil(S): 4, it tags already.  Otherwise the runner's search
 *     and choice of action with the goal cells dil(S) & OPEN: the opponent nearest by PATH decides.
 *   CTF_ROLE_GUARD   S = the members of opp(t) that carry a flag; if nobody does, the members within Chebyshev distance
 *     CTF_GUARD_ZONE of flag_pos[t] (the reference's DEFENSIVE_ZONE_DISTANCE, gridworld_ctf.py:87, :882, and the zone in which a
 *     guardian hits harder, GUARDIAN_DEFENSE_DISTANCE, :226, :808-810).  S not empty: the chaser's rule on S.  S empty: within
 *     Chebyshev distance 1 of flag_pos[t] 4, otherwise the runner's search towards flag_pos[t].
 * An agent that carries a flag acts as the runner does, whatever its role.  Exploration is ctf_scripted_actions' rule bit for bit (the
 * same key, counter and tag), applied last; actions 5..8 are never produced.  actions_dev, the stream order and what is read are as for
 * ctf_scripted_actions: one kernel launch and nothing else (none for an empty mask), capturable.  A role_pack whose asked agents are
 * all runners launches ctf_scripted_actions' kernel.
 * CTF_E_INVALID, before anything is launched: a nibble above CTF_ROLE_GUARD, a non-zero nibble at or above N, a mask bit at or above
 * N, a NULL actions_dev. */
#define CTF_ROLE_RUNNER 0u
#define CTF_ROLE_CHASER 1u
#define CTF_ROLE_GUARD 2u
#define CTF_GUARD_ZONE 3
int ctf_scripted_roles(ctf_env* env, int8_t* actions_dev /* int8 [E][N] */, uint32_t agent_mask, uint64_t role_pack, uint32_t epsilon_q32,
                       uint64_t seed, uint32_t step, uint32_t env_offset, void* stream);

/* Scripted opponents that use their TYPE: ctf_scripted_roles with bit i of ability_mask = agent i moves with its type's ability.  Roles,
 * goal sets Q (the 3 x 3 window of a flag, dil(opp), dil(S)), what is decided before the search (the carrier's goal, a chaser in dil(S)
 * and a posted guard next to its flag stay) and the exploration rule (same key, counter and tag, uniform on 0..4, applied last) are
 * ctf_scripted_roles'.  What changes is how an agent MOVES towards Q, by its class, decided from the state the call reads:
 *   DIGGER   ability bit set and type 3 (miner).  Passable cells are OPEN (0), DESTRUCTIBLE_TILE1 (2) and DESTRUCTIBLE_TILE2 (3);
 *     blocks, flags and every agent are walls.  Entering a cell costs w = 1 (OPEN), 2 (tile 3: one hit, then the move) or 3 (tile 2:
 *     two hits, then the move), the counts mine_block and movement_handler give (gridworld_ctf.py:669-690, :577-580).  Goal cells:
 *     Q & passable.  D(c) = the least sum of entry costs over 4-neighbour paths from c into a goal cell; the goal cell's own cost is
 *     counted, the start cell's is not, D of a goal cell is 0.  The action is the lowest-numbered of 0..3 whose neighbour n is inside
 *     the grid, passable and has the minimum finite w(n) + D(n); none: 4.  Moving into a destructible tile IS the mining action, so
 *     the output is still 0..3.
 *   VAULTER  ability bit set, type 2 and (hp[a] - VAULT_HP_COST) > VAULT_MIN_HP, evaluated in f64 as the step evaluates it
 *     (gridworld_ctf.py:649-650).  Passable cells are OPEN only.  Moves: the four unit moves and the jumps 5..8 with deltas (-2,0),
 *     (2,0), (0,2), (0,-2); a jump needs its landing cell inside the grid and OPEN, the cell jumped over may hold anything (:123-133,
 *     :643-650).  Every move costs 1, and later jumps are taken to be affordable: the agent plans again at every call, as a walker
 *     once its hp permits no jump.  The action is the lowest-numbered of 0, 1, 2, 3, 5, 6, 7, 8 whose landing cell has the minimum
 *     finite D (a walk wins a tie with a jump); none: 4.
 *   WALKER   everyone else: ctf_scripted_roles' action, bit for bit, whatever the ability bit says.
 * actions_dev, the stream order and what is read are as for ctf_scripted_actions: one kernel launch and nothing else (none for an
 * empty mask), capturable; every rng_mode, log_metrics == 0 included; env state is only read.  When ability_mask & agent_mask names no
 * agent of type 2 or 3, the launch is ctf_scripted_roles' own.
 * CTF_E_INVALID, before anything is launched: everything ctf_scripted_roles refuses, and an ability_mask bit at or above N. */
int ctf_scripted_abilities(ctf_env* env, int8_t* actions_dev /* int8 [E][N] */, uint32_t agent_mask, uint64_t role_pack, uint32_t ability_mask,
                           uint32_t epsilon_q32, uint64_t seed, uint32_t step, uint32_t env_offset, void* stream);

/* The scripted planners' COST-TO-GO: for every asked agent, how far it is from the goal set its scripted planner heads for, under the
 * rules that planner moves by — a path cost that knows walls, destructible tiles, jumps and other agents, where a Chebyshev distance
 * does not.  A potential for reward shaping (F = gamma Phi(s') - Phi(s) leaves the optimal policy alone), a progress measure for
 * evaluations, a filter for curricula.  Roles (role_pack), classes (ability_mask, type and hp) and goal sets Q (the 3 x 3 window of
 * a flag, dil(opp), dil(S), before any tile is asked for) are ctf_scripted_abilities'.  cost_dev[e][a] is THE COST OF REACHING Q, not
 * "the planner's next move + 1":
 *   0              a is decided before the search (a chaser standing in dil(S), a posted guard next to its flag), or a's own cell
 *                  lies in Q (a runner next to the flag it wants: ctf_scripted_abilities still moves such an agent, to another open
 *                  cell of the window, so a cost of 0 does not mean action 4);
 *   >= 1           the least total entry cost, over move sequences of a's class, from a's cell into a cell of Q the class may enter:
 *                  WALKER 1 + d(n), the minimum over the four neighbours n; DIGGER w(n) + D(n), the minimum over the four neighbours,
 *                  with entry costs 1 / 2 / 3; VAULTER 1 + d(n), the minimum over the eight landing cells — the number of steps the
 *                  planner needs if nothing else moves.  At most 3 G G;
 *   CTF_COST_NONE  no such sequence exists, or a stands outside the grid (no valid state has one).
 * With epsilon 0, on the same state and arguments: cost == CTF_COST_NONE implies ctf_scripted_abilities' action 4, cost >= 1 an
 * action other than 4.  There is no exploration and no seed: the cost is a function of the state.
 *   cost_dev  int16 [E][N]: written only for the agents whose bit is set in agent_mask; every other entry is left alone
 * One kernel launch and nothing else (none for an empty mask; one kernel for every role and class): stream-ordered, no allocation,
 * no synchronisation, capturable.  Works in every rng_mode and with log_metrics == 0; env state is only read.
 * CTF_E_INVALID, before anything is launched: everything ctf_scripted_abilities refuses, a NULL cost_dev, an odd cost_dev address. */
#define CTF_COST_NONE (-1)
int ctf_scripted_costs(ctf_env* env, int16_t* cost_dev /* int16 [E][N] */, uint32_t agent_mask, uint64_t role_pack, uint32_t ability_mask,
                       void* stream);

/* WHAT EACH ACTION WOULD DO in the state as it stands: the `act` part of the step (gridworld_ctf.py:700-732) as a pure function of
 * the state — grid, position, hp, has_flag, inventory — and the config, for every asked agent i and action a in 0..8.  ctf_action_mask
 * knows the agent's TYPE only; this knows walls, grid edges, other agents, an empty block inventory, a vaulter whose hp no longer
 * pays for a jump and a spawn window that refuses a block.  effect(i, a) is a byte of flags: what act(i, a) would do IF AGENT i ACTED
 * NOW, BEFORE ANYONE ELSE MOVES.  Inside a real step the agents act in a shuffled order, so another agent may move first (or tag
 * this one out) and the action may then do something else: every multi-agent action mask carries that caveat.
 *   CTF_EFF_MOVES     the agent's position changes (:577-580)
 *   CTF_EFF_JUMPS     the move is a vault: actions 5..8, type 2, landing cell open, (hp - VAULT_HP_COST) > VAULT_MIN_HP evaluated in f64
 *                     as the step evaluates it (:643-657); the hp falls by the cost.  Implies MOVES
 *   CTF_EFF_PICKS_UP  the move picks the other flag up (:583-591).  Implies MOVES
 *   CTF_EFF_CAPTURES  the move captures (:594-610, HOME_FLAG_CAPTURE included); a pickup and a capture in one move set both.  Implies MOVES
 *   CTF_EFF_MINES     a miner hits a destructible tile (:669-690): tile 2 becomes 3, tile 3 becomes open
 *   CTF_EFF_BREAKS    that hit opens the cell (the tile was 3); the inventory rises by one unless it is at its cap.  Implies MINES
 *   CTF_EFF_LAYS      a miner lays a block (:659-667: inventory > 0, target open and outside both spawn windows)
 * Bit 7 is always 0; MOVES, MINES and LAYS exclude one another.  effect == 0: the action leaves grid, positions, hp, flags, inventory
 * and counters untouched (action 4, actions 5..8 of types 0 and 1, a target outside the grid or neither open nor minable).  An agent
 * whose position is outside the grid has every effect 0.  Tagging, healing and the shuffle are not part of `act` nor of the effect.
 *   effects_dev  u8  [E][N][9] or NULL: effects_dev[e][i][a] = effect(i, a)
 *   mask_dev     u16 [E][N]    or NULL: bit a of mask_dev[e][i] is set iff effect(i, a) != 0; bit 4 and bits 9..15 are never set
 *                (a caller that wants "stay" legal ORs 0x10 in)
 * Only the entries of the agents whose bit is set in agent_mask are written; every other byte is left alone.  One kernel launch and
 * nothing else (none for an empty mask): stream-ordered, no allocation, no synchronisation, capturable.  Works in every rng_mode and
 * with log_metrics == 0; env state is only read and no status bit is set.
 * CTF_E_INVALID, before anything is launched: a null handle, both outputs NULL, a mask bit at or above N, an odd mask_dev address. */
#define CTF_EFF_MOVES 1u
#define CTF_EFF_JUMPS 2u
#define CTF_EFF_PICKS_UP 4u
#define CTF_EFF_CAPTURES 8u
#define CTF_EFF_MINES 16u
#define CTF_EFF_BREAKS 32u
#define CTF_EFF_LAYS 64u
int ctf_action_effects(ctf_env* env, uint16_t* mask_dev /* u16 [E][N] or NULL */, uint8_t* effects_dev /* u8 [E][N][9] or NULL */,
                       uint32_t agent_mask, void* stream);

/* A RANDOM OPPONENT THAT NEVER BUMPS INTO A WALL: for each asked agent i of env e, S = its mask under ctf_action_effects' rule.
 * S empty: action 4, no draw.  Otherwise w = Philox4x32-10(key = (seed lo, seed hi), counter = (env_offset + e, step, i, 0x45464631
 * "EFF1")), k = (w[0] * popcount(S)) >> 32, and the action is the index of the (k + 1)-th lowest set bit of S.  These are env
 * actions: they go to ctf_step as they are.  Write discipline (only the asked agents' bytes), stream order, capturability and
 * refusals are ctf_scripted_actions': one kernel launch and nothing else, CTF_E_INVALID for a null handle, a NULL actions_dev or a
 * mask bit at or above N. */
int ctf_random_effective_actions(ctf_env* env, int8_t* actions_dev /* i8 [E][N] */, uint32_t agent_mask, uint64_t seed, uint32_t step,
                                 uint32_t env_offset, void* stream);

/* RANDOMISED EPISODE STARTS: ctf_reset with the asked agents drawn onto open cells round their start cells, on the device.  For every
 * env e whose mask byte is non-zero (NULL = all):
 *   A. everything ctf_reset does: the grid becomes the init grid; hp, flags and inventories are reset; the step count, the captures
 *      and `done` are reset; the counters are zeroed; `perm` is kept and both generators are untouched;
 *   B. placement, for i = 0 .. N - 1 in ascending order.  An agent outside agent_mask stays on s_i = start_pos[i].  For an agent
 *      inside it the candidate set C_i is {s_i} together with every cell c with init_grid[c] == 0 (OPEN), cheb(c, s_i) <= radius, c
 *      not taken by an earlier agent of this call and — with CTF_SCATTER_OWN_SIDE — cheb(c, flag_pos[t]) <= cheb(c, flag_pos[1 - t]),
 *      t the agent's team.  s_i holds an agent tile in the init grid, so it is never OPEN: nobody but i can draw it and n = |C_i| >= 1
 *      always; there is no failure case and no status bit.  r = round + (episode_dev ? episode_dev[e] : 0), a u32 add that wraps;
 *      w = Philox4x32-10(key = (seed lo, seed hi), counter = (env_offset + e, r, i, 0x53435431 "SCT1")) — ctf_random_actions'
 *      generator; k = (w[0] * n) >> 32; the agent's cell is the (k + 1)-th element of C_i in ascending row-major cell index.  Then
 *      pos[i] = cell, grid[s_i] = 0 and grid[cell] = init_grid[s_i];
 *   C. with episode_dev, episode_dev[e] += 1 (masked envs only).  Visitation (log_metrics): when every agent stands on its s_i the
 *      env is left exactly as ctf_reset leaves it; otherwise the base maps are written out — zeros, 1 at each agent's cell — and the
 *      log is empty: the device form ctf_import_states gives for those maps at step 0.
 * Envs outside the mask are untouched, their episode_dev entry included.  Any radius >= G - 1 means the whole grid.  radius == 0 or
 * agent_mask == 0 gives ctf_reset's result bit for bit (k_reset itself is launched; with episode_dev, which k_reset does not know, the
 * placement kernel with an empty agent mask — the same bytes) and episode_dev is still advanced.
 * One kernel launch and nothing else: stream-ordered, no allocation, no synchronisation, no host state; capturable behind ctf_step,
 * and with episode_dev every replay of the graph draws afresh.  Works in every rng_mode and with log_metrics == 0.  A retained
 * observation buffer needs no ctf_obs_invalidate: this is a state change like ctf_reset.
 * WHAT IT IS NOT: the reference has no such reset.  A plain ctf_reset, and the in-kernel auto-reset of CTF_STEP_AUTO_RESET, still go
 * to the config's start cells: a loop that wants scattered starts steps WITHOUT auto-reset and calls this with env_mask_dev =
 * done_dev, behind the harvests (which only read).
 * CTF_E_INVALID, before anything is launched: a null handle, radius < 0, a mask bit at or above N, a flag bit other than
 * CTF_SCATTER_OWN_SIDE, an episode_dev that is not 4-byte aligned. */
#define CTF_SCATTER_OWN_SIDE 1u
int ctf_reset_scattered(ctf_env* env, const uint8_t* env_mask_dev /* u8 [E] or NULL = all */,
                        uint32_t agent_mask, int32_t radius, uint32_t flags,
                        uint64_t seed, uint32_t round, uint32_t* episode_dev /* u32 [E] or NULL */,
                        uint32_t env_offset, void* stream);

const char* ctf_last_error(void); /* thread-local */
int32_t ctf_abi_version(void);
/* sizeof(ctf_config) / sizeof(ctf_state_view) as compiled, so a binding can verify its struct mirror */
int32_t ctf_sizeof_config(void);
int32_t ctf_sizeof_state_view(void);

#ifdef __cplusplus
}
#endif
#endif /* CTF_ENV_H */
