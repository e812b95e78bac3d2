/*
 * gym_po_amd — C ABI of the MI355X-native vectorised env engine for gym_po's POMDP gridworlds.
 *
 * This is the drop-in boundary: a plain C shared library (libgympo_amd.so; no torch types,
 * plain pointers and sizes). Every device pointer below is a HIP device pointer owned by the
 * CALLER (e.g. a torch-ROCm tensor's data_ptr()); env state and lookup tables are owned by the
 * handle. All calls are asynchronous on the given hipStream_t (passed as void*; NULL = the
 * default stream) unless documented otherwise. A handle is not re-entrant; use one per
 * stream/thread. Every entry point returns 0 on success, a negative GP_E* code otherwise, and
 * gp_last_error() returns thread-local text for the last failure.
 *
 * Reference interfaces replaced (paths relative to DavidSlayback/gym-po-taxi):
 *   gp_create(GP_KIND_GRID)   MultistoryFourRoomsEnv.__init__   gym_po/envs/rooms/msrooms.py:266-367
 *                             RoomsEnv.__init__                  gym_po/envs/rooms/rooms.py:84-175
 *   gp_create(GP_KIND_TAXI)   TaxiVecEnv.__init__                gym_po/envs/extended_taxi.py:158-230
 *   gp_create(GP_KIND_CROOMS) CRoomsEnv.__init__                 gym_po/envs/rooms/crooms.py:104-244
 *   gp_create(GP_KIND_ANTTAG) AntTagEnv task rules (grid restatement, build-defined)
 *                                                                gym_po/envs/ant_tag.py:88-157
 *   gp_create(GP_KIND_CARFLAG) CarVecEnv.__init__ / DiscreteActionCarVecEnv.__init__
 *                                                                gym_po/envs/car_flag.py:50-85, :289-299
 *   gp_create(GP_KIND_ROCKSAMPLE) RockSample (the reference has only the Obs / ACTION enums and a constructor
 *                             signature; the rules are build-defined) gym_po/envs/rocksample/rocksample.py
 *   gp_create(GP_KIND_HEAVENHELL) AntHeavenHellEnv task rules (grid restatement, build-defined)
 *                                                                gym_po/envs/ant_heaven_hell.py:35-40, :99-137
 *   gp_seed / gp_seed_words   gymnasium Env.reset(seed=) -> seeding.np_random(seed)
 *                             (msrooms.py:376, rooms.py:184, extended_taxi.py:239, crooms.py:246-249)
 *   gp_reset                  *.reset()      msrooms.py:369-381, rooms.py:177-189,
 *                                            extended_taxi.py:232-242, crooms.py:251-266
 *   gp_step                   *.step()       msrooms.py:390-413, rooms.py:198-222,
 *                                            extended_taxi.py:244-287, crooms.py:276-298
 *   gp_rollout                K x step() in one call (agent rollout loop, tester.py:24-26)
 *   gp_get_state/gp_set_state the env's array state (agent_zyx/goal_zyx/elapsed, s/elapsed/...)
 *   gp_set_replay             replaces env.np_random's draws with pre-decided per-env values
 */
#ifndef GYM_PO_AMD_H
#define GYM_PO_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GP_ABI_VERSION 1

/* ---- status codes ---- */
#define GP_OK 0
#define GP_E_INVALID (-1)   /* bad argument / config (reference would raise)           */
#define GP_E_HIP (-2)       /* HIP runtime error                                         */
#define GP_E_UNSUPPORTED (-3)/* mode not available for this env kind                     */
#define GP_E_STATE (-4)     /* call order (e.g. step before reset)                       */
#define GP_E_DEVICE (-5)    /* a device-side failure of an earlier asynchronous launch (a persistent
                               kernel's cross-block wait timed out): outputs and env state since the
                               last seed are invalid; reported by gp_check / gp_metrics /
                               gp_get_rng_state, cleared by reseeding                          */

/* ---- env kinds ---- */
#define GP_KIND_GRID 1   /* FourRooms (multistory) and ROOMS: discrete cell gridworlds */
#define GP_KIND_TAXI 2
#define GP_KIND_CROOMS 3
#define GP_KIND_ANTTAG 4
#define GP_KIND_CARFLAG 5 /* Car-Flag: 1-D heaven/hell POMDP (car_flag.py) */
#define GP_KIND_ROCKSAMPLE 6 /* RockSample (Smith & Simmons 2004), build-defined rules: gp_rocksample_config */
#define GP_KIND_HEAVENHELL 7 /* grid Heaven-Hell (the task of ant_heaven_hell.py), build-defined rules: gp_heavenhell_config */
#define GP_KIND_POMDP 8 /* tabular POMDP (T / O / R tables), build-defined rules: gp_pomdp_config */

/* ---- RNG modes ---- */
#define GP_RNG_NUMPY 0   /* seed-identical to numpy Generator(PCG64(SeedSequence(seed))): GRID, CROOMS, TAXI, CARFLAG */
#define GP_RNG_PHILOX 1  /* counter-based Philox4x32-10 keyed by (seed, env, step): fusable rollouts */
#define GP_RNG_REPLAY 2  /* pre-decided per-env draws supplied by gp_set_replay each step       */

/* ---- observation dtypes reported by gp_obs_info ---- */
#define GP_DTYPE_I32 0
#define GP_DTYPE_U8 1
#define GP_DTYPE_F32 2
#define GP_DTYPE_F64 3

/* ---- GRID config (FourRooms / ROOMS) ---- */
#define GP_FLAVOR_ROOMS 0      /* rooms.py: wall == -1, binary Hansen (observations.py:44-71)       */
#define GP_FLAVOR_MULTISTORY 1 /* msrooms.py: wall == 0, stairs 2/3, ternary Hansen (msrooms.py:162) */

#define GP_OBS_HANSEN 0     /* scalar Hansen index x goal multiplier            int32 [B]       */
#define GP_OBS_HANSEN_VEC 1 /* per-direction codes                              uint8 [B,n]     */
#define GP_OBS_TABLE 2      /* table[agent] + table2[goal] (mdp / room scalars)  int32 [B]       */
#define GP_OBS_COORDS 3     /* agent (and goal) coordinates                     int32 [B,d|2d]  */
#define GP_OBS_WINDOW 4     /* n x n local window (observations.py:74-103)      uint8 [B,n,n]   */
#define GP_OBS_ONEHOT 5     /* one-hot of the scalar obs (taxi)                 uint8 [B,space] */
#define GP_OBS_F32 6        /* float observation (crooms coords)                float [B,d]     */

typedef struct gp_grid_config {
  int32_t flavor;          /* GP_FLAVOR_*                                                       */
  int32_t depth, height, width; /* grid shape (depth = floors; 1 for ROOMS)                     */
  const int32_t* cells;    /* [depth*height*width] C-order cell values (room id / walk code)    */
  int32_t n_actions;       /* 4 (cardinal N,E,S,W) or 8 (ordinal N,NE,...,NW) (action_utils.py)  */
  double action_failure_probability;
  int32_t obs_kind;        /* GP_OBS_HANSEN / _HANSEN_VEC / _TABLE / _COORDS / _WINDOW          */
  int32_t obs_dirs;        /* Hansen directions: 4 or 8                                         */
  int32_t obs_goal;        /* include goal information (obs_type contains "goal")               */
  int32_t obs_n;           /* window size for GP_OBS_WINDOW                                     */
  const int32_t* obs_table;  /* GP_OBS_TABLE: per-cell value for the agent    [ncells]          */
  const int32_t* obs_table2; /* GP_OBS_TABLE: per-cell value for the goal (may be NULL) [ncells] */
  int32_t fixed_goal;      /* flat cell index, or -1 = random over valid goal cells; a value
                              >= ncells is an unreachable goal (ROOMS "32" ENDS quirk)          */
  int32_t fixed_agent;     /* flat cell index, or -1 = random over valid agent cells            */
  int32_t time_limit;      /* truncated = elapsed > time_limit                                  */
  float step_reward, wall_reward, goal_reward;
} gp_grid_config;

typedef struct gp_taxi_config {
  int32_t rows, cols;      /* navigable grid (5x5 TAXI_MAP, 8x8 EXTENDED_TAXI_MAP)              */
  int32_t desc_rows, desc_cols;
  const char* desc;        /* [desc_rows*desc_cols] bordered char map ('|' walls, ':' pseudo)   */
  int32_t pseudo_walls;    /* 1 if the map uses ':' columns (cc(r,c) = (r+1, 2c+1))            */
  int32_t n_locs;
  const int32_t* locs;     /* [n_locs*2] (row, col) of R,G,Y,B in row-major order               */
  int32_t num_passengers;
  int32_t time_limit;
  int32_t obs_kind;        /* GP_OBS_TABLE (raw state s, extended_taxi.py:368) or GP_OBS_HANSEN
                              ((hansen[r,c]*(L+1)+p)*L+d, extended_taxi.py:370-372)              */
  int32_t one_hot;         /* 1: emit that index one-hot, uint8 [B, n_obs] (GP_OBS_ONEHOT layout;
                              a build-side encoding, the reference has none)                     */
  float reward_goal, reward_bad, reward_any;
} gp_taxi_config;

typedef struct gp_crooms_config {
  int32_t height, width;
  const int32_t* cells;    /* room-id grid, wall == -1 (layouts.py np_to_grid)                    */
  int32_t use_velocity;    /* crooms.py:304-310: v = clip(v + a, +-5), proposed = agent + v        */
  double cell_size;        /* >= 1 (smaller cells index past the grid: the reference raises)       */
  int32_t action_kind;     /* 0 = continuous (y,x) [B,2]; 4 / 8 = discrete cardinal / ordinal [B]  */
  int32_t action_f64;      /* continuous actions are float64 [B,2] (1) or float32 [B,2] (0)        */
  double action_failure_probability;
  double action_std, action_power;
  int32_t obs_kind;        /* GP_OBS_F32 (vector mdp: agent [+ goal] y,x) or GP_OBS_HANSEN /
                              _HANSEN_VEC / _TABLE / _WINDOW evaluated on floor(coord / cell_size)  */
  int32_t obs_f64;         /* GP_OBS_F32 emitted as float64 (GP_DTYPE_F64) instead of float32       */
  int32_t obs_dirs, obs_goal, obs_n;
  const int32_t* obs_table;  /* GP_OBS_TABLE: per-cell value for the agent [height*width]         */
  const int32_t* obs_table2; /* GP_OBS_TABLE: per-cell value for the goal (may be NULL)           */
  int32_t goal_fixed;      /* 1: goal cell (goal_y, goal_x) every reset (may lie off the grid)    */
  int32_t goal_y, goal_x;
  int32_t agent_fixed;     /* 1: agent cell (agent_y, agent_x) every reset                         */
  int32_t agent_y, agent_x;
  int32_t time_limit;
  float step_reward, wall_reward, goal_reward;
  double goal_threshold;   /* terminated = ||agent - goal||_2 <= goal_threshold (float64)         */
} gp_crooms_config;

typedef struct gp_anttag_config {
  int32_t size;            /* arena cells per side (interior)                                   */
  int32_t tag_radius2;     /* squared Chebyshev/Euclid radius (cells^2) for a tag              */
  int32_t visible_radius2; /* squared radius under which the target is observed                */
  int32_t min_start_dist2; /* squared minimum start separation                                 */
  int32_t time_limit;
  float tag_reward, step_reward;
  int32_t obs_index;       /* 0: obs = int32 [ant y, ant x, target y, target x] (GP_DTYPE_I32, width 4), the target
                              (-1, -1) unless visible. 1: obs = the scalar int32 (width 1)
                              ant_cell * (nc + 1) + (visible ? target_cell : nc), nc = size * size, cell = y * size + x:
                              the same information (a bijection onto the vectors that occur), in [0, nc * (nc + 1)).
                              Transitions, draws, rewards, flags, state and metrics do not depend on it. The index
                              obs has no buffer alignment requirement; the vector obs needs 16-B aligned buffers. */
} gp_anttag_config;

/* Car-Flag (car_flag.py:50-144, :286-303). Observation: GP_DTYPE_F32, width 3 (position, velocity, direction). */
typedef struct gp_carflag_config {
  int32_t time_limit;      /* truncated = elapsed >= time_limit (car_flag.py:129)                  */
  int32_t action_kind;     /* 0 = continuous float32 [B] (all-float32 arithmetic); 1 = continuous float64 [B]
                              (float64 arithmetic, stored as f32); n >= 2 = discrete int32 [B] into action_table
                              (float64 arithmetic, DiscreteActionCarVecEnv)                          */
  const double* action_table; /* [n] forces of the discrete actions (np.linspace(-1, 1, n)); else NULL */
} gp_carflag_config;

/* RockSample (GP_KIND_ROCKSAMPLE; GP_RNG_PHILOX only: there is no reference stream, so GP_RNG_NUMPY / GP_RNG_REPLAY
 * return GP_E_UNSUPPORTED). The reference names the env and never builds it; these rules are this build's.
 *   grid     height x width cells, 1 <= height, width <= 16, cell = y * width + x, north is y - 1.
 *   rocks    n_rocks (1..16) distinct cells; per env a good mask, bit i set = rock i is good.
 *   actions  A = 5 + n_rocks: 0 N, 1 E, 2 S, 3 W, 4 SAMPLE, 5 + i = CHECK rock i. [-A, 0) wraps as numpy indexing
 *            does; anything else is flagged GP_DERR_ACTION and clamped.
 *   step     elapsed += 1, reading = NULL (0). N / S / W: move if the target is inside the grid (step_reward), else
 *            stay (wall_reward). E: the same, except that from the last column the agent exits: terminated,
 *            exit_reward. SAMPLE on rock i's cell: good_reward if bit i is set, else bad_reward; bit i is cleared.
 *            SAMPLE elsewhere: empty_reward. CHECK i: check_reward; with y = x0 >> 1,
 *            correct = y < sensor_thr[cell][i], the reading is GOOD (1) if (bit i) == correct, else BAD (2).
 *   end      truncated = elapsed >= time_limit (gymnasium TimeLimit), independent of terminated. On either the env
 *            resets in the same step: agent on init_cell, mask = x1 & (2^n_rocks - 1), elapsed = 0; the step's obs
 *            is that of the reset state with reading NULL.
 *   draws    one Philox4x32-10 block per (env, step), counter (env, step_lo, step_hi, 0x726f636b) under the handle's
 *            key, step being the host-tracked index of the other philox kinds: x0 the check, x1 the reset mask.
 *            gp_reset draws every mask from x1 of the block at the reset's step index.
 *   obs      int32 [B]: the reading (obs_cell = 0, 3 values) or cell * 3 + reading (obs_cell = 1).
 *   state    gp_get_state / gp_set_state: agent cell, good mask, elapsed, int32 [B] each (set clamps the cell to the
 *            grid and elapsed to [0, 65535], keeps the low n_rocks bits of the mask, and makes the last reading NULL).
 * GP_E_INVALID: a side or n_rocks out of range, duplicate rocks, a rock or init_cell off the grid, time_limit outside
 * [1, 65535] (elapsed is kept in 16 bits), a sensor_thr entry above 2^31. */
typedef struct gp_rocksample_config {
  int32_t height, width, n_rocks;
  const int32_t* rocks;       /* [n_rocks] rock cells                                                */
  int32_t init_cell;          /* the agent's cell at every episode start                            */
  const uint32_t* sensor_thr; /* [height*width][n_rocks]: P(check of rock i from cell is right) * 2^31, <= 2^31
                                 (lowered by the caller, e.g. floor(0.5 * (1 + 2^(-d / d0)) * 2^31): no libm
                                 call of the library decides a result)                                */
  int32_t obs_cell;           /* 0: obs = reading; 1: obs = cell * 3 + reading                       */
  int32_t time_limit;
  float exit_reward, good_reward, bad_reward, empty_reward, check_reward, step_reward, wall_reward;
} gp_rocksample_config;

/* Grid Heaven-Hell (GP_KIND_HEAVENHELL; GP_RNG_PHILOX only: there is no reference stream, so GP_RNG_NUMPY /
 * GP_RNG_REPLAY return GP_E_UNSUPPORTED). A build-defined grid restatement of the task of the reference's
 * AntHeavenHellEnv (ant_heaven_hell.py:35-40 the heaven / hell / priest points and the radius, :99-119 the reset with a
 * fair coin for the heaven side, :121-137 the step; walls and start box: assets/ant_heaven_hell.xml:72-100 and
 * ant_heaven_hell.py:74). The reference env is a MuJoCo ant: parity with it is unpinned by construction.
 *   maze     height x width cells, 1 <= height, width <= 16, cell = row * width + col, north is row - 1; one flag
 *            byte per cell: 0 wall, else 1 (free) plus at most one of 2 (left area) / 4 (right area) / 8 (priest
 *            area), plus 16 (start cell). A start cell is in neither the left nor the right area.
 *   state    per env the agent cell, the heaven side (0 = the left area is heaven, 1 = the right) and elapsed;
 *            gp_get_state / gp_set_state exchange them as int32 [B] each (set clamps the cell to the grid and elapsed
 *            to [0, 65535] and keeps the low bit of the side; NULL leaves a field alone).
 *   actions  0 N, 1 E, 2 S, 3 W; [-4, 0) wraps as numpy indexing does; anything else is flagged (GP_E_DEVICE from
 *            gp_check) and clamped.
 *   draws    one Philox4x32-10 block per (env, step), counter (env, step_lo, step_hi, 0x6868656c) under the handle's
 *            key: y = x0 >> 1, the action slips iff y >= keep_thr, to (a + 1 + ((uint64)x1 * 3 >> 32)) & 3; a reset
 *            takes the start cell starts[((uint64)x2 * n_start) >> 32] (the start cells ascending) and the side
 *            x3 & 1. gp_reset draws from the block of its own step index.
 *   step     the move goes to the neighbour cell; off the grid or a wall: the agent stays, wall_reward; else
 *            step_reward. After the move a cell in the left or right area terminates, and the reward is replaced by
 *            heaven_reward if that area is the heaven side, else hell_reward. truncated = elapsed + 1 >= time_limit,
 *            independent of terminated. An episode end resets the env in the same step (draws of the same block).
 *   obs      int32 [B], taken after the autoreset: obs_base[cell] * 3 + signal, signal 0 outside the priest area,
 *            inside it 1 = heaven left, 2 = heaven right; n_obs = obs_base_n * 3.
 * GP_E_INVALID, naming the fault: a side outside [1, 16], a flag byte outside the set above, no start cell, a start
 * cell in the left or right area, an obs_base entry outside [0, obs_base_n), obs_base_n outside [1, 256], keep_thr
 * above 2^31, time_limit outside [1, 65535] (elapsed is kept in 16 bits). */
typedef struct gp_heavenhell_config {
  int32_t height, width;
  const uint8_t* flags;       /* [height * width] flag bytes                                          */
  const int32_t* obs_base;    /* [height * width] the obs base of each cell (the cell, a Hansen code) */
  int32_t obs_base_n;         /* obs_base values lie in [0, obs_base_n); at most 256                  */
  uint32_t keep_thr;          /* floor((1 - action_failure_probability) * 2^31); 2^31 = never slips   */
  int32_t time_limit;
  float heaven_reward, hell_reward, step_reward, wall_reward;
} gp_heavenhell_config;

/* Tabular POMDP (GP_KIND_POMDP; GP_RNG_PHILOX only: there is no reference stream, so GP_RNG_NUMPY / GP_RNG_REPLAY
 * return GP_E_UNSUPPORTED). A finite POMDP given as its tables (Cassandra's T / O / R); build-defined, no reference
 * counterpart. Everything that decides an outcome arrives as integers: no float arithmetic and no libm call of the
 * library decides a result (as with RockSample's sensor_thr).
 *   sizes    n_states S, n_actions A, n_obs O: 1 <= S <= 65,536, 1 <= A <= 64, 1 <= O <= 65,536. The library pads each
 *            stored row to 16-B quads with 2^31 (Sp = (S + 3) & ~3, Op = (O + 3) & ~3); S A Sp <= 2^28 and
 *            A S Op <= 2^28.
 *   tables   every threshold row holds cumulative probabilities scaled to 2^31, nondecreasing within [0, 2^31] and
 *            ending at 2^31 (gp_set_controller's rule).
 *   state    per env the state s, elapsed, and the last observation (a draw, not a function of the state: the handle
 *            keeps it); gp_get_state / gp_set_state exchange (state, elapsed, obs) as int32 [B] each (set clamps to
 *            [0, S), [0, 65535] and [0, O); NULL leaves a field alone).
 *   actions  [-A, 0) wraps as numpy indexing does; anything else is flagged (GP_E_DEVICE from gp_check) and clamped.
 *   draws    one Philox4x32-10 block per (env, step), counter (env, step_lo, step_hi, 0x706f6d64) under the handle's
 *            key; with y_i = x_i >> 1: s' = #{i < S : y0 >= trans_thr[s][a][i]}; if the episode goes on, obs =
 *            #{i < O : y1 >= obs_thr[a][s'][i]}; if the step ended it, s0 = #{i < S : y2 >= start_thr[i]} and obs =
 *            #{i < O : y3 >= reset_obs_thr[s0][i]}. gp_reset takes y2, y3 from the block of its own step index. Counts
 *            are clamped to S - 1 / O - 1.
 *   step     reward = reward[s][a][s'], terminated = terminal[s'], truncated = elapsed + 1 >= time_limit, independent
 *            of terminated. An episode end resets the env in the same step, and the step's obs is the reset obs.
 *   obs      int32 [B], the stored draw; n_obs = O.
 * GP_E_INVALID, naming the fault: a size outside its range, a NULL table, a padded table above 2^28 entries, a threshold
 * row that is not nondecreasing within [0, 2^31] or does not end at 2^31 (the table and the row are named), time_limit
 * outside [1, 65535] (elapsed is kept in 16 bits). */
typedef struct gp_pomdp_config {
  int32_t n_states, n_actions, n_obs;
  int32_t time_limit;
  const uint32_t* trans_thr;     /* [S][A][S] row (s, a): cumulative P(s' | s, a) * 2^31                  */
  const uint32_t* obs_thr;       /* [A][S][O] row (a, s'): cumulative P(o | a, s') * 2^31 (O: a : s' : o) */
  const uint32_t* start_thr;     /* [S] the start-state law                                              */
  const uint32_t* reset_obs_thr; /* [S][O] row s0: the law of the first obs given the start state        */
  const float* reward;           /* [S][A][S] indexed (s, a, s')                                         */
  const uint8_t* terminal;       /* [S] nonzero: entering the state ends the episode                     */
} gp_pomdp_config;

typedef struct gp_env gp_env;

const char* gp_last_error(void);
int gp_abi_version(void);

/* kind = GP_KIND_*, config points to the matching gp_*_config. Tables are built and uploaded
 * to `device` synchronously. rng_mode = GP_RNG_*. */
int gp_create(int kind, const void* config, int64_t num_envs, int device, int rng_mode, gp_env** out);
void gp_destroy(gp_env* env);

/* obs layout: dtype = GP_DTYPE_*, width = elements per env (1 for scalar obs). */
int gp_obs_info(const gp_env* env, int* dtype, int* width);
int64_t gp_num_envs(const gp_env* env);

/* numpy-compatible seeding: SeedSequence(entropy, spawn_key) -> PCG64 (and the Philox key).
 * entropy = little-endian uint32 words of a non-negative integer (numpy's convention).
 * Synchronous: both wait for the device (they clear the device error word, which queued launches may still write),
 * so a seed given after queued work takes effect after that work. */
int gp_seed_words(gp_env* env, const uint32_t* entropy, int n_entropy, const uint32_t* spawn_key, int n_spawn);
int gp_seed(gp_env* env, uint64_t seed);
/* raw PCG64 state: {state_hi, state_lo, inc_hi, inc_lo, has_uint32, uinteger}. get syncs. */
int gp_set_rng_state(gp_env* env, const uint64_t st[6]);
int gp_get_rng_state(gp_env* env, uint64_t st[6]);

/* Reset every env (reset()), writing the initial observation to `obs` (device). `obs` may sit at any address that is
 * aligned to its element type; exactly the B observations are written. */
int gp_reset(gp_env* env, void* obs, void* stream);

/* One batched step with same-step autoreset. actions: int32 [B] (discrete), float [B,2]
 * (continuous C-ROOMS) or float32 / float64 [B] (continuous CARFLAG, by its action_kind); obs as
 * gp_obs_info; rew float [B]; term/trunc uint8 [B]. */
int gp_step(gp_env* env, const void* actions, void* obs, float* rew, uint8_t* term, uint8_t* trunc,
            void* stream);

/* K consecutive steps. actions [K,B(,2)], outputs [K,B,...]. Philox mode, and numpy mode on GRID
 * (persistent kernel with a per-step grid exchange; 16-B aligned buffers, B % 4 == 0), fuse the K
 * steps in one launch with the state in registers; other cases issue K step launches.
 *
 * Caller buffers (gp_step, gp_rollout, gp_plan_*). Every buffer may sit at any address aligned to its element type (4 B
 * for int32 / float planes, 8 B for float64, any byte for uint8 planes), and B need not be a multiple of anything: the
 * kernels choose their store width per buffer and per step, and write exactly the documented bytes of the outputs and
 * never an input. Off 16 B a plane takes narrower stores (slower, same values). Exceptions:
 *   GRID in GP_RNG_NUMPY never refuses: when a buffer is off the boundaries above (windowed kernel: outputs on 16 B;
 *     fused kernel: actions, obs and rew on 16 B, term / trunc on 4 B, B % 4 == 0) the launch falls back, from the
 *     windowed to the fused kernel and from there to K single steps, each of which chooses again from the addresses of
 *     its own planes (one step needs no B % 4 == 0) between those kernels and the step kernels, with identical results.
 *     gp_query "launches_windowed" / "launches_fused" / "launches_step" count which one ran.
 *   CROOMS refuses (GP_E_INVALID, "crooms: misaligned action / obs / reward buffer") an obs base off 16 B and a
 *     continuous action base off 16 B (float64 [B,2]) or 8 B (float32 [B,2]); the planes of later steps need not keep
 *     that alignment, and rew / term / trunc go anywhere.
 *   ANTTAG with the vector obs refuses (GP_E_INVALID, "anttag: obs buffer must be 16-B aligned") an obs base off 16 B.
 * A refused call writes nothing and advances nothing (state, step index, metrics). */
int gp_rollout(gp_env* env, int K, const void* actions, void* obs, float* rew, uint8_t* term, uint8_t* trunc,
               void* stream);
/* A prepared gp_rollout (the agent loop's allocation-free hot path, bench.py's timed call): the arguments are
 * validated and bound once; gp_plan_run(plan) enqueues the K steps with nothing to marshal per call (one
 * pointer across the FFI instead of eight). The buffers must outlive the plan; gp_plan_destroy frees it. */
typedef struct gp_plan gp_plan;
int gp_plan_create(gp_env* env, int K, const void* actions, void* obs, float* rew, uint8_t* term, uint8_t* trunc,
                   void* stream, gp_plan** out);
int gp_plan_run(gp_plan* plan);
void gp_plan_destroy(gp_plan* plan);

/* ---- closed-loop rollouts: a tabular finite-state controller evaluated inside the rollout kernel ----
 * GRID in GP_RNG_PHILOX with a scalar obs (GP_OBS_HANSEN / GP_OBS_TABLE), ROCKSAMPLE (either obs), ANTTAG with the
 * index obs (obs_index = 1) in GP_RNG_PHILOX, TAXI with the Hansen obs (GP_OBS_HANSEN, one_hot 0 or 1) in
 * GP_RNG_PHILOX, HEAVENHELL (any obs base), POMDP, and CROOMS in GP_RNG_PHILOX with a scalar obs (GP_OBS_HANSEN /
 * GP_OBS_TABLE) and discrete actions (action_kind 4 or 8); every other kind, rng mode and obs kind:
 * GP_E_UNSUPPORTED. (No reference counterpart: the reference's agents act from the host, one step() per action.)
 *
 * The controller has M = n_nodes nodes (1..8; M = 1 is a memoryless policy obs -> action distribution). With A the
 * env's action count and L = A * M, thr_host is uint32 [M][n_obs][L] (host memory): row (node, obs) holds the
 * cumulative probabilities of the joint choice j = action * M + next_node, scaled to 2^31. Each row must be
 * nondecreasing, hold no entry above 2^31 and end at 2^31 (else GP_E_INVALID). n_obs is the size of the env's scalar
 * observation space; an obs >= n_obs met on the device is clamped and flagged (gp_check: GP_E_DEVICE).
 *
 * Per env-step, before the env transition: obs = the env's scalar obs of the state it is in (the reset obs, then the
 * post-autoreset obs of the previous step; computed from the state, never read from an output buffer); one
 * Philox4x32-10 block with counter (env, step_lo, step_hi, 0x67706f63) under the env draws' key, step being the same
 * host-tracked index the env's own draws of that step use (theirs carry 0x67706f21); y = x0 >> 1;
 * j = #{i < L : y >= thr[node][obs][i]}; action = j / M; after the transition node = j % M, or 0 if the step ended
 * the episode (terminated | truncated). The env's draws and the step index advance exactly as in gp_rollout: feeding
 * the emitted actions to gp_rollout on a twin handle reproduces every output and the final state bit for bit.
 * ROCKSAMPLE: the obs includes the reading of the previous step, which the handle keeps beside its state (every
 * step, open or closed loop, records it; gp_reset and gp_set_state make it NULL); the env draws carry 0x726f636b.
 * A = 5 + n_rocks need not be a multiple of 4: thr_host rows hold exactly L = A * M entries, and the library pads each
 * uploaded row to a multiple of 4 entries with 2^31, which no y reaches. A * M > 64 is GP_E_INVALID (the j / M
 * multiply is exact below 64).
 * ANTTAG: the obs is the index obs of the state word; the env draws carry 0x616e7431. A = 5, so L = 5 M <= 40 and rows
 * are padded to 16-B quads as ROCKSAMPLE's are. n_obs is the caller's (the obs space has size^2 * (size^2 + 1) values).
 * TAXI: obs_kind GP_OBS_HANSEN in GP_RNG_PHILOX, any map and num_passengers; GP_RNG_NUMPY, GP_RNG_REPLAY and the
 * raw-state obs (GP_OBS_TABLE) are GP_E_UNSUPPORTED, the message saying which applies (the raw-state obs is refused by
 * decision, not by the kernel: a fully observed Taxi is not pinned by any test yet). The obs is obs_of[s], the scalar
 * Hansen index of the state the env is in, whether the obs plane is scalar or one-hot (one_hot = 1: gp_rollout_controller
 * writes obs as uint8 [K,B,n_obs] rows, and the table is still indexed by the scalar). The env draws carry 0x74617869.
 * A = 5 (the action -1 no-op of gp_step is never emitted), so L = 5 M <= 40; rows hold exactly L entries and are padded
 * to 16-B quads as ROCKSAMPLE's are, and j is clamped to 5 M - 1, so a padding entry is never chosen. A completed task
 * whose episode continues (a goal move with num_passengers > 1) does not reset the node. n_obs is the caller's (the
 * Hansen obs space has 16 * n_locs * (n_locs + 1) values). The table is staged in LDS when the env's tables plus the
 * table fit the "ctrl_lds_max" budget below (5 x 5 map: M = 1), else read from global memory.
 * HEAVENHELL: the obs is that of the state word; the env draws carry 0x6868656c. A = 4, so rows hold exactly L = 4 M <= 32
 * entries, whole 16-B quads: nothing is padded. n_obs is the caller's (the obs space has obs_base_n * 3 values). The
 * table is staged in LDS behind the env's tables when both fit the "ctrl_lds_max" budget (the 48-value Hansen obs:
 * M = 2 is 3 KB, M = 5 is 18.75 KB; M = 8, 48 KB, needs the knob raised), else read from global memory.
 * CROOMS: GP_RNG_PHILOX, obs_kind GP_OBS_HANSEN or GP_OBS_TABLE, action_kind 4 (cardinal) or 8 (ordinal); GP_RNG_NUMPY,
 * GP_RNG_REPLAY, action_kind 0 (yx: no discrete action space) and the vector, window and continuous obs kinds (no
 * scalar obs) are GP_E_UNSUPPORTED, the message saying which applies. use_velocity, a random or fixed goal, a fixed
 * agent, cell_size, action_std, action_power and float32 / float64 I/O do not matter. The obs is computed from the
 * float64 position and the goal in registers exactly as the obs plane's value is; the controller's block always has
 * 10 Philox rounds; the env draws carry 0x63726f6f (noise) and 0x6d733121 (failure and reset draws). A = 4 or 8, so
 * rows hold exactly L = A M <= 64 entries, whole 16-B quads: nothing is padded (A = 8 with M = 8 sits at the j / M
 * multiply's limit). n_obs is the caller's (Hansen-4: 80 values, Hansen-8: 2,304, mdp: the valid cells, mdp_goal:
 * their square). The table is staged in LDS behind the env's tables when both fit the "ctrl_lds_max" budget (layout
 * "4": Hansen-4 with 4 actions and M = 1 is 1.25 KB; Hansen-8 with 8 actions is 72 KB at M = 1 and mdp_goal has
 * 40,000 obs values: global memory). An obs the env computes outside [0, n_obs) (cell_size > 1 puts positions on
 * wall cells, whose table value is -1, as in the reference) is clamped and flagged like any other.
 * POMDP: the obs is the stored last obs of the env (the reset's draw, then each step's); the env draws carry 0x706f6d64.
 * A is the model's (1..64), so L = A M <= 64; rows hold exactly L entries and are padded to 16-B quads as ROCKSAMPLE's
 * are where L is no multiple of 4. n_obs is the caller's (the obs space has O values). The table is staged in LDS behind
 * the env's LDS bytes (the model blob when it is in LDS itself, see "pomdp_lds_max" below, else nothing) when both fit
 * the "ctrl_lds_max" budget, else read from global memory: four combinations, one kernel instance each.
 *
 * gp_set_controller validates the table, uploads it synchronously and zeroes every node; thr_host = NULL removes the
 * controller. The nodes (uint8 [B], handle state) persist across calls; gp_reset zeroes them; gp_step / gp_rollout
 * (and, TAXI and CROOMS, gp_set_state) leave them alone.
 * gp_rollout_controller runs K steps in one launch. obs [K,B] int32, rew [K,B] float, term / trunc [K,B] uint8 as
 * gp_rollout; actions int32 [K,B]: the actions taken; nodes uint8 [K,B]: the node each action was chosen in. Every
 * output pointer may be NULL (not stored); with all of them NULL the call is a pure policy evaluation, read through
 * gp_metrics. GP_E_STATE before gp_reset or without a controller. The planes may sit at any element-aligned address
 * (as gp_rollout's), except CROOMS, whose kernel stores pairs of envs: obs, actions and rew off 8 B, or nodes, term and
 * trunc off 2 B, are refused (GP_E_INVALID, "crooms: misaligned obs / action / reward (8 B) or node / flag (2 B)
 * buffer"; NULL planes are not checked); the refused call writes and advances nothing.
 * gp_controller_nodes: get (device uint8 [B], may be NULL) receives the nodes, then set (device uint8 [B], may be
 * NULL) replaces them, both asynchronously on `stream`. A node >= n_nodes is clamped and flagged by the next
 * closed-loop launch. */
int gp_set_controller(gp_env* env, int n_nodes, int n_obs, const uint32_t* thr_host);
int gp_rollout_controller(gp_env* env, int K, void* obs, int32_t* actions, uint8_t* nodes, float* rew, uint8_t* term,
                          uint8_t* trunc, void* stream);
int gp_controller_nodes(gp_env* env, uint8_t* get, const uint8_t* set, void* stream);

/* ---- controller populations: P controllers run side by side, one score row per controller ----
 * GRID only, under the kind and mode gate of gp_set_controller (GP_RNG_PHILOX, GP_OBS_HANSEN / GP_OBS_TABLE); every
 * other kind: GP_E_UNSUPPORTED. (No reference counterpart.)
 *
 * Groups. A population is P = n_ctrl controllers that share n_nodes M, n_obs and the env's action count A. Env e is
 * driven by controller p = e / G, G = group_envs a positive multiple of 1024 (the envs of one rollout block, gp_query
 * "controller_group_multiple"), so that every block serves exactly one controller. P must equal ceil(B / G); the last
 * group is short when B is no multiple of G. thr_host is uint32 [P][M][n_obs][L], L = A * M: P tables of
 * gp_set_controller, back to back.
 *
 * Choice rule. Exactly the single-controller rule above with thr[p] in place of thr: the 0x67706f63 Philox block of
 * (env, step), y = x0 >> 1, j = #{i < L : y >= thr[p][node][obs][i]}, action = j / M, node = j % M or 0 at episode
 * end, the obs / node clamps and GP_DERR_CTRL. The draws are keyed by (env, step), so the trajectory of env e under a
 * population equals its trajectory on a same-seed twin handle with thr[e / G] installed by gp_set_controller.
 *
 * Scores. Each controller has five counters, accumulated by every closed-loop launch since they were last zeroed, in
 * this order: episodes, return_sum, length_sum, env_steps, discounted_return_sum. The first four mean for the group
 * what gp_metrics means for the batch: the rewards of all its env-steps, the lengths of the episodes that ended.
 * discounted_return_sum = sum of fl32(w * rew) over the group's env-steps, w the env's discount weight before the
 * step: at launch start w = W[elapsed] from the env's stored elapsed count; after each step w = 1.0f if the step ended
 * the episode, else fl32(w * gamma). W is a float32 table of 65,536 entries built on the host, W[0] = 1,
 * W[t] = fl32(W[t-1] * gamma), gamma a float32 in (0, 1]. Every product is rounded once (never contracted into an
 * FMA), so a launch that begins mid-episode, or after gp_set_state, weighs as one long launch would, with no per-env
 * state beyond the elapsed count. Each thread adds its float terms (return_sum: the float rewards) into doubles;
 * they are reduced per block in double and added into a slot only that block writes (no float or double atomics);
 * the host sums a group's slots in block order. Results are deterministic for a given B, G and launch sequence.
 * gp_metrics keeps its meaning and its bits: a population run reports what a twin running the same actions reports.
 *
 * gp_set_controller_population validates every row as gp_set_controller does (the message names the controller, the
 * node and the obs), uploads synchronously, zeroes every node and score, and replaces any installed controller or
 * population; thr_host = NULL removes whichever is installed. GP_E_INVALID: group_envs no positive multiple of 1024;
 * n_ctrl != ceil(B / group_envs); gamma outside (0, 1] or NaN; n_nodes outside [1, 8] or n_obs outside [1, 2^24];
 * more than 2^28 table entries in total; a bad row. gp_set_controller in turn removes a population. gp_reset zeroes
 * the scores together with the nodes. gp_rollout_controller runs whichever is installed; gp_controller_nodes is
 * unchanged. A block stages only its own controller's table in LDS, under gp_set_controller's budget rule applied to
 * one controller's bytes ("ctrl_lds_max" included).
 * gp_controller_scores: out (host, [P][5] doubles in the order above; cap_rows >= P rows, else GP_E_INVALID); syncs
 * and runs the device-error check of gp_metrics; clear != 0 zeroes the scores after reading. GP_E_STATE without a
 * population. */
int gp_set_controller_population(gp_env* env, int n_ctrl, int64_t group_envs, int n_nodes, int n_obs, float gamma,
                                 const uint32_t* thr_host);
int gp_controller_scores(gp_env* env, double* out, int cap_rows, int clear);

/* ---- controller statistics: visit counts and return-to-go sums per table cell, exact integers ----
 * The sufficient statistics of policy-gradient, Monte Carlo policy-iteration and EM steps over a controller's
 * parameters, from K stored closed-loop steps, in one launch. Every kind with closed-loop rollouts (GRID, ROCKSAMPLE,
 * ANTTAG, TAXI, HEAVENHELL, CROOMS, POMDP); the others: GP_E_UNSUPPORTED. (No reference counterpart.)
 *
 * The call is a pure function of the planes it is given: it reads nothing of the env's state and needs no gp_reset.
 * The handle supplies the shape: M = n_nodes and n_obs of the installed controller, A = the env's action count, and
 * P, G of an installed population (P = 1 otherwise). GP_E_STATE without a controller or population. All pointers are
 * device pointers on the handle's device; the call is asynchronous on `stream`.
 *   obs0 int32 [B]: the obs before the first of the K steps; obs int32 [K,B]: the obs after each step (the scalar obs
 *   plane of gp_rollout_controller); actions int32 [K,B]; nodes uint8 [K,B]: the node each action was chosen in;
 *   next_nodes uint8 [B]: the nodes after the K-th step (gp_controller_nodes right after the rollout); rew float
 *   [K,B]; term / trunc uint8 [K,B]; bootstrap float [B] or NULL (= 0): the value after the K-th step; gamma a
 *   float32 in (0, 1] (else, NaN included, GP_E_INVALID).
 *
 * Tables. counts and ret_q are int64 [P][M][n_obs][A][M+1], 8-byte aligned (else GP_E_INVALID). The call ADDS to
 * them; the caller zeroes them. Rows hold exactly A * (M + 1) entries, never the padded stride some kinds upload.
 *
 * Cell of a visit. Env e belongs to controller p = e / G. At step k: n = nodes[k][e]; o = k ? obs[k-1][e] : obs0[e],
 * the obs the choice was conditioned on; a = actions[k][e]; ended = term[k][e] | trunc[k][e]; the last index is M if
 * ended, else nodes[k+1][e] (next_nodes[e] for k = K - 1). Column M means "this choice ended the episode": the
 * rollouts zero the node at episode end, so the planes do not hold the drawn next node there, and it has no effect on
 * the return either; a gradient uses the action marginal for these visits.
 *
 * Return-to-go, float32. G_K = bootstrap ? bootstrap[e] : 0; for k = K-1 .. 0: G_k = ended ? rew[k][e]
 * : fl32(rew[k][e] + fl32(gamma * G_{k+1})): two roundings, never contracted into an FMA. Truncation stops the return
 * exactly as termination does (the discounted_return_sum convention of the population scores above).
 *
 * Accumulation. counts[cell] += 1; ret_q[cell] += rint(G_k * 2^20) as int64 (round to nearest even). The scaling by
 * 2^20 is exact, so the only rounding is to units of 2^-20: at most 2^-21 per visit. Integer sums do not depend on the
 * order of the adds: the tables are bit-reproducible and independent of the launch geometry (no float atomics).
 * Overflow: an entry of ret_q overflows once the sum of |G| over its visits reaches 2^43 (2^63 / 2^20); the caller
 * reads and clears the tables before that.
 *
 * Bad visits. A visit whose node is >= M, whose obs is outside [0, n_obs), whose action is outside [0, A), whose
 * non-ended next node is >= M, or with !(|G_k| < 2^31) (NaN and infinity included) is skipped, never clamped into
 * another cell, and flags the handle: gp_check then returns GP_E_DEVICE until the next seed. The G chain goes on
 * through the visit.
 *
 * Paths. When one controller's tables fit an LDS budget (12 B per cell; default 40 KiB, the knob "stats_lds_max"
 * below) each block keeps a private histogram in LDS and adds its non-zero cells to the tables at its end; otherwise
 * (and for K >= 2^22) every visit is a 64-bit integer atomic on the tables. The results are identical bit for bit.
 * gp_query "stats_lds": which one the handle's last call took (1 LDS, 0 global, -1 none yet). K = 0 is a no-op. */
int gp_controller_stats(gp_env* env, int K, const int32_t* obs0, const int32_t* obs, const int32_t* actions,
                        const uint8_t* nodes, const uint8_t* next_nodes, const float* rew, const uint8_t* term,
                        const uint8_t* trunc, const float* bootstrap, float gamma, int64_t* counts, int64_t* ret_q,
                        void* stream);

/* ---- belief filter and alpha-vector policies (POMDP only; every other kind: GP_E_UNSUPPORTED) ----
 * An exact Bayes filter kept per env on the device, a piecewise-linear policy over it, and a closed-loop rollout that
 * does env step, filter update and action choice in one launch. Build-defined (no reference counterpart); pinned bit
 * for bit to the numpy restatement tests/belief_oracle.py.
 *
 * Float laws. Built from the handle's integer thresholds: for a threshold row thr,
 *   p[i] = (float)(uint32)(thr[i] - thr[i-1]) * 2^-31, thr[-1] = 0 (one round-to-nearest conversion, an exact scale;
 *   numpy: np.diff(thr.astype(np.int64), prepend=0).astype(np.float32) * np.float32(2**-31)).
 * Tf[s][a][s'] from trans_thr, Zf[a][s'][o] from obs_thr, Rf[s][o] from reset_obs_thr, the default prior from start_thr.
 * Arithmetic. float32, every product and every sum rounded separately (no FMA), denormals kept, sums sequential in
 * ascending index from +0, division correctly rounded.
 * Filter step. Belief b[S], action a (wrapped / clamped exactly as gp_step does), stored obs o after the step,
 * ended = term | trunc.
 *   not ended: acc(s') = sum_s fl(b[s] Tf[s][a][s']); u(s') = terminal[s'] ? +0 : fl(Zf[a][s'][o] acc(s')) (a step that
 *              did not end tells the agent that s' is not terminal)
 *   ended:     u(s) = fl(prior[s] Rf[s][o]) (the stored obs is the reset obs)
 *   both:      n = sum_s u(s); b'(s) = fl(u(s) / n). If !(n > 0) or n is not finite: b' = prior, and the handle is
 *              flagged (gp_check: GP_E_DEVICE until the next seed).
 * gp_reset, and gp_belief_enable, set b by the ended rule from each env's stored obs. gp_step, gp_rollout,
 * gp_rollout_controller and gp_set_state leave the beliefs alone (as they leave controller nodes alone): advance them
 * with gp_belief_filter over the planes those calls wrote.
 * The device skips entries with Tf == 0 and whole columns with Zf == 0 or a terminal s': all operands are >= 0 and the
 * accumulators start at +0, so the bits are those of the dense loop (beliefs given through gp_belief_set must be
 * finite and >= 0 for that).
 * Policy. N vectors alpha[N][S] (finite, |alpha| <= 1e30) and vec_action[N] in [0, A): v_j = sum_s fl(b[s] alpha[j][s]);
 * j* is the first j that attains the maximum (replaced only on a strict >); the action is vec_action[j*], chosen from
 * the belief before the step, as a controller chooses from the obs before the step. No random draw is spent: feeding
 * the emitted actions to gp_rollout on a twin handle reproduces obs, rew, term, trunc, state and metrics bit for bit.
 * Limits. Belief: S <= 4,096. Policy: N <= 4,096 and N S <= 2^22. Beyond them GP_E_INVALID. A failed allocation
 * installs nothing.
 *
 * gp_belief_enable: prior float [S] (host) is used as given; NULL = the start law. Allocates two planes of S B floats,
 *   builds the float laws, sets every belief by the reset rule; synchronous. Calling it again replaces the prior.
 * gp_belief_disable frees them (a policy stays installed).
 * gp_belief_get / gp_belief_set: device float [B][S]; values are stored as given. GP_E_STATE without a filter.
 * gp_belief_filter advances the stored beliefs over K stored steps of planes [K,B] (actions int32, obs int32, term /
 *   trunc uint8; device), whoever wrote them: gp_rollout, gp_rollout_controller, or a replay. A pure function of its
 *   inputs and the stored beliefs; the env state is not read. Actions are wrapped and clamped as gp_step does
 *   (flagged like there), obs values outside [0, O) are clamped and flagged (gp_check: GP_E_DEVICE).
 * gp_set_belief_policy: alpha float [N][S], vec_action int32 [N] (host); N = 0 removes the policy.
 * gp_rollout_belief: K closed-loop steps in one launch. obs int32 [K,B], actions int32 [K,B], vec int32 [K,B] (j*),
 *   value float [K,B] (v_j*), rew float [K,B], term / trunc uint8 [K,B]; every output may be NULL. Accumulates
 *   gp_metrics as gp_rollout does. GP_E_STATE before gp_reset, without an enabled filter or without a policy. The
 *   beliefs after the launch are bit-equal to gp_belief_filter run over the planes it wrote.
 * Placement: when two LDS buffers of a block's 1,024 beliefs (8,192 S bytes, gp_query "belief_onchip_bytes") fit 60 KB
 * beside the model blob, and the knob "belief_onchip_max", the beliefs stay in LDS across the K steps of a launch;
 * else they are read and written in the global planes. Bit-equal. gp_query: "belief" (0 / 1), "belief_onchip",
 * "belief_vectors" (N of the installed policy). */
int gp_belief_enable(gp_env* env, const float* prior);
int gp_belief_disable(gp_env* env);
int gp_belief_get(gp_env* env, float* out, void* stream);
int gp_belief_set(gp_env* env, const float* in, void* stream);
int gp_belief_filter(gp_env* env, int K, const int32_t* actions, const int32_t* obs, const uint8_t* term,
                     const uint8_t* trunc, void* stream);
int gp_set_belief_policy(gp_env* env, int n_vectors, const float* alpha, const int32_t* vec_action);
int gp_rollout_belief(gp_env* env, int K, void* obs, int32_t* actions, int32_t* vec, float* value, float* rew,
                      uint8_t* term, uint8_t* trunc, void* stream);

/* ---- point-based value backup (POMDP only; every other kind: GP_E_UNSUPPORTED) ----
 * The step of point-based value iteration (Pineau, Gordon & Thrun 2003): from belief points and a set of
 * alpha-vectors, one new vector, its action and its value per point. Build-defined; pinned bit for bit to the numpy
 * restatement tests/pbvi_oracle.py. The float laws Tf, Zf and the arithmetic are the filter's (above): float32, every
 * product and every sum rounded separately (no FMA), sums sequential in ascending index from +0, the first maximiser
 * wins (replaced only on a strict >). reward[s][a][s'] and terminal[s'] are the handle's.
 * Rule. For a point b[S], the set alpha[N][S] and float32 gamma, for every action a:
 *   1. acc_a(s') = sum_s fl(b[s] Tf[s][a][s'])                                   (the filter step's acc)
 *   2. for every obs o: u(s') = terminal[s'] ? +0 : fl(Zf[a][s'][o] acc_a(s')); score_j = sum_s' fl(u(s') alpha[j][s']);
 *      j*(a, o) = the first maximiser over j
 *   3. w_a(s') = terminal[s'] ? +0 : sum_o fl(Zf[a][s'][o] alpha[j*(a, o)][s']), o ascending
 *   4. for every s: r_a(s) = sum_s' fl(Tf[s][a][s'] reward[s][a][s']); h_a(s) = sum_s' fl(Tf[s][a][s'] w_a(s'));
 *      beta_a(s) = fl(r_a(s) + fl(gamma h_a(s)))
 *   5. v_a = sum_s fl(b[s] beta_a(s)); a* = the first maximiser over a
 * Outputs per point: the vector beta_a*, the action a*, the value v_a*. A terminal s' is absorbing with value 0; the
 * time limit is not part of the value.
 * The device skips the terms with Tf == 0 or Zf == 0 and those of step 2 at a terminal s': with finite points, alpha
 * and reward they are +-0 and an accumulator that starts at +0 is never -0, so the bits are those of the dense loop.
 *
 * gp_belief_backup: points float [P][S] (device; finite, as gp_belief_set takes them; not normalised), alpha float
 *   [N][S] (host), alpha_out float [P][S], act_out int32 [P], value_out float [P] (device; each may be NULL). Reads
 *   the model and writes only its outputs: beliefs, env state, step counter, metrics and an installed policy are
 *   untouched. The vectors are copied before the call returns (it waits for the stream's earlier work first); the
 *   kernels run on `stream`. P = 0 is a no-op.
 *   GP_E_STATE without an enabled filter (the float laws live there). GP_E_INVALID, naming the fault: alpha not finite
 *   or above 1e30 in magnitude, gamma outside [0, 1] or NaN, N < 1, N > 4,096 or N S > 2^22, P < 0 or P > 2^20, or
 *   a scratch of 4 P A S + 2 P A O bytes above 2^30.
 *   The scratch and three compressed tables (rows of Tf, Zf by (a, o) and by (a, s')) are built at the first call,
 *   owned by the handle and freed by gp_belief_disable / gp_destroy; the scratch grows to the largest P seen.
 *   gp_query: "backup_scratch_bytes", "backup_tables" (0 / 1). */
int gp_belief_backup(gp_env* env, int n_points, const float* points, int n_vectors, const float* alpha, float gamma,
                     float* alpha_out, int32_t* act_out, float* value_out, void* stream);

/* ---- belief-set expansion (POMDP only; every other kind: GP_E_UNSUPPORTED) ----
 * The other half of point-based value iteration (Pineau, Gordon & Thrun 2003): for every belief point the successor
 * under the filter that lies farthest, in L1, from a reference set. Build-defined; pinned bit for bit to the numpy
 * restatement tests/expand_oracle.py. The float laws Tf, Zf, terminal and the arithmetic are the filter's (above):
 * float32, every product, difference, quotient and sum rounded separately (no FMA), sums sequential in ascending index
 * from +0, the first maximiser wins (replaced only on a strict >).
 * Rule. Points b[P][S] and a reference set q[Q][S] (NULL: the points themselves, Q = P) are finite and >= 0 and are
 * used as given, not normalised. For every point, action a and obs o:
 *   1. acc_a(s') = sum_s fl(b[s] Tf[s][a][s'])                                   (the backup's step 1)
 *   2. u(s') = terminal[s'] ? +0 : fl(Zf[a][s'][o] acc_a(s')); n(a, o) = sum_s' u(s'). The candidate (a, o) is live
 *      iff n > 0 and n is finite; its successor is b'(s') = fl(u(s') / n): the filter step of a step that did not
 *      end, so a live successor is the filter's belief bit for bit. Successors through an episode end are no
 *      candidates (they are the reset beliefs, which depend on no point).
 *   3. dist(a, o) = min over q of L1(b', q), L1 = sum_s |fl(b'[s] - q[s])|, s ascending from +0. All values are finite
 *      and >= 0, so the minimum is exact whatever its order.
 *   4. (a*, o*) = the first live candidate of the largest dist, a ascending, then o ascending.
 * Outputs per point: succ = b' of (a*, o*), dist, act = a*, obs = o*, mass = n(a*, o*). A point without a live
 * candidate: act = obs = -1, dist = mass = +0, a row of +0.
 * The device skips the terms of n with Zf == 0 and those at a terminal s' (u >= 0 and the accumulator starts at +0:
 * the bits of the dense loop); the L1 sums are dense.
 *
 * gp_belief_expand: points float [P][S], ref float [Q][S] or NULL (device), succ_out float [P][S], dist_out float [P],
 *   act_out / obs_out int32 [P], mass_out float [P] (device; each may be NULL). Asynchronous on `stream`: nothing is
 *   copied or waited for unless the scratch grows. Reads the model and writes only its outputs: beliefs, env state,
 *   step counter, metrics, an installed policy and the backup's results are untouched. P = 0 is a no-op.
 *   GP_E_STATE without an enabled filter. GP_E_INVALID, naming the fault: P < 0 or P > 2^20, with ref given Q < 1 or
 *   Q > 2^20, a scratch of 4 P A S + 4 P A O + 8 P A + 4 S Q bytes above 2^30, or P > 0 without points.
 *   The scratch (acc [P][A][S], shared with gp_belief_backup; n [P][A][O]; per (p, a) the best (dist, o); the reference
 *   set transposed [S][Q]) is owned by the handle, grows to the largest call seen and is freed by gp_belief_disable /
 *   gp_destroy; the (a, o) lists of Zf are the backup's tables. gp_query: "expand_scratch_bytes" (acc included).
 *   One stream per handle for the calls that share this scratch: gp_belief_expand and gp_belief_backup of one handle
 *   write the same acc, and a gp_belief_backup that grows it waits only for its own stream before it frees the old one.
 *   Queue them on one stream (or order the streams with events and let no call grow the scratch under another's
 *   queued work); calls of different handles share nothing. */
int gp_belief_expand(gp_env* env, int n_points, const float* points, int n_ref, const float* ref, float* succ_out,
                     float* dist_out, int32_t* act_out, int32_t* obs_out, float* mass_out, void* stream);

/* Canonical state (device pointers, int32 unless noted). GRID: agent cell, goal cell, elapsed
 * [B] each. TAXI: s, elapsed, n_dropoffs. CROOMS: agent yx f64[B,2], goal cell yx i32[B,2],
 * velocity f64[B,2], elapsed i32[B]. ANTTAG: agent cell, target cell, elapsed. ROCKSAMPLE: agent cell, good
 * mask, elapsed. HEAVENHELL: agent cell, heaven side (0 left, 1 right), elapsed. POMDP: state, elapsed, last obs.
 * CARFLAG: s f32[B,3]
 * (position, velocity, direction), elapsed i32[B], heavens f32[B] (+-1), priests f32[B] (+-0.5; set takes
 * both by sign).
 * TAXI packs n_dropoffs into 4 bits: gp_set_state clamps it to [0, 15] and a goal move from 15 leaves it at 15
 * (the reference counts on without bound). terminated is decided on the unsaturated count, so s, elapsed, the
 * rewards and both flags follow the reference for every count gp_set_state can store; only the count read back
 * by gp_get_state stops at 15. An episode started by reset never gets there (num_passengers <= 15 ends it). */
int gp_get_state(gp_env* env, void* a, void* b, void* c, void* d, void* stream);
int gp_set_state(gp_env* env, const void* a, const void* b, const void* c, const void* d, void* stream);

/* Replay mode: device pointers holding this step's pre-decided per-env draws (read by the next
 * gp_step). GRID: uniform k53 uint64 [B] (u = k*2^-53), goal index int32 [B], agent index
 * int32 [B] (indices into the valid-cell lists). TAXI: reset state int32 [B], passenger/dest
 * pair int32 [B] (p*n_locs+d). CROOMS: action noise f64 [B,2] (the value numpy's
 * normal(scale=action_std) returned), wall noise f64 [B,2] (normal(scale=0.5)), goal/agent index
 * int32 [B] each, uniform k53 uint64 [B] for discrete action failures. CARFLAG: uniform k53 uint64 [B] of
 * the reset position (x = -0.2 + 0.4 * k * 2^-53), heaven index int32 [B] into (-1, 1), priest index
 * int32 [B] into (-0.5, 0.5). */
int gp_set_replay(gp_env* env, const void* u, const void* i0, const void* i1, const void* f0, const void* f1);

/* Valid-cell lists (host copies) used by the index draws: which = 0 goal, 1 agent. */
int gp_valid_cells(const gp_env* env, int which, int32_t* out, int cap);

/* On-device episode statistics since the last gp_reset (syncs): {episodes, return_sum,
 * length_sum, env_steps}.
 *
 * The law of return_sum. It is the sum of the float32 rewards of all env-steps since gp_reset, accumulated in float64
 * from the thread on: each thread adds its rewards into a double ((double)rew, K steps x its envs x every tile its
 * block loops over), the block reduces in double (wave shuffles, the waves' partials in wave order), and the block's
 * total is added in double into the block's slot; gp_metrics sums the slots in slot order. The kernels that count
 * reward kinds instead (numpy-mode GRID: the windowed and the fused rollout) form (double)count * (double)reward once
 * per thread per launch, each product exact, and reduce the same way. No float32 partial sum exists anywhere. With N
 * env-steps of rewards r:
 *     |return_sum - exact sum| <= N * 2^-52 * sum|r|
 * (N - 1 additions of relative error 2^-53 each: under half of it). This is the bound the population scores
 * (gp_controller_scores) already carry per group. Dyadic rewards whose sums fit 53 bits give the exact sum.
 * The value is deterministic for a given B and launch sequence wherever a block owns its slot (every kernel but the
 * grid-wide numpy-mode TAXI and CROOMS steps, where more blocks than slots add their totals atomically: their last
 * bits may differ between runs, inside the bound). Rewards, obs, flags, env state and RNG do not depend on any of this.
 *
 * The counters. episodes, length_sum and env_steps are exact integers: 32-bit per thread within one launch, 64-bit
 * from the wave shuffle on (lanes, waves, slot, host). The per-thread limit of one launch is
 *     K * envs per thread (4) * tiles per block < 2^32
 * (CARFLAG's per-thread length sum is 64-bit already); a block's totals may pass 2^32 (a 1,024-env block at
 * K >= 2^22 with nothing stored). */
int gp_metrics(gp_env* env, double out[4]);

/* Syncs the handle's device and returns GP_E_DEVICE if any launch since the last seed failed on the
 * device (numpy-mode GRID: a persistent kernel's cross-block wait timed out; any kind: an action outside
 * [-n, n) was given, where the reference raises IndexError at msrooms.py:400 / rooms.py:208 /
 * extended_taxi.py:248 — the device clamps it and flags the handle; closed-loop rollouts: an obs or node outside the
 * controller table, clamped and flagged likewise; gp_controller_stats: a visit it had to skip), else GP_OK. The
 * asynchronous step/rollout calls cannot report such failures themselves; gp_metrics and
 * gp_get_rng_state run the same check. (No reference counterpart: numpy steps are synchronous.) */
int gp_check(gp_env* env);
/* Chooses, on this handle's device, the faster of interchangeable kernels for launches of K steps. Numpy-mode GRID
 * with both the windowed (wgrid_rollout) and the fused (grid_rollout_numpy) kernel eligible: their results are
 * identical, and which is faster at short launches differs between MI355X boards. Times `reps` K-step launches of
 * each on scratch actions / outputs from the current state, restores that state exactly (env state, stream
 * state, metrics), and sends K-step launches to the faster. *chosen (host, may be NULL) = 1 windowed, 0 fused,
 * -1 not applicable (other kinds / modes: a no-op). After gp_reset; syncs. (No reference counterpart.) */
int gp_autotune(gp_env* env, int K, int reps, int* chosen);
/* Introspection of a handle (host-only, no sync): key = "num_envs", "rng_mode", and for GRID
 * "fused_blocks" (persistent grid size of the fused numpy rollout, 0 = not eligible),
 * "fused_tiles_per_block", "fused_staged" (1 = LDS-staged outputs + store waves),
 * "fused_tile_envs", "philox_step" (GP_RNG_PHILOX: the counter's step index that the next reset / step draws
 * with; a K-step rollout, open or closed loop, advances it by K), "controller_nodes" (node count of the installed
 * controller, 0 = none), "controller_lds" (1 = its table is staged in LDS; ROCKSAMPLE, ANTTAG: always 0); ROCKSAMPLE,
 * ANTTAG, TAXI, HEAVENHELL, CROOMS and POMDP answer the last three too, TAXI also "controller_blocks" (persistent grid size of its closed-loop
 * rollout, 0 = no controller). POMDP also: "pomdp_lds" (1 = the model blob is staged in LDS, 0 = read from global
 * memory) and "pomdp_model_bytes" (the blob's size, what "pomdp_lds_max" is compared with). GRID also: "controller_population" (P of the installed population, 0 = none),
 * "controller_group_envs" (its G), "controller_group_multiple" (1024: what G must be a multiple of); with a population
 * "controller_nodes" and "controller_lds" answer for one controller's table. Every kind with closed-loop rollouts
 * also: "controller_n_obs" and "controller_actions" (n_obs of the installed table and the env's A: the shape
 * gp_controller_stats uses; GP_E_STATE without a controller), "stats_lds" (the path of the handle's last
 * gp_controller_stats launch: 1 LDS histogram, 0 global atomics, -1 none yet). GRID also: "launches_windowed",
 * "launches_fused", "launches_step" (GP_RNG_NUMPY: the launches since gp_create that took the windowed kernel, the
 * fused kernel and the step kernels, the last counting one per step; gp_autotune's scratch launches included). Unknown
 * keys return GP_E_INVALID. */
int gp_query(const gp_env* env, const char* key, int64_t* value);
/* ---- the normal sampler of rng_mode=philox (C-ROOMS noise), diagnostics ----
 * Replaces numpy's Generator.standard_normal (numpy/random/src/distributions/distributions.c,
 * random_standard_normal; the reference draws rng.normal at gym_po/envs/rooms/crooms.py:175-178, :324).
 * gp_standard_normal_words: numpy's algorithm (256-layer ziggurat) over the caller's u64 word stream, in
 *   order, on one device lane: words device u64[nwords], out device f64[n] (NaN for every normal whose
 *   words run out, mid-draw included),
 *   *used (host) = words consumed. Over numpy's raw PCG64 words it returns numpy's normals.
 * gp_normal_tail_counts: n normals of the philox-mode sampler keyed by `key` (gp_seed's Philox key words),
 *   never stored: counts[j] = #{|z| > thr[j]} (host arrays, nthr <= 8), moments = {sum z, sum z^2}. Syncs. */
int gp_standard_normal_words(const uint64_t* words, int64_t nwords, double* out, int64_t n, int64_t* used,
                             void* stream);
int gp_normal_tail_counts(uint64_t key, int64_t n, const double* thr, int nthr, uint64_t* counts,
                          double moments[2], void* stream);

/* Device-side start-state law of TAXI resets (host copy): P(state index k) over valid states. */
int gp_taxi_reset_distribution(const gp_env* env, double* out, int cap);

/* rgb_array frames of TAXI envs 0..n-1 (replaces TaxiVecEnv.render(idx=arange(n)), extended_taxi.py:289-309,
 * up to and including str_map_to_img's colouring and Hansen highlight :126-142 and tile_images
 * render_utils.py:63-88): uint8 RGB, frames tiled ceil(sqrt(n)) x ceil(n / ceil(sqrt(n))), zero padding.
 * dims (host, out) = {rows, cols, frame_rows, frame_cols}; out (device, rows*cols*3) may be NULL to query dims.
 * Other env kinds: GP_E_UNSUPPORTED (the reference renders none of them). Asynchronous on `stream`. */
int gp_taxi_render(gp_env* env, int n, int hansen_highlight, uint8_t* out, int32_t dims[4], void* stream);
/* cv2.resize(src, (dw, dh), interpolation=cv2.INTER_AREA) for uint8 sh x sw x ch device images when at least
 * one axis is enlarged (the resize of str_map_to_img, extended_taxi.py:144-146): OpenCV's generic resize path
 * restated (cv2 is absent here: parity unpinned). dst rows are dst_pitch bytes apart. Synchronises `stream`. */
int gp_resize_area_u8(const uint8_t* src, int sh, int sw, int ch, uint8_t* dst, int dh, int dw, int dst_pitch,
                      void* stream);

/* Kernel timing: when enabled, hipEvents bracket every launch of the env's step kernel on its
 * stream; gp_profile_read syncs and returns the summed kernel time (ms) and launch count since
 * the last read (then clears). Used by bench.py for the live roofline measurement. */
int gp_set_profiling(gp_env* env, int enable);
int gp_profile_read(gp_env* env, double* total_ms, int64_t* n_launches);
/* Same for the numpy-mode reset resolver kernel that follows each step kernel. */
int gp_profile_read_resolver(gp_env* env, double* total_ms, int64_t* n_launches);

/* ---- diagnostics (never needed in production; no reference counterpart) ----
 * Process-wide test / tuning knobs, read by gp_create (handles created earlier keep their values):
 *   "disable_fused" (GRID numpy mode: 1 = the two-kernel path only; CROOMS numpy mode: 1 = two launches per
 *   draw call), "no_staging" (1 = the fused kernel's env waves store outputs directly), "xmode" (fused exchange variant, default 1), "spin_limit" (polls
 *   before a cross-block wait gives up, 0 = default), "fault_block" (this block never publishes: forces
 *   the timeout path; -1 = off), "fused_tile" (GRID fused kernel envs per tile: 512, 1024 or 2048; 0 = by
 *   size), "no_spw" (GRID fused kernel: 1 = no speculative word windows), "generic_kernels" (CROOMS: 1 = the
 *   generic philox rollout even where a compile-time-specialised one exists), "no_wgrid" (GRID numpy mode: 1 =
 *   never the windowed kernel csrc/wgrid.hip), "wg_halo" (its window halo: 256 or 512 draws), "wg_bias" (added
 *   to its predicted reset count: forces window regenerations), "wg_tmode" (its timing-study variants, TM_* in
 *   csrc/wgrid.hip; results invalid for some), "ctrl_lds_max" (GRID, TAXI, HEAVENHELL and CROOMS closed-loop rollouts, read by
 *   gp_set_controller instead: the controller table is staged in LDS when the env's tables plus the table take at
 *   most this many bytes of LDS per block, at most 60 KB; 0 = always read from global memory, -1 = the default,
 *   32 KB), "persist_bpc" (TAXI / CROOMS / ANTTAG / ROCKSAMPLE / HEAVENHELL persistent rollouts: blocks per CU, 0 = every
 *   resident block; TAXI keeps the value it was created with for its closed-loop grid too), "stats_lds_max"
 *   (gp_controller_stats, read at every call instead: one controller's tables are accumulated in a block-private LDS
 *   histogram when they take at most this many bytes, 12 per cell, at most 60 KB; 0 = always global atomics, -1 = the
 *   default, 40 KiB), "pomdp_lds_max" (POMDP, read at gp_create: the model blob is staged in dynamic LDS when it takes
 *   at most this many bytes, at most 60 KB; 0 = always global memory, -1 = the default, 32 KB), "belief_onchip_max"
 *   (POMDP belief filter, read by gp_belief_enable: the beliefs stay in LDS across a launch when their two buffers,
 *   8,192 bytes per state, take at most this many bytes and fit 60 KB beside the model blob; 0 = always the global
 *   planes, -1 = the default, whatever fits).
 *   gp_debug_reset restores the defaults. Unknown key: GP_E_INVALID. */
int gp_debug_set(const char* key, int64_t value);
void gp_debug_reset(void);

/* ---- host-only helpers (no device needed) ---- */
/* PCG64 state {state_hi, state_lo, inc_hi, inc_lo, has_uint32, uinteger} that numpy's
 * Generator(PCG64(SeedSequence(entropy, spawn_key))) starts from. */
int gp_pcg64_seed_state(const uint32_t* entropy, int n_entropy, const uint32_t* spawn_key, int n_spawn,
                        uint64_t out[6]);
/* log1p(-u[i]) for u in [0, 1) exactly as the C library computes it (glibc 2.35 __log1p restated, the version
 * the C-ROOMS exact mode's ziggurat tail uses on the device: numpy's random_standard_normal calls npy_log1p ->
 * libm, distributions.c). Host-only check entry for the CPU tests. */
int gp_zig_log1p_neg(const double* u, double* out, int64_t n);
/* exp(x[i]) exactly as the C library computes it (glibc 2.35 __exp restated, csrc/gp_libm.h: the device copy the
 * exact-stream paths use where numpy calls libm's exp, e.g. random_binomial_inversion's q^n = exp(n log q),
 * distributions.c). fma != 0: the -mfma build glibc selects on CPUs with FMA (x86-64 ifunc), else the plain one.
 * Host-only check entry for the CPU tests. */
int gp_exp_libm(const double* x, double* out, int64_t n, int fma);
/* Philox4x32-R blocks (R = rounds: 7 or 10) of n counters ctr[6 i .. 6 i + 5] = {c0, c1, c2, c3, k0, k1} into
 * out[4 i .. 4 i + 3], computed by the header the philox-mode kernels inline (gp_common.h philox4x32<R>).
 * Host-only check entry for the CPU tests (oracle/philox.py is checked against it). */
int gp_philox_blocks(const uint32_t* ctr, int rounds, uint32_t* out, int64_t n);
/* Which build of the C library's exp this host runs (the one numpy's distributions get): 1 = the -mfma build,
 * 0 = the plain build, -1 = neither restatement matches (exact-stream exp-dependent branches then follow the FMA
 * build: parity unpinned). Decided once per process by comparing libm with both restatements where they differ;
 * the exact-stream kernels (Taxi numpy-mode resets, C-ROOMS exact-mode wedge) use that build on the device. */
int gp_exp_host_variant(void);
/* P(argmax = k), k < m, for Multinomial(n, uniform over m) counts, ties to the first index:
 * the law of TaxiVecEnv._reset_mask (extended_taxi.py:344-352). Returns m. */
int gp_argmax_multinomial_distribution(int m, int n, double* out);

#ifdef __cplusplus
}
#endif
#endif /* GYM_PO_AMD_H */
