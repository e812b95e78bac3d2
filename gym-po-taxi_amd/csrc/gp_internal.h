// gp_internal.h — handle layout shared by the per-kind backends (not part of the C ABI).
#pragma once
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/gym_po_amd.h"
#include "gp_common.h"

// numpy Generator(PCG64) state as the host sees it.
struct RngHost {
  u128 state = 0, inc = 1;
  uint32_t has_u32 = 0, uinteger = 0;
};

// SeedSequence(entropy, spawn_key).generate_state(n, uint64) — numpy bit_generator.pyx restated.
std::vector<uint64_t> seed_sequence_u64(const std::vector<uint32_t>& entropy, const std::vector<uint32_t>& spawn_key,
                                        int n_words64);
RngHost pcg64_from_seed(const std::vector<uint32_t>& entropy, const std::vector<uint32_t>& spawn_key);
// P(argmax = k) for Multinomial(n, uniform over m) counts, ties -> first (taxi reset law).
std::vector<double> argmax_multinomial_distribution(int m, int n);
// Radix-64 jump tables (JT_LEVELS x 64) for increment `inc`.
std::vector<PcgJump> build_jump_tables(u128 inc);

// Diagnostic knobs (gp_debug_set), read by the backends at gp_create.
struct GpDebugKnobs {
  int disable_fused = 0, no_staging = 0, xmode = 1, fault_block = -1;
  int fused_tile = 0;       // GRID fused kernel: envs per tile (512 / 1024 / 2048); 0 = chosen by size
  uint32_t spin_limit = 0;  // 0 = the kernel's default
  int generic_kernels = 0;  // CROOMS: 1 = never the compile-time-specialised philox rollout (A/B and parity tests)
  int no_spw = 0;           // GRID fused kernel: 1 = no speculative word windows (A/B and parity tests)
  int no_wgrid = 0;         // GRID: 1 = never the windowed kernel (wgrid.hip): the older fused kernel instead
  int wg_halo = 0;          // GRID windowed kernel: window halo (256 or 512 draws); 0 = default
  int wg_bias = 0;          // GRID windowed kernel: added to the predicted reset count (forces window misses)
  int wg_tmode = 0;         // GRID windowed kernel: timing-study variants (wgrid.hip TM_*); some give wrong results
  int wg_kmax = -1;         // GRID: longest launch (steps) on the windowed kernel; longer ones on the fused kernel (-1 default)
  int xg_min_envs = -1;      // CROOMS exact mode: largest B on the one-workgroup kernel (-1 = crooms.hip XG_MIN_ENVS)
  int xg_ppt_min = -1;       // CROOMS exact mode: normal calls above this many 256-position blocks take 4 per thread
  int xg_spb_min = -1;       // CROOMS exact mode: env kernels above this many env blocks take 4 per workgroup
  int taxi_npg_min = -1;    // TAXI numpy mode: largest B on the one-workgroup kernel (-1 = taxi.hip NPG_MIN_ENVS)
  int64_t fused_step = -1;  // GRID: the fused kernel's tag counter (GridCtl::step) set at every seed (-1 = kept)
  int wg_block_envs = 0;    // GRID windowed kernel: the smallest envs per block to use (0 = the smallest that fits)
  int wg_fill_simd = 0;     // GRID windowed kernel: per-SIMD window-row deltas, 4 signed nibbles (0 = WG_FILL_SIMD)
  int64_t wg_fill_wave = 0; // GRID windowed kernel: per-wave deltas on top, 8 signed nibbles (wave 0 lowest)
  int ctrl_lds_max = -1;    // GRID / TAXI / HEAVENHELL / CROOMS closed-loop rollouts: dynamic LDS bytes per block up to which the controller table is staged in LDS (0 = never; -1 = gp_ctrl.h CTRL_LDS_BUDGET; at most 60 KB); read by gp_set_controller
  int pomdp_lds_max = -1;   // POMDP: bytes up to which the model blob (the T / O / R tables) is staged in dynamic LDS (0 = never: global memory; -1 = gp_ctrl.h CTRL_LDS_BUDGET; at most 60 KB); read at gp_create
  int stats_lds_max = -1;  // gp_controller_stats: LDS bytes per block up to which one controller's tables are accumulated in a block-private LDS histogram (0 = never: global atomics; -1 = ctrl_stats.hip STATS_LDS_BUDGET; at most 60 KB); read at every call
  int belief_onchip_max = -1;  // POMDP belief filter: LDS bytes per block (8,192 per state: two buffers of 1,024 envs) up to which the beliefs of a block's envs stay in LDS across a launch (0 = never: global planes; -1 = whatever fits 60 KB beside the model blob); read by gp_belief_enable
  int persist_bpc = 0;      // TAXI / CROOMS / ANT-TAG / ROCKSAMPLE / HEAVENHELL streaming rollouts: blocks per CU (0 = every resident block, persistent_grid); TAXI keeps the value of gp_create for its closed-loop grid (set_controller)
};
const GpDebugKnobs& gp_debug_knobs();

// Grid of a persistent grid-stride tile loop (the Taxi / C-ROOMS / Ant-Tag rollouts: K steps per tile with the
// tile's state in registers): every resident block (occupancy x CUs), capped by the tiles. An equal number of
// tiles per block measured slower (round 6, profiles/r06_persist_grid.txt: C-ROOMS at 2^21 envs 17.4 us/step with
// 1,024 blocks of 4 tiles vs 15.7 with 1,280 blocks of 3-4; Ant-Tag 14.6 vs 13.9): per-wave latency, not the
// SIMDs' issue rate, bounds these loops, so more resident waves win even with a ragged last round. The knob
// persist_bpc forces the blocks per CU (A/Bs).
inline int persistent_grid(int ntiles, int cus, int occ) {
  const int forced = gp_debug_knobs().persist_bpc;
  const int bpc = forced > 0 ? forced : (occ < 1 ? 1 : (occ > 8 ? 8 : occ));
  const int g = cus * bpc;
  return ntiles < g ? (ntiles > 0 ? ntiles : 1) : g;
}

// What gp_controller_stats (ctrl_stats.hip) needs to know of a handle: the shape of the installed controller or
// population and the handle's device error word. Filled by EnvBackend::controller_shape.
struct CtrlShape {
  int M = 0, n_obs = 0, A = 0;  // nodes and obs values of the installed table, actions of the env
  int P = 1;                    // controllers of an installed population (1: a single controller)
  int64_t G = 0;                // envs per group of a population, a multiple of 1024 (0: a single controller)
  uint32_t* derr = nullptr;     // device error word (GP_DERR_*)
};

// Per-kind backend interface; gp_env owns one.
// hipEvent pairs around the step-kernel launches (gp_set_profiling / gp_profile_read).
struct KernelTimer {
  bool on = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;
  size_t used = 0;
  double acc_ms = 0;
  int64_t acc_n = 0;
  void begin(hipStream_t s);
  void end(hipStream_t s);
  int read(double* ms, int64_t* n);
  ~KernelTimer();
};

struct EnvBackend {
  KernelTimer timer;   // the step kernel (K1 / fused rollout)
  KernelTimer timer2;  // the reset resolver (K2, numpy mode)
  int64_t B = 0;
  int device = 0;
  int rng_mode = GP_RNG_NUMPY;
  int persist_grid = 0;  // blocks of the persistent rollout grid (Taxi / C-ROOMS / Ant-Tag; gp_query "persist_blocks")
  int persist_occ = 0;   // resident blocks per CU of that rollout kernel (the occupancy query)
  int obs_dtype = GP_DTYPE_I32;
  int obs_width = 1;
  bool has_reset = false;
  RngHost rng;                 // host copy of the numpy-mode RNG state (authoritative until uploaded)
  uint32_t philox_key[2] = {0, 0};
  virtual ~EnvBackend() {}
  virtual int seed(const RngHost& r, const uint32_t key[2]) = 0;
  virtual int set_rng_state(const RngHost& r) = 0;
  virtual int get_rng_state(RngHost* r) = 0;
  virtual int reset(void* obs, hipStream_t s) = 0;
  virtual int step(const void* act, void* obs, float* rew, uint8_t* term, uint8_t* trunc, hipStream_t s) = 0;
  virtual int rollout(int K, const void* act, void* obs, float* rew, uint8_t* term, uint8_t* trunc, hipStream_t s);
  virtual int get_state(void* a, void* b, void* c, void* d, hipStream_t s) = 0;
  virtual int set_state(const void* a, const void* b, const void* c, const void* d, hipStream_t s) = 0;
  virtual int set_replay(const void* u, const void* i0, const void* i1, const void* f0, const void* f1) {
    gp_set_error("replay mode not supported by this env kind");
    return GP_E_UNSUPPORTED;
  }
  // Closed-loop rollouts (gp_set_controller / gp_rollout_controller / gp_controller_nodes): GRID in philox mode,
  // ROCKSAMPLE, ANTTAG with the index obs in philox mode, TAXI with the Hansen obs in philox mode, HEAVENHELL,
  // CROOMS with a scalar obs and discrete actions in philox mode, POMDP.
  // What the seven share lives in gp_ctrl.h (CtrlHost: install / clear, the LDS staging rule, the node plane, the
  // rollout_controller precondition; the device helpers of the pick); a kind keeps its refusals, its kernels and
  // the sizing of its closed-loop grid.
  virtual int set_controller(int n_nodes, int n_obs, const uint32_t* thr_host) {
    gp_set_error("controllers are not supported by this env kind");
    return GP_E_UNSUPPORTED;
  }
  virtual int rollout_controller(int K, void* obs, int32_t* act, uint8_t* nodes, float* rew, uint8_t* term,
                                 uint8_t* trunc, hipStream_t s) {
    gp_set_error("closed-loop rollouts are not supported by this env kind");
    return GP_E_UNSUPPORTED;
  }
  virtual int controller_nodes(uint8_t* get, const uint8_t* set, hipStream_t s) {
    gp_set_error("controllers are not supported by this env kind");
    return GP_E_UNSUPPORTED;
  }
  // Controller populations (gp_set_controller_population / gp_controller_scores): GRID only (CtrlHost::install with
  // n_ctrl tables; the group checks, the weight table and the score slots are grid.hip's).
  virtual int set_controller_population(int n_ctrl, int64_t group_envs, int n_nodes, int n_obs, float gamma,
                                        const uint32_t* thr_host) {
    gp_set_error("controller populations are not supported by this env kind (GRID only)");
    return GP_E_UNSUPPORTED;
  }
  virtual int controller_scores(double* out, int cap_rows, int clear) {
    gp_set_error("controller populations are not supported by this env kind (GRID only)");
    return GP_E_UNSUPPORTED;
  }
  // Controller statistics (gp_controller_stats): the seven kinds with closed-loop rollouts answer the shape of what is
  // installed (GP_E_STATE: nothing is); the call itself is kind-independent (ctrl_stats.hip).
  virtual int controller_shape(CtrlShape* out) const {
    gp_set_error("controllers are not supported by this env kind");
    return GP_E_UNSUPPORTED;
  }
  int ctrl_shape_of(int M, int n_obs, int A, int P, int64_t G, uint32_t* derr, CtrlShape* out) const {
    if (!M) {
      gp_set_error("gp_controller_stats without a controller (gp_set_controller / gp_set_controller_population)");
      return GP_E_STATE;
    }
    *out = CtrlShape{M, n_obs, A, P > 0 ? P : 1, P > 0 ? G : 0, derr};
    return GP_OK;
  }
  // Belief filter and alpha-vector policies (gp_belief_* / gp_set_belief_policy / gp_rollout_belief): POMDP only.
  int no_belief() const {
    gp_set_error("belief filters are not supported by this env kind (POMDP only)");
    return GP_E_UNSUPPORTED;
  }
  virtual int belief_enable(const float* prior) { return no_belief(); }
  virtual int belief_disable() { return no_belief(); }
  virtual int belief_get(float* out, hipStream_t s) { return no_belief(); }
  virtual int belief_set(const float* in, hipStream_t s) { return no_belief(); }
  virtual int belief_filter(int K, const int32_t* act, const int32_t* obs, const uint8_t* term, const uint8_t* trunc,
                            hipStream_t s) {
    return no_belief();
  }
  virtual int set_belief_policy(int n_vec, const float* alpha, const int32_t* vec_action) { return no_belief(); }
  virtual int rollout_belief(int K, void* obs, int32_t* act, int32_t* vec, float* value, float* rew, uint8_t* term,
                             uint8_t* trunc, hipStream_t s) {
    return no_belief();
  }
  // Point-based value backup (gp_belief_backup; pomdp_backup.hip): POMDP only.
  virtual int belief_backup(int P, const float* points, int N, const float* alpha, float gamma, float* alpha_out,
                            int32_t* act_out, float* value_out, hipStream_t s) {
    return no_belief();
  }
  // Belief-set expansion (gp_belief_expand; pomdp_expand.hip): POMDP only.
  virtual int belief_expand(int P, const float* points, int Q, const float* ref, float* succ_out, float* dist_out,
                            int32_t* act_out, int32_t* obs_out, float* mass_out, hipStream_t s) {
    return no_belief();
  }
  int stats_path = -1;  // the last gp_controller_stats launch: 1 = LDS histogram, 0 = global atomics (gp_query "stats_lds")
  virtual int valid_cells(int which, int32_t* out, int cap) const { return 0; }
  virtual int metrics(double out[4]) = 0;  // (the sum of the kind's MetricSlots: gp_common.h sum_metric_slots)
  // Syncs and reports device-side failures of earlier launches (GP_E_DEVICE); kinds without
  // cross-block waits have none.
  virtual int check() { return GP_OK; }
  // Introspection (gp_query): kernel geometry of this handle.
  virtual int query(const char* key, int64_t* v) const {
    if (!strcmp(key, "num_envs")) *v = B;
    else if (!strcmp(key, "rng_mode")) *v = rng_mode;
    else if (!strcmp(key, "persist_blocks")) *v = persist_grid;
    else if (!strcmp(key, "persist_occupancy")) *v = persist_occ;
    else if (!strcmp(key, "stats_lds")) *v = stats_path;
    else if (!strcmp(key, "controller_n_obs") || !strcmp(key, "controller_actions")) {
      CtrlShape c;
      if (int e = controller_shape(&c)) return e;
      *v = key[11] == 'n' ? c.n_obs : c.A;
    } else {
      gp_set_error("gp_query: unknown key '%s'", key);
      return GP_E_INVALID;
    }
    return GP_OK;
  }
  virtual int debug_stamps(unsigned long long* out, int cap) { return 0; }
  // gp_autotune: pick the faster of interchangeable kernels for K-step launches on this device (no-op here)
  virtual int autotune(int K, int reps, int* chosen) {
    if (chosen) *chosen = -1;
    return GP_OK;
  }
  virtual int reset_distribution(double* out, int cap) const {
    gp_set_error("no reset distribution for this env kind");
    return GP_E_UNSUPPORTED;
  }
  // rgb_array frames of envs 0..n-1, tiled (gp_taxi_render)
  virtual int render(int n, int hansen, uint8_t* out, int32_t dims[4], hipStream_t s) {
    gp_set_error("rendering is not available for this env kind (the reference does not render it either)");
    return GP_E_UNSUPPORTED;
  }
  size_t obs_elem_size() const { return obs_dtype == GP_DTYPE_U8 ? 1 : (obs_dtype == GP_DTYPE_F64 ? 8 : 4); }
  virtual size_t rollout_action_bytes_per_env() const { return 4; }
};

// ctrl_stats.hip: the one launch of gp_controller_stats (K >= 1, arguments validated by the caller); *lds_path receives
// 1 if it took the LDS histogram, 0 if global atomics.
int ctrl_stats_launch(const CtrlShape& c, int64_t B, int K, const int32_t* obs0, const int32_t* obs,
                      const int32_t* actions, const uint8_t* nodes, const uint8_t* next_nodes, const float* rew,
                      const uint8_t* term, const uint8_t* trunc, const float* bootstrap, float gamma, int64_t* counts,
                      int64_t* ret_q, int* lds_path, hipStream_t s);

std::unique_ptr<EnvBackend> make_grid_backend(const gp_grid_config* cfg, int64_t B, int device, int rng_mode, int* err);
std::unique_ptr<EnvBackend> make_taxi_backend(const gp_taxi_config* cfg, int64_t B, int device, int rng_mode, int* err);
std::unique_ptr<EnvBackend> make_crooms_backend(const gp_crooms_config* cfg, int64_t B, int device, int rng_mode,
                                                int* err);
std::unique_ptr<EnvBackend> make_anttag_backend(const gp_anttag_config* cfg, int64_t B, int device, int rng_mode,
                                                int* err);
std::unique_ptr<EnvBackend> make_carflag_backend(const gp_carflag_config* cfg, int64_t B, int device, int rng_mode,
                                                 int* err);
std::unique_ptr<EnvBackend> make_rocksample_backend(const gp_rocksample_config* cfg, int64_t B, int device,
                                                    int rng_mode, int* err);
std::unique_ptr<EnvBackend> make_heavenhell_backend(const gp_heavenhell_config* cfg, int64_t B, int device,
                                                    int rng_mode, int* err);
std::unique_ptr<EnvBackend> make_pomdp_backend(const gp_pomdp_config* cfg, int64_t B, int device, int rng_mode,
                                               int* err);

// Small device-buffer owner.
struct DevBuf {
  void* p = nullptr;
  size_t n = 0;
  DevBuf() {}
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
  int alloc(size_t bytes) {
    if (p) (void)hipFree(p);
    p = nullptr;
    n = bytes;
    if (bytes == 0) return GP_OK;
    GP_HIP_CHECK(hipMalloc(&p, bytes));
    GP_HIP_CHECK(hipMemset(p, 0, bytes));
    return GP_OK;
  }
  template <class T>
  int upload(const std::vector<T>& v) {
    int e = alloc(v.size() * sizeof(T) + 16);
    if (e) return e;
    if (!v.empty()) GP_HIP_CHECK(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return GP_OK;
  }
  template <class T>
  T* as() const {
    return (T*)p;
  }
};

// The per-handle device error word of the kinds without a control block (taxi, ant-tag, C-ROOMS philox /
// replay): kernels OR GP_DERR_* bits into it; check() syncs, reads it and reports GP_E_DEVICE.
struct DevErr {
  DevBuf buf;
  int alloc() { return buf.alloc(16); }
  uint32_t* ptr() const { return buf.as<uint32_t>(); }
  int clear();                       // on seed: a new stream, earlier errors no longer apply
  int check(const char* kind) const;  // GP_OK or GP_E_DEVICE with gp_last_error() text
};

