// rocksample.hip — RockSample (GP_KIND_ROCKSAMPLE; Smith & Simmons, "Heuristic Search Value Iteration for POMDPs",
// UAI 2004). The reference names the env (gym_po/envs/rocksample/rocksample.py: the Obs enum NULL / GOOD / BAD, the
// ACTION enum NORTH, EAST, SOUTH, WEST, SAMPLE and a constructor signature) and builds none of it: the rules below
// are this build's, as Ant-Tag's are (tests/rocksample_oracle.py restates them in numpy).
//
// Spec:
//   grid     H x W cells, 1 <= H, W <= 16, cell = y * W + x, north is y - 1
//   rocks    k (1..16) distinct cells, the same for every env of a handle; per env a k-bit good mask (bit i set =
//            rock i is good); the agent starts every episode on init_cell
//   actions  A = 5 + k: 0 N, 1 E, 2 S, 3 W, 4 SAMPLE, 5 + i = CHECK rock i; [-A, 0) wraps as numpy indexing does,
//            anything else is flagged GP_DERR_ACTION and clamped
//   step     elapsed += 1, reading = NULL (0); then by action
//              N / S / W  move if the target is inside the grid (step_reward), else stay (wall_reward)
//              E          the same, except that from the last column the agent exits: terminated, exit_reward
//              SAMPLE     on rock i's cell: good_reward if bit i is set, else bad_reward, and bit i is cleared;
//                         on a cell with no rock: empty_reward
//              CHECK i    check_reward; y = x0 >> 1, correct = y < thr[cell][i]; the reading is GOOD (1) if
//                         (bit i) == correct, else BAD (2)
//   end      truncated = elapsed >= time_limit (gymnasium TimeLimit), independent of terminated; on either the env
//            resets in the same step (agent on init_cell, mask = x1 & (2^k - 1), elapsed = 0) and the step's obs is
//            that of the reset state with reading NULL
//   draws    one Philox4x32-10 block per (env, step), counter (env, step_lo, step_hi, TAG): x0 the check, x1 the
//            reset mask (every rock good with probability 1/2, independently). Lanes that neither check nor end an
//            episode skip the block: nothing of it would be used.
//   sensor   thr uint32 [H*W][k] comes with the config (lowered in Python: floor(0.5 (1 + 2^(-d / d0)) 2^31), d the
//            Euclidean distance to the rock): kernel and oracle share one table, no libm call decides a result
//   obs      int32 [B]: the reading, or cell * 3 + reading (obs_cell)
// State per env: 8 B in two uint32 planes, cm = cell | mask << 8 | last reading << 24 and el = elapsed (16 bits
// used), each loaded and stored once per launch as 16-B quads and kept in two registers across the K steps. One
// 64-bit word per env would need 32-B accesses per thread for the same bytes; one uint32 cannot hold cell (8 bits),
// mask (16) and a 16-bit elapsed. The last reading is no part of the canonical state (gp_get_state): it is the part
// of the previous obs the closed-loop rollouts condition on, kept so that split launches continue exactly.
#include <algorithm>
#include <cstring>
#include <vector>

#include "gp_ctrl.h"
#include "gp_internal.h"

namespace {

constexpr int TPB = 256;
constexpr int EPT = 4;
constexpr int EPB = TPB * EPT;
constexpr int WAVES = TPB / 64;
constexpr int MAX_SIDE = 16;   // cells fit 8 bits of the packed state
constexpr int MAX_ROCKS = 16;  // the good mask fits 16 bits
constexpr int NMOVE = 4, A_SAMPLE = 4, A_CHECK = 5;
constexpr uint32_t TAG = 0x726f636bu;  // 'rock'
constexpr uint8_t NO_ROCK = 0xFF;

struct RsDev {
  int32_t B, ntiles, W, H, k, ncells, A;
  uint32_t divm;  // ceil(2^16 / W): cell / W == (cell * divm) >> 16 for cells < 256
  int32_t init_cell, obs_cell, time_limit;
  uint32_t kmask;  // 2^k - 1
  float r_exit, r_good, r_bad, r_empty, r_check, r_step, r_wall;
  uint32_t key0, key1;
  const uint8_t* tabs;  // [ncells][k] uint32 sensor thresholds | [ncells] rock index at the cell (u8, NO_ROCK = none)
  int32_t off_rock, tab_bytes;
  uint32_t* cm;  // [B] cell | mask << 8 | last reading << 24
  uint32_t* el;  // [B] elapsed
  MetricSlot* mslot;
  uint32_t* derr;  // device error word (GP_DERR_*)
};

__device__ __forceinline__ void stage_tables(const RsDev& p, uint8_t* lds) {
  const uint4* src = (const uint4*)p.tabs;
  uint4* dst = (uint4*)lds;
  for (int i = threadIdx.x; i < p.tab_bytes / 16; i += TPB) dst[i] = src[i];
}

__device__ __forceinline__ Philox4 rs_block(const RsDev& p, int env, uint64_t step, uint32_t tag) {
  return philox4x32_10((uint32_t)env, (uint32_t)step, (uint32_t)(step >> 32), tag, p.key0, p.key1);
}

__device__ __forceinline__ int32_t rs_obs(const RsDev& p, uint32_t cm) {
  const int32_t reading = (int32_t)(cm >> 24);
  return p.obs_cell ? (int32_t)(cm & 0xFFu) * 3 + reading : reading;
}

__device__ __forceinline__ StepOut rs_env_step(const RsDev& p, const uint8_t* lds, uint32_t& cm, uint32_t& el, int a,
                                               int env, bool live, uint64_t step, double& rsum, uint32_t& eps,
                                               uint32_t& lens) {
  const uint32_t* thr = reinterpret_cast<const uint32_t*>(lds);
  const uint8_t* rock_at = lds + p.off_rock;
  int cell = (int)(cm & 0xFFu);
  uint32_t mask = (cm >> 8) & 0xFFFFu, reading = 0, e1 = el + 1u;
  // an action outside [-A, A) is flagged as numpy indexing would raise, then clamped
  if (live && action_out_of_range(a, p.A)) flag_bad_action(p.derr);
  if (a < 0) a += p.A;
  a = min(max(a, 0), p.A - 1);
  StepOut o;
  o.term = 0;
  if (a < NMOVE) {
    const int y = (int)(((uint32_t)cell * p.divm) >> 16), x = cell - y * p.W;
    const int ny = y + (a == 2) - (a == 0), nx = x + (a == 1) - (a == 3);
    if (a == 1 && x == p.W - 1) {
      o.term = 1;
      o.rew = p.r_exit;
    } else if (ny >= 0 && ny < p.H && nx >= 0 && nx < p.W) {
      cell = ny * p.W + nx;
      o.rew = p.r_step;
    } else {
      o.rew = p.r_wall;
    }
  } else if (a == A_SAMPLE) {
    const uint32_t rk = rock_at[cell];
    if (rk != NO_ROCK) {
      o.rew = (mask >> rk) & 1u ? p.r_good : p.r_bad;
      mask &= ~(1u << rk);
    } else {
      o.rew = p.r_empty;
    }
  } else {
    o.rew = p.r_check;
  }
  o.trunc = e1 >= (uint32_t)p.time_limit ? 1 : 0;
  const bool done = o.term | o.trunc;
  if (!live) return o;
  rsum += (double)o.rew;
  if (a >= A_CHECK || done) {  // the only users of the step's block
    const Philox4 z = rs_block(p, env, step, TAG);
    if (done) {
      eps += 1u;
      lens += e1;
      cell = p.init_cell;
      mask = z.x[1] & p.kmask;
      e1 = 0;
    } else {
      const int i = a - A_CHECK;
      const uint32_t correct = (z.x[0] >> 1) < thr[cell * p.k + i] ? 1u : 0u;
      reading = ((mask >> i) & 1u) == correct ? 1u : 2u;
    }
  }
  cm = (uint32_t)cell | (mask << 8) | (reading << 24);
  el = e1;
  return o;
}

// K steps of every env: a persistent grid-stride loop over 1,024-env tiles, 4 consecutive envs per thread with their
// state in registers across the K steps. CTRL = false: the actions come from `act` [K, B], loaded one step ahead.
// CTRL = true (gp_rollout_controller): each action is drawn by the installed controller from the env's obs and node
// (gp_ctrl.h; the rows are read from global memory, L1 / L2 hot); `aout` / `nodes` receive the actions and nodes.
// Every output pointer may be null (not stored): gp_rollout passes all of obs / rew / term / trunc.
template <bool CTRL>
__global__ __launch_bounds__(TPB) void rs_rollout(RsDev p, CtrlDev c, int K, uint64_t step0,
                                                  const int32_t* __restrict__ act, int32_t* __restrict__ obs,
                                                  int32_t* __restrict__ aout, uint8_t* __restrict__ nodes,
                                                  float* __restrict__ rew, uint8_t* __restrict__ term,
                                                  uint8_t* __restrict__ trunc) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  stage_tables(p, lds);
  __syncthreads();
  double rsum = 0.0;
  uint32_t eps = 0, lens = 0, nst = 0;
  for (int tile = blockIdx.x; tile < p.ntiles; tile += gridDim.x) {
    const int env0 = tile * EPB + threadIdx.x * EPT;
    uint32_t cm[EPT], el[EPT];
    load4<uint32_t>(p.cm, env0, p.B, cm);
    load4<uint32_t>(p.el, env0, p.B, el);
    uint8_t nd[EPT] = {0, 0, 0, 0};
    int a_nxt[EPT] = {0, 0, 0, 0};
    if constexpr (CTRL) {
      load4<uint8_t>(c.node, env0, p.B, nd);
#pragma unroll
      for (int i = 0; i < EPT; ++i)
        ctrl_clamp_node(nd[i], c.M, env0 + i < p.B, p.derr);
    } else {
      if (K > 0) load4<int32_t>(act, env0, p.B, a_nxt);
    }
    for (int k = 0; k < K; ++k) {
      const size_t off = (size_t)k * p.B;
      const uint64_t step = step0 + (uint64_t)k;
      int32_t a[EPT];
      uint32_t jj[EPT] = {0, 0, 0, 0};
      uint8_t n4[EPT];
      if constexpr (CTRL) {
        const uint32_t lreal = (uint32_t)(p.A * c.M);  // entries of a row before its padding to 16-B quads
#pragma unroll
        for (int i = 0; i < EPT; ++i) {
          const int env = env0 + i;
          const uint32_t y = env < p.B ? rs_block(p, env, step, CTRL_TAG).x[0] >> 1 : 0u;
          jj[i] = ctrl_pick(c.thr, nd[i], c.n_obs, c.L, lreal, (uint32_t)rs_obs(p, cm[i]), y, env < p.B, p.derr);
          a[i] = (int32_t)ctrl_action(jj[i], c.inv_m);
          n4[i] = nd[i];
        }
      } else {
#pragma unroll
        for (int i = 0; i < EPT; ++i) a[i] = a_nxt[i];
        if (k + 1 < K) load4<int32_t>(act + off + p.B, env0, p.B, a_nxt);  // one step ahead
      }
      float r[EPT];
      uint8_t tm[EPT], tr[EPT];
      int32_t ob[EPT];
#pragma unroll
      for (int i = 0; i < EPT; ++i) {
        const bool live = env0 + i < p.B;
        const StepOut o = rs_env_step(p, lds, cm[i], el[i], a[i], env0 + i, live, step, rsum, eps, lens);
        r[i] = o.rew;
        tm[i] = o.term;
        tr[i] = o.trunc;
        ob[i] = rs_obs(p, cm[i]);
        nst += live ? 1u : 0u;
        if constexpr (CTRL)  // episode end: node 0
          nd[i] = (o.term | o.trunc) ? (uint8_t)0 : (uint8_t)ctrl_node(jj[i], (uint32_t)a[i], c.M);
      }
      if constexpr (CTRL) {
        if (aout) store4<int32_t>(aout + off, env0, p.B, a);
        if (nodes) store4<uint8_t>(nodes + off, env0, p.B, n4);
      }
      if (rew) store4<float>(rew + off, env0, p.B, r);
      if (term) store4<uint8_t>(term + off, env0, p.B, tm);
      if (trunc) store4<uint8_t>(trunc + off, env0, p.B, tr);
      if (obs) store4<int32_t>(obs + off, env0, p.B, ob);
    }
    store4<uint32_t>(p.cm, env0, p.B, cm);
    store4<uint32_t>(p.el, env0, p.B, el);
    if constexpr (CTRL) store4<uint8_t>(c.node, env0, p.B, nd);
  }
  block_metrics<WAVES>(p, rsum, eps, lens, nst);
}

__global__ __launch_bounds__(TPB) void rs_reset(RsDev p, uint64_t step, int32_t* __restrict__ obs) {
  for (int env = blockIdx.x * TPB + threadIdx.x; env < p.B; env += gridDim.x * TPB) {
    const uint32_t cm = (uint32_t)p.init_cell | ((rs_block(p, env, step, TAG).x[1] & p.kmask) << 8);
    p.cm[env] = cm;
    p.el[env] = 0u;
    obs[env] = rs_obs(p, cm);
  }
}

__global__ void rs_get_state(RsDev p, int32_t* agent, int32_t* rocks, int32_t* el) {
  const int env = blockIdx.x * TPB + threadIdx.x;
  if (env >= p.B) return;
  const uint32_t cm = p.cm[env];
  if (agent) agent[env] = (int32_t)(cm & 0xFFu);
  if (rocks) rocks[env] = (int32_t)((cm >> 8) & 0xFFFFu);
  if (el) el[env] = (int32_t)p.el[env];
}
// A null pointer leaves its field alone. The last reading becomes NULL: the state is a new one, nothing was read in it.
__global__ void rs_set_state(RsDev p, const int32_t* agent, const int32_t* rocks, const int32_t* el) {
  const int env = blockIdx.x * TPB + threadIdx.x;
  if (env >= p.B) return;
  uint32_t cm = p.cm[env] & 0xFFFFFFu;
  if (agent) cm = (cm & ~0xFFu) | (uint32_t)min(max(agent[env], 0), p.ncells - 1);
  if (rocks) cm = (cm & 0xFFu) | (((uint32_t)rocks[env] & p.kmask) << 8);
  p.cm[env] = cm;
  if (el) p.el[env] = (uint32_t)min(max(el[env], 0), 65535);
}

// ------------------------------------------------------------------ host backend ----
struct RockSampleBackend : EnvBackend {
  RsDev d{};
  CtrlHost ctrl;
  int grid = 1;
  uint64_t philox_step = 0;
  DevBuf b_tabs, b_cm, b_el, b_slot;
  DevErr derr;

  int build(const gp_rocksample_config* cfg);
  int seed(const RngHost& r, const uint32_t key[2]) override {
    rng = r;
    d.key0 = key[0];
    d.key1 = key[1];
    philox_step = 0;
    return derr.clear();
  }
  int check() override { return derr.check("rocksample"); }
  int set_rng_state(const RngHost&) override {
    gp_set_error("rocksample: no numpy stream (build-defined env; philox mode)");
    return GP_E_UNSUPPORTED;
  }
  int get_rng_state(RngHost*) override {
    gp_set_error("rocksample: no numpy stream (build-defined env; philox mode)");
    return GP_E_UNSUPPORTED;
  }
  int query(const char* key, int64_t* v) const override {
    if (!strcmp(key, "philox_step")) *v = (int64_t)philox_step;
    else if (!strcmp(key, "controller_nodes")) *v = ctrl.dev.M;  // node count of the installed controller (0 = none)
    else if (!strcmp(key, "controller_lds")) *v = 0;         // the table is read from global memory
    else return EnvBackend::query(key, v);
    return GP_OK;
  }
  int reset(void* obs, hipStream_t s) override {
    GP_HIP_CHECK(hipMemsetAsync(d.mslot, 0, sizeof(MetricSlot) * grid, s));
    if (int e = ctrl.reset_nodes(B, s)) return e;
    const unsigned nb = (unsigned)std::min<int64_t>((B + TPB - 1) / TPB, 65536);
    hipLaunchKernelGGL(rs_reset, dim3(nb), dim3(TPB), 0, s, d, philox_step, (int32_t*)obs);
    ++philox_step;
    GP_HIP_CHECK(hipGetLastError());
    has_reset = true;
    return GP_OK;
  }
  int rollout(int K, const void* act, void* obs, float* rew, uint8_t* term, uint8_t* trunc, hipStream_t s) override {
    if (!has_reset) {
      gp_set_error("step() before reset()");
      return GP_E_STATE;
    }
    timer.begin(s);
    hipLaunchKernelGGL(rs_rollout<false>, dim3(grid), dim3(TPB), d.tab_bytes, s, d, CtrlDev{}, K, philox_step,
                       (const int32_t*)act, (int32_t*)obs, (int32_t*)nullptr, (uint8_t*)nullptr, rew, term, trunc);
    timer.end(s);
    philox_step += (uint64_t)K;
    GP_HIP_CHECK(hipGetLastError());
    return GP_OK;
  }
  int step(const void* act, void* obs, float* rew, uint8_t* term, uint8_t* trunc, hipStream_t s) override {
    return rollout(1, act, obs, rew, term, trunc, s);
  }
  int get_state(void* a, void* b, void* c, void*, hipStream_t s) override {
    hipLaunchKernelGGL(rs_get_state, dim3((unsigned)((B + TPB - 1) / TPB)), dim3(TPB), 0, s, d, (int32_t*)a,
                       (int32_t*)b, (int32_t*)c);
    GP_HIP_CHECK(hipGetLastError());
    return GP_OK;
  }
  int set_state(const void* a, const void* b, const void* c, const void*, hipStream_t s) override {
    hipLaunchKernelGGL(rs_set_state, dim3((unsigned)((B + TPB - 1) / TPB)), dim3(TPB), 0, s, d, (const int32_t*)a,
                       (const int32_t*)b, (const int32_t*)c);
    GP_HIP_CHECK(hipGetLastError());
    has_reset = true;
    return GP_OK;
  }
  int controller_shape(CtrlShape* out) const override { return ctrl_shape_of(ctrl.dev.M, ctrl.dev.n_obs, d.A, 0, 0, derr.ptr(), out); }
  int set_controller(int n_nodes, int n_obs, const uint32_t* thr_host) override;
  int rollout_controller(int K, void* obs, int32_t* act, uint8_t* nodes, float* rew, uint8_t* term, uint8_t* trunc,
                         hipStream_t s) override {
    if (int e = ctrl.ready(has_reset)) return e;
    timer.begin(s);
    hipLaunchKernelGGL(rs_rollout<true>, dim3(grid), dim3(TPB), d.tab_bytes, s, d, ctrl.dev, K, philox_step,
                       (const int32_t*)nullptr, (int32_t*)obs, act, nodes, rew, term, trunc);
    timer.end(s);
    philox_step += (uint64_t)K;
    GP_HIP_CHECK(hipGetLastError());
    return GP_OK;
  }
  int controller_nodes(uint8_t* get, const uint8_t* set, hipStream_t s) override { return ctrl.nodes(get, set, B, s); }
  int metrics(double out[4]) override {
    GP_HIP_CHECK(hipDeviceSynchronize());
    std::vector<MetricSlot> m(grid);
    GP_HIP_CHECK(hipMemcpy(m.data(), d.mslot, sizeof(MetricSlot) * grid, hipMemcpyDeviceToHost));
    sum_metric_slots(m.data(), m.size(), out);
    return check();
  }
};

// A = 5 + k is no multiple of 4 in general: CtrlHost::install pads the rows. The table is read from global memory.
int RockSampleBackend::set_controller(int n_nodes, int n_obs, const uint32_t* thr_host) {
  if (!thr_host) return ctrl.clear();
  return ctrl.install("gp_set_controller", d.A, n_nodes, n_obs, thr_host, B);
}

int RockSampleBackend::build(const gp_rocksample_config* cfg) {
  const int H = cfg->height, W = cfg->width, k = cfg->n_rocks, nc = H * W;
  if (H < 1 || H > MAX_SIDE || W < 1 || W > MAX_SIDE) {
    gp_set_error("rocksample: grid %d x %d outside [1, %d] per side", H, W, MAX_SIDE);
    return GP_E_INVALID;
  }
  if (k < 1 || k > MAX_ROCKS) {
    gp_set_error("rocksample: %d rocks outside [1, %d]", k, MAX_ROCKS);
    return GP_E_INVALID;
  }
  if (!cfg->rocks || !cfg->sensor_thr) {
    gp_set_error("rocksample: rocks and sensor_thr are required");
    return GP_E_INVALID;
  }
  if (cfg->init_cell < 0 || cfg->init_cell >= nc) {
    gp_set_error("rocksample: init_cell %d off the %d x %d grid", cfg->init_cell, H, W);
    return GP_E_INVALID;
  }
  if (cfg->time_limit < 1 || cfg->time_limit > 65535) {
    gp_set_error("rocksample: time_limit %d outside [1, 65535] (elapsed is kept in 16 bits)", cfg->time_limit);
    return GP_E_INVALID;
  }
  std::vector<uint8_t> rock_at(nc, NO_ROCK);
  for (int i = 0; i < k; ++i) {
    const int c = cfg->rocks[i];
    if (c < 0 || c >= nc) {
      gp_set_error("rocksample: rock %d at cell %d off the %d x %d grid", i, c, H, W);
      return GP_E_INVALID;
    }
    if (rock_at[c] != NO_ROCK) {
      gp_set_error("rocksample: rocks %d and %d share cell %d", (int)rock_at[c], i, c);
      return GP_E_INVALID;
    }
    rock_at[c] = (uint8_t)i;
  }
  const size_t nthr = (size_t)nc * k;
  for (size_t i = 0; i < nthr; ++i)
    if (cfg->sensor_thr[i] > (1u << 31)) {
      gp_set_error("rocksample: sensor_thr[%zu][%zu] = %u above 2^31", i / k, i % k, cfg->sensor_thr[i]);
      return GP_E_INVALID;
    }
  std::vector<uint8_t> blob((nthr * 4 + 15) & ~(size_t)15, 0);
  memcpy(blob.data(), cfg->sensor_thr, nthr * 4);
  d.off_rock = (int32_t)blob.size();
  blob.resize(blob.size() + (((size_t)nc + 15) & ~(size_t)15), NO_ROCK);
  memcpy(blob.data() + d.off_rock, rock_at.data(), nc);
  d.tab_bytes = (int32_t)blob.size();
  int e;
  if ((e = b_tabs.upload(blob))) return e;
  d.tabs = b_tabs.as<uint8_t>();
  d.B = (int32_t)B;
  d.ntiles = (int32_t)((B + EPB - 1) / EPB);
  d.H = H;
  d.W = W;
  d.k = k;
  d.ncells = nc;
  d.A = A_CHECK + k;
  d.divm = (65536u + (uint32_t)W - 1u) / (uint32_t)W;
  d.init_cell = cfg->init_cell;
  d.obs_cell = cfg->obs_cell != 0;
  d.time_limit = cfg->time_limit;
  d.kmask = (1u << k) - 1u;
  d.r_exit = cfg->exit_reward;
  d.r_good = cfg->good_reward;
  d.r_bad = cfg->bad_reward;
  d.r_empty = cfg->empty_reward;
  d.r_check = cfg->check_reward;
  d.r_step = cfg->step_reward;
  d.r_wall = cfg->wall_reward;
  obs_dtype = GP_DTYPE_I32;
  obs_width = 1;
  if ((e = b_cm.alloc((size_t)B * 4 + 16)) || (e = b_el.alloc((size_t)B * 4 + 16))) return e;
  d.cm = b_cm.as<uint32_t>();
  d.el = b_el.as<uint32_t>();
  hipDeviceProp_t prop;
  GP_HIP_CHECK(hipGetDeviceProperties(&prop, device));
  int occ = 0, occ_c = 0;
  GP_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, rs_rollout<false>, TPB, d.tab_bytes));
  GP_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ_c, rs_rollout<true>, TPB, d.tab_bytes));
  occ = std::min(occ, occ_c);  // one grid (and one set of metric slots) for both
  grid = persistent_grid(d.ntiles, prop.multiProcessorCount, occ);
  persist_grid = grid;
  persist_occ = occ;
  if ((e = b_slot.alloc(sizeof(MetricSlot) * grid))) return e;
  d.mslot = b_slot.as<MetricSlot>();
  if ((e = derr.alloc())) return e;
  d.derr = derr.ptr();
  return GP_OK;
}

}  // namespace

std::unique_ptr<EnvBackend> make_rocksample_backend(const gp_rocksample_config* cfg, int64_t B, int device,
                                                    int rng_mode, int* err) {
  if (rng_mode != GP_RNG_PHILOX) {
    gp_set_error("rocksample: rng_mode %s does not exist for this build-defined env (no reference stream); use philox",
                 rng_mode == GP_RNG_NUMPY ? "numpy" : "replay");
    *err = GP_E_UNSUPPORTED;
    return nullptr;
  }
  if (B < 1 || B > (int64_t)1 << 30) {
    gp_set_error("rocksample: num_envs %lld out of range", (long long)B);
    *err = GP_E_INVALID;
    return nullptr;
  }
  if (hipSetDevice(device) != hipSuccess) {
    gp_set_error("rocksample: hipSetDevice(%d) failed", device);
    *err = GP_E_HIP;
    return nullptr;
  }
  auto be = std::make_unique<RockSampleBackend>();
  be->B = B;
  be->device = device;
  be->rng_mode = rng_mode;
  int e = be->build(cfg);
  if (e) {
    *err = e;
    return nullptr;
  }
  return be;
}
