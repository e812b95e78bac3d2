// heavenhell.hip — grid Heaven-Hell (GP_KIND_HEAVENHELL): a build-defined grid restatement of the task of the
// reference's AntHeavenHellEnv (gym_po/envs/ant_heaven_hell.py), as Ant-Tag's grid is of its tag task. The reference
// env is a MuJoCo ant, which is out of scope here, so parity with it is unpinned by construction: the device is
// pinned bit for bit to the numpy restatement of the rules below (tests/heavenhell_oracle.py), and that one to a
// scalar statement in plain integers.
//
// Sources of the rules: ant_heaven_hell.py:35-40 (the heaven / hell / priest points and the radius 2.0), :99-119 (the
// reset: the heaven side is a fair coin), :121-137 (the step: +-1 and done inside either area, the side revealed only
// within the priest's radius, the ant's own position not in the obs); the walls and the start box are those of
// assets/ant_heaven_hell.xml:72-100 and ant_heaven_hell.py:74 (lowered to cells by the Python helper
// heaven_hell_maze; this file only sees flag bytes).
//
// Spec:
//   maze     H x W cells, 1 <= H, W <= 16, cell = row * W + col, north is row - 1; one flag byte per cell:
//            1 free, 2 left area, 4 right area, 8 priest area, 16 start (areas and starts are free cells; a start
//            cell is in neither the left nor the right area; at least one start cell)
//   state    one uint32 per env: cell | side << 8 | elapsed << 16 (side: 0 = heaven is the left area, 1 = the right;
//            time_limit <= 65,535)
//   actions  0 N, 1 E, 2 S, 3 W; [-4, 0) wraps as numpy indexing does, anything else is flagged GP_DERR_ACTION and
//            clamped
//   draws    one Philox4x32-10 block per (env, step), counter (env, step_lo, step_hi, TAG) under the handle's key:
//              y = x0 >> 1: the action slips iff y >= keep_thr (keep_thr = floor((1 - p) 2^31), lowered on the host;
//                           2^31 = never)
//              a slipped action becomes (a + 1 + ((uint64)x1 * 3 >> 32)) & 3 (one of the three others, uniform)
//              reset: the start cell is starts[((uint64)x2 * n_start) >> 32] (starts ascending), the side x3 & 1
//            With keep_thr == 2^31 the lanes that do not end an episode skip the block: nothing of it would be used.
//   step     the move goes to the neighbour cell; off the grid or not free: the agent stays, wall_reward; else
//            step_reward. After the move a cell in the left or right area terminates, and the reward is replaced by
//            heaven_reward if that area is the heaven side, else hell_reward.
//   end      truncated = elapsed + 1 >= time_limit (gymnasium TimeLimit), independent of terminated; on either the
//            env resets in the same step from the same block, and the step's obs is that of the reset state
//   obs      int32 [B], a function of the state word alone: base[cell] * 3 + signal, signal 0 outside the priest
//            area, inside it 1 = heaven left, 2 = heaven right. base is a per-cell table of the config (the cell, or
//            its Hansen-4 code): the kernel has one obs path.
// Geometry (that of rs_rollout / anttag_rollout_idx): a persistent grid-stride loop over 1,024-env tiles, 256 threads,
// 4 consecutive envs per thread with their state words in registers across the K steps, the per-cell tables in
// dynamic LDS (at most 768 B), actions loaded one step ahead, 16-B / 4-B quad accesses with an element-wise fallback.
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
constexpr int MAX_SIDE = 16;  // cells fit 8 bits of the state word
constexpr int NACT = 4;
constexpr uint32_t TAG = 0x6868656cu;  // 'hhel'
constexpr uint32_t F_FREE = 1u, F_LEFT = 2u, F_RIGHT = 4u, F_PRIEST = 8u, F_START = 16u;
constexpr uint32_t F_ALL = 31u, TOP = 1u << 31;

struct HhDev {
  int32_t B, ntiles, W, H, ncells, n_start;
  uint32_t divm;      // ceil(2^16 / W): cell / W == (cell * divm) >> 16 for cells < 256
  uint32_t keep_thr;  // the action slips iff (x0 >> 1) >= keep_thr; 2^31: never
  int32_t time_limit;
  float r_heaven, r_hell, r_step, r_wall;
  uint32_t key0, key1;
  const uint8_t* tabs;  // [ncells] flags | [ncells] obs base | [n_start] start cells ascending; each padded to 16 B
  int32_t off_base, off_start, tab_bytes;
  uint32_t* st;  // [B] cell | side << 8 | elapsed << 16
  MetricSlot* mslot;
  uint32_t* derr;  // device error word (GP_DERR_*)
};

__device__ __forceinline__ Philox4 hh_block(const HhDev& p, int env, uint64_t step, uint32_t tag) {
  return philox4x32_10((uint32_t)env, (uint32_t)step, (uint32_t)(step >> 32), tag, p.key0, p.key1);
}

// `tabs`: the table blob, in LDS (rollouts) or global memory (reset)
__device__ __forceinline__ int32_t hh_obs(const HhDev& p, const uint8_t* tabs, uint32_t st) {
  const uint32_t cell = st & 0xFFu, side = (st >> 8) & 1u;
  const uint32_t signal = (tabs[cell] & F_PRIEST) ? 1u + side : 0u;
  return (int32_t)((uint32_t)tabs[p.off_base + cell] * 3u + signal);
}

__device__ __forceinline__ uint32_t hh_reset_word(const HhDev& p, const uint8_t* tabs, uint32_t x2, uint32_t x3) {
  const uint32_t si = (uint32_t)(((uint64_t)x2 * (uint32_t)p.n_start) >> 32);
  return (uint32_t)tabs[p.off_start + si] | ((x3 & 1u) << 8);
}

__device__ __forceinline__ StepOut hh_env_step(const HhDev& p, const uint8_t* lds, uint32_t& st, int a, int env,
                                               bool live, uint64_t step, double& rsum, uint32_t& eps, uint32_t& lens) {
  int cell = (int)(st & 0xFFu);
  const uint32_t side = (st >> 8) & 1u;
  uint32_t e1 = (st >> 16) + 1u;
  // the four rewards as values, read before any branch: a reward chosen by selecting between the fields of the
  // by-value argument struct makes the compiler keep a copy of them in the private segment (24 B of scratch)
  const float r_step = p.r_step, r_wall = p.r_wall, r_heaven = p.r_heaven, r_hell = p.r_hell;
  // an action outside [-4, 4) is flagged as numpy indexing would raise, then clamped
  if (live && action_out_of_range(a, NACT)) flag_bad_action(p.derr);
  if (a < 0) a += NACT;
  a = min(max(a, 0), NACT - 1);
  const bool slippery = p.keep_thr < TOP;  // uniform
  uint32_t x2 = 0u, x3 = 0u;  // the reset's words of the step's block
  if (slippery) {
    const Philox4 z = hh_block(p, env, step, TAG);
    if ((z.x[0] >> 1) >= p.keep_thr) a = (a + 1 + (int)(((uint64_t)z.x[1] * 3u) >> 32)) & 3;
    x2 = z.x[2];
    x3 = z.x[3];
  }
  const int y = (int)(((uint32_t)cell * p.divm) >> 16), x = cell - y * p.W;
  const int ny = y + (a == 2) - (a == 0), nx = x + (a == 1) - (a == 3);
  const bool inside = ny >= 0 && ny < p.H && nx >= 0 && nx < p.W;
  const int ncell = inside ? ny * p.W + nx : cell;  // (in bounds of the table either way)
  StepOut o;
  if (inside && (lds[ncell] & F_FREE)) {
    cell = ncell;
    o.rew = r_step;
  } else {
    o.rew = r_wall;
  }
  const uint32_t f = lds[cell];
  o.term = (f & (F_LEFT | F_RIGHT)) ? 1 : 0;
  if (o.term) o.rew = ((f & F_RIGHT) ? 1u : 0u) == side ? r_heaven : r_hell;
  o.trunc = e1 >= (uint32_t)p.time_limit ? 1 : 0;
  if (!live) return o;  // a padding lane: its word is never stored and counts for nothing
  rsum += (double)o.rew;
  if (o.term | o.trunc) {
    if (!slippery) {
      const Philox4 z = hh_block(p, env, step, TAG);
      x2 = z.x[2];
      x3 = z.x[3];
    }
    eps += 1u;
    lens += e1;
    st = hh_reset_word(p, lds, x2, x3);
  } else {
    st = (uint32_t)cell | (side << 8) | (e1 << 16);
  }
  return o;
}

// K steps of every env. CTRL = false: the actions come from `act` [K, B], loaded one step ahead. CTRL = true
// (gp_rollout_controller): each action is drawn by the installed controller from the env's obs and node (gp_ctrl.h);
// `aout` / `nodes` receive the actions and nodes. CL: the controller table is staged in the dynamic LDS behind the
// env's tables (c.lds_off = p.tab_bytes, 16-B granules); otherwise its rows are read from global memory. A = 4, so a
// row holds exactly L = 4 M entries: whole 16-B quads, no padding. Every output pointer may be null (not stored;
// block-uniform branches): gp_rollout passes all of obs / rew / term / trunc.
template <bool CTRL, bool CL>
__global__ __launch_bounds__(TPB) void hh_rollout(HhDev p, CtrlDev c, int K, uint64_t step0,
                                                  const int32_t* __restrict__ act, int32_t* __restrict__ obs,
                                                  int32_t* __restrict__ aout, uint8_t* __restrict__ nodes,
                                                  float* __restrict__ rew, uint8_t* __restrict__ term,
                                                  uint8_t* __restrict__ trunc) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  {
    const uint4* src = (const uint4*)p.tabs;
    uint4* dst = (uint4*)lds;
    for (int i = threadIdx.x; i < p.tab_bytes / 16; i += TPB) dst[i] = src[i];
  }
  if constexpr (CL) {
    const uint4* src = (const uint4*)c.thr;
    uint4* dst = (uint4*)(lds + c.lds_off);
    for (int i = threadIdx.x; i < c.bytes / 16; i += TPB) dst[i] = src[i];
  }
  __syncthreads();
  const uint32_t* cthr = CL ? reinterpret_cast<const uint32_t*>(lds + c.lds_off) : c.thr;
  double rsum = 0.0;
  uint32_t eps = 0, lens = 0, nst = 0;
  for (int tile = blockIdx.x; tile < p.ntiles; tile += gridDim.x) {
    const int env0 = tile * EPB + threadIdx.x * EPT;
    uint32_t st[EPT];
    load4<uint32_t>(p.st, env0, p.B, st);  // (padding lanes: word 0, cell 0: in bounds of every table)
    uint8_t nd[EPT] = {0, 0, 0, 0};
    int a_nxt[EPT] = {0, 0, 0, 0};
    int32_t ob[EPT] = {0, 0, 0, 0};
    if constexpr (CTRL) {
      load4<uint8_t>(c.node, env0, p.B, nd);
#pragma unroll
      for (int i = 0; i < EPT; ++i) {
        ctrl_clamp_node(nd[i], c.M, env0 + i < p.B, p.derr);
        ob[i] = hh_obs(p, lds, st[i]);
      }
    } else {
      if (K > 0) load4<int32_t>(act, env0, p.B, a_nxt);
    }
    for (int k = 0; k < K; ++k) {
      const size_t off = (size_t)k * p.B;
      const uint64_t step = step0 + (uint64_t)k;
      int32_t a[EPT];
      uint32_t jj[EPT] = {0, 0, 0, 0};
      uint8_t n4[EPT] = {0, 0, 0, 0};
      if constexpr (CTRL) {
#pragma unroll
        for (int i = 0; i < EPT; ++i) {
          const int env = env0 + i;
          const uint32_t y = env < p.B ? hh_block(p, env, step, CTRL_TAG).x[0] >> 1 : 0u;
          jj[i] = ctrl_pick(cthr, nd[i], c.n_obs, c.L, (uint32_t)c.L, (uint32_t)ob[i], y, env < p.B, p.derr);
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
#pragma unroll
      for (int i = 0; i < EPT; ++i) {
        const bool live = env0 + i < p.B;
        const StepOut o = hh_env_step(p, lds, st[i], a[i], env0 + i, live, step, rsum, eps, lens);
        r[i] = o.rew;
        tm[i] = o.term;
        tr[i] = o.trunc;
        ob[i] = hh_obs(p, lds, st[i]);
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
    store4<uint32_t>(p.st, env0, p.B, st);
    if constexpr (CTRL) store4<uint8_t>(c.node, env0, p.B, nd);
  }
  block_metrics<WAVES>(p, rsum, eps, lens, nst);
}

__global__ __launch_bounds__(TPB) void hh_reset(HhDev p, uint64_t step, int32_t* __restrict__ obs) {
  for (int env = blockIdx.x * TPB + threadIdx.x; env < p.B; env += gridDim.x * TPB) {
    const Philox4 z = hh_block(p, env, step, TAG);
    const uint32_t st = hh_reset_word(p, p.tabs, z.x[2], z.x[3]);
    p.st[env] = st;
    obs[env] = hh_obs(p, p.tabs, st);
  }
}

__global__ void hh_get_state(HhDev p, int32_t* agent, int32_t* side, int32_t* el) {
  const int env = blockIdx.x * TPB + threadIdx.x;
  if (env >= p.B) return;
  const uint32_t st = p.st[env];
  if (agent) agent[env] = (int32_t)(st & 0xFFu);
  if (side) side[env] = (int32_t)((st >> 8) & 1u);
  if (el) el[env] = (int32_t)(st >> 16);
}
// A null pointer leaves its field alone. The agent cell is clamped to the grid and elapsed to [0, 65535]; the side
// keeps its low bit.
__global__ void hh_set_state(HhDev p, const int32_t* agent, const int32_t* side, const int32_t* el) {
  const int env = blockIdx.x * TPB + threadIdx.x;
  if (env >= p.B) return;
  uint32_t st = p.st[env] & 0xFFFF01FFu;
  if (agent) st = (st & ~0xFFu) | (uint32_t)min(max(agent[env], 0), p.ncells - 1);
  if (side) st = (st & ~0x100u) | (((uint32_t)side[env] & 1u) << 8);
  if (el) st = (st & 0xFFFFu) | ((uint32_t)min(max(el[env], 0), 65535) << 16);
  p.st[env] = st;
}

// ------------------------------------------------------------------ host backend ----
struct HeavenHellBackend : EnvBackend {
  HhDev d{};
  CtrlHost ctrl;
  int grid = 1, grid_ctrl = 1, cus = 1;
  size_t lds_ctrl = 0;  // dynamic LDS of the closed-loop launches
  uint64_t philox_step = 0;
  DevBuf b_tabs, b_st, b_slot;
  DevErr derr;

  int build(const gp_heavenhell_config* cfg);
  int seed(const RngHost& r, const uint32_t key[2]) override {
    rng = r;
    d.key0 = key[0];
    d.key1 = key[1];
    philox_step = 0;
    return derr.clear();
  }
  int check() override { return derr.check("heavenhell"); }
  int set_rng_state(const RngHost&) override {
    gp_set_error("heavenhell: no numpy stream (build-defined env; philox mode)");
    return GP_E_UNSUPPORTED;
  }
  int get_rng_state(RngHost*) override {
    gp_set_error("heavenhell: no numpy stream (build-defined env; philox mode)");
    return GP_E_UNSUPPORTED;
  }
  int query(const char* key, int64_t* v) const override {
    if (!strcmp(key, "philox_step")) *v = (int64_t)philox_step;
    else if (!strcmp(key, "controller_nodes")) *v = ctrl.dev.M;  // node count of the installed controller (0 = none)
    else if (!strcmp(key, "controller_lds")) *v = ctrl.dev.M && ctrl.dev.lds_off >= 0;  // its table is staged in LDS
    else return EnvBackend::query(key, v);
    return GP_OK;
  }
  int reset(void* obs, hipStream_t s) override {
    GP_HIP_CHECK(hipMemsetAsync(d.mslot, 0, sizeof(MetricSlot) * grid, s));
    if (int e = ctrl.reset_nodes(B, s)) return e;
    const unsigned nb = (unsigned)std::min<int64_t>((B + TPB - 1) / TPB, 65536);
    hipLaunchKernelGGL(hh_reset, dim3(nb), dim3(TPB), 0, s, d, philox_step, (int32_t*)obs);
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
    hipLaunchKernelGGL((hh_rollout<false, false>), dim3(grid), dim3(TPB), d.tab_bytes, s, d, CtrlDev{}, K,
                       philox_step, (const int32_t*)act, (int32_t*)obs, (int32_t*)nullptr, (uint8_t*)nullptr, rew,
                       term, trunc);
    timer.end(s);
    philox_step += (uint64_t)K;
    GP_HIP_CHECK(hipGetLastError());
    return GP_OK;
  }
  int step(const void* act, void* obs, float* rew, uint8_t* term, uint8_t* trunc, hipStream_t s) override {
    return rollout(1, act, obs, rew, term, trunc, s);
  }
  int get_state(void* a, void* b, void* c, void*, hipStream_t s) override {
    hipLaunchKernelGGL(hh_get_state, dim3((unsigned)((B + TPB - 1) / TPB)), dim3(TPB), 0, s, d, (int32_t*)a,
                       (int32_t*)b, (int32_t*)c);
    GP_HIP_CHECK(hipGetLastError());
    return GP_OK;
  }
  int set_state(const void* a, const void* b, const void* c, const void*, hipStream_t s) override {
    hipLaunchKernelGGL(hh_set_state, dim3((unsigned)((B + TPB - 1) / TPB)), dim3(TPB), 0, s, d, (const int32_t*)a,
                       (const int32_t*)b, (const int32_t*)c);
    GP_HIP_CHECK(hipGetLastError());
    has_reset = true;
    return GP_OK;
  }
  int controller_shape(CtrlShape* out) const override { return ctrl_shape_of(ctrl.dev.M, ctrl.dev.n_obs, NACT, 0, 0, derr.ptr(), out); }
  int set_controller(int n_nodes, int n_obs, const uint32_t* thr_host) override;
  int rollout_controller(int K, void* obs, int32_t* act, uint8_t* nodes, float* rew, uint8_t* term, uint8_t* trunc,
                         hipStream_t s) override {
    if (int e = ctrl.ready(has_reset)) return e;
    timer.begin(s);
    if (ctrl.dev.lds_off >= 0)
      hipLaunchKernelGGL((hh_rollout<true, true>), dim3(grid_ctrl), dim3(TPB), lds_ctrl, s, d, ctrl.dev, K, philox_step,
                         (const int32_t*)nullptr, (int32_t*)obs, act, nodes, rew, term, trunc);
    else
      hipLaunchKernelGGL((hh_rollout<true, false>), dim3(grid_ctrl), dim3(TPB), lds_ctrl, s, d, ctrl.dev, K, philox_step,
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

// A = 4: rows of whole 16-B quads. The closed-loop grid is sized from the kernel's occupancy at the launch's
// dynamic-LDS size (CtrlHost::stage) and never exceeds the open loop's (one set of metric slots).
int HeavenHellBackend::set_controller(int n_nodes, int n_obs, const uint32_t* thr_host) {
  if (!thr_host) return ctrl.clear();
  if (int e = ctrl.install("gp_set_controller", NACT, n_nodes, n_obs, thr_host, B)) return e;
  lds_ctrl = ctrl.stage((size_t)d.tab_bytes, true);
  int occ = 0;
  const hipError_t he =
      ctrl.dev.lds_off >= 0 ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, hh_rollout<true, true>, TPB, lds_ctrl)
                            : hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, hh_rollout<true, false>, TPB, lds_ctrl);
  if (he != hipSuccess) ctrl.dev = CtrlDev{};  // (no controller, as after a failed allocation)
  GP_HIP_CHECK(he);
  grid_ctrl = std::min(persistent_grid(d.ntiles, cus, occ), grid);
  return GP_OK;
}

int HeavenHellBackend::build(const gp_heavenhell_config* cfg) {
  const int H = cfg->height, W = cfg->width, nc = H * W;
  if (H < 1 || H > MAX_SIDE || W < 1 || W > MAX_SIDE) {
    gp_set_error("heavenhell: maze %d x %d outside [1, %d] per side", H, W, MAX_SIDE);
    return GP_E_INVALID;
  }
  if (!cfg->flags || !cfg->obs_base) {
    gp_set_error("heavenhell: flags and obs_base are required");
    return GP_E_INVALID;
  }
  if (cfg->time_limit < 1 || cfg->time_limit > 65535) {
    gp_set_error("heavenhell: time_limit %d outside [1, 65535] (elapsed is kept in 16 bits)", cfg->time_limit);
    return GP_E_INVALID;
  }
  if (cfg->keep_thr > TOP) {
    gp_set_error("heavenhell: keep_thr %u above 2^31", cfg->keep_thr);
    return GP_E_INVALID;
  }
  if (cfg->obs_base_n < 1 || cfg->obs_base_n > 256) {
    gp_set_error("heavenhell: obs_base_n %d outside [1, 256]", cfg->obs_base_n);
    return GP_E_INVALID;
  }
  std::vector<uint8_t> starts;
  for (int c = 0; c < nc; ++c) {
    const uint32_t f = cfg->flags[c];
    const int areas = ((f & F_LEFT) != 0) + ((f & F_RIGHT) != 0) + ((f & F_PRIEST) != 0);
    if ((f & ~F_ALL) || (!(f & F_FREE) && f) || areas > 1) {
      gp_set_error("heavenhell: cell %d (row %d, col %d) holds flag byte 0x%02x outside the set (a wall is 0; a free "
                   "cell is 1, plus at most one of 2 left / 4 right / 8 priest, plus 16 start)", c, c / W, c % W, f);
      return GP_E_INVALID;
    }
    if ((f & F_START) && (f & (F_LEFT | F_RIGHT))) {
      gp_set_error("heavenhell: start cell %d (row %d, col %d) lies in the %s area", c, c / W, c % W,
                   (f & F_LEFT) ? "left" : "right");
      return GP_E_INVALID;
    }
    if (f & F_START) starts.push_back((uint8_t)c);
    if (cfg->obs_base[c] < 0 || cfg->obs_base[c] >= cfg->obs_base_n) {
      gp_set_error("heavenhell: obs_base[%d] = %d outside [0, %d)", c, cfg->obs_base[c], cfg->obs_base_n);
      return GP_E_INVALID;
    }
  }
  if (starts.empty()) {
    gp_set_error("heavenhell: the maze has no start cell");
    return GP_E_INVALID;
  }
  const size_t pad_nc = ((size_t)nc + 15) & ~(size_t)15, pad_ns = (starts.size() + 15) & ~(size_t)15;
  std::vector<uint8_t> blob(2 * pad_nc + pad_ns, 0);
  for (int c = 0; c < nc; ++c) {
    blob[c] = cfg->flags[c];
    blob[pad_nc + c] = (uint8_t)cfg->obs_base[c];
  }
  memcpy(blob.data() + 2 * pad_nc, starts.data(), starts.size());
  d.off_base = (int32_t)pad_nc;
  d.off_start = (int32_t)(2 * pad_nc);
  d.tab_bytes = (int32_t)blob.size();
  int e;
  if ((e = b_tabs.upload(blob))) return e;
  d.tabs = b_tabs.as<uint8_t>();
  d.B = (int32_t)B;
  d.ntiles = (int32_t)((B + EPB - 1) / EPB);
  d.H = H;
  d.W = W;
  d.ncells = nc;
  d.n_start = (int32_t)starts.size();
  d.divm = (65536u + (uint32_t)W - 1u) / (uint32_t)W;
  d.keep_thr = cfg->keep_thr;
  d.time_limit = cfg->time_limit;
  d.r_heaven = cfg->heaven_reward;
  d.r_hell = cfg->hell_reward;
  d.r_step = cfg->step_reward;
  d.r_wall = cfg->wall_reward;
  obs_dtype = GP_DTYPE_I32;
  obs_width = 1;
  if ((e = b_st.alloc((size_t)B * 4 + 16))) return e;
  d.st = b_st.as<uint32_t>();
  hipDeviceProp_t prop;
  GP_HIP_CHECK(hipGetDeviceProperties(&prop, device));
  cus = prop.multiProcessorCount;
  int occ = 0;
  GP_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, hh_rollout<false, false>, TPB, d.tab_bytes));
  grid = persistent_grid(d.ntiles, cus, occ);
  grid_ctrl = grid;
  persist_grid = grid;
  persist_occ = occ;
  if ((e = b_slot.alloc(sizeof(MetricSlot) * grid))) return e;
  d.mslot = b_slot.as<MetricSlot>();
  if ((e = derr.alloc())) return e;
  d.derr = derr.ptr();
  return GP_OK;
}

}  // namespace

std::unique_ptr<EnvBackend> make_heavenhell_backend(const gp_heavenhell_config* cfg, int64_t B, int device,
                                                    int rng_mode, int* err) {
  if (rng_mode != GP_RNG_PHILOX) {
    gp_set_error("heavenhell: rng_mode %s does not exist for this build-defined env (no reference stream); use philox",
                 rng_mode == GP_RNG_NUMPY ? "numpy" : "replay");
    *err = GP_E_UNSUPPORTED;
    return nullptr;
  }
  if (B < 1 || B > (int64_t)1 << 30) {
    gp_set_error("heavenhell: num_envs %lld out of range", (long long)B);
    *err = GP_E_INVALID;
    return nullptr;
  }
  if (hipSetDevice(device) != hipSuccess) {
    gp_set_error("heavenhell: hipSetDevice(%d) failed", device);
    *err = GP_E_HIP;
    return nullptr;
  }
  auto be = std::make_unique<HeavenHellBackend>();
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
