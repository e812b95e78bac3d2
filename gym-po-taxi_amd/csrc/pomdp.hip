// pomdp.hip — tabular POMDP (GP_KIND_POMDP): a finite POMDP given as its T / O / R tables (Cassandra's notation), so
// that the closed-loop controller machinery runs on any finite model (Tiger, Hallway, Tag, ...) without a kernel of
// its own. There is no reference env: the device is pinned bit for bit to the numpy restatement of the rules below
// (tests/pomdp_oracle.py), and that one to a scalar statement in plain integers. Grid Heaven-Hell
// lowers to these tables exactly (gym_po_amd.envs.tabular_pomdp.heaven_hell_pomdp), which gives that kind a second,
// independent statement.
//
// Spec:
//   sizes    S states, A actions, O observations: 1 <= S <= 65,536, 1 <= A <= 64, 1 <= O <= 65,536; time_limit in
//            [1, 65,535]. Stored rows are padded to 16-B quads with 2^31: Sp = (S + 3) & ~3, Op = (O + 3) & ~3;
//            S A Sp <= 2^28 and A S Op <= 2^28.
//   config   integers decide every outcome (no float arithmetic, no libm call of the library):
//              trans_thr     uint32 [S][A][S]  row (s, a): cumulative P(s' | s, a) scaled to 2^31
//              obs_thr       uint32 [A][S][O]  row (a, s'): cumulative P(o | a, s') scaled to 2^31
//              start_thr     uint32 [S]        the start-state law
//              reset_obs_thr uint32 [S][O]     row s0: the law of the first obs given the start state
//              reward        float  [S][A][S]  indexed (s, a, s')
//              terminal      uint8  [S]
//            every threshold row nondecreasing within [0, 2^31] and ending at 2^31
//   state    one uint32 per env: s | elapsed << 16, and beside it the last observation as int32 (a draw, not a
//            function of the state: the handle keeps it, as RockSample keeps its reading)
//   actions  [-A, 0) wraps as numpy indexing does, anything else is flagged GP_DERR_ACTION and clamped
//   draws    one Philox4x32-10 block per (env, step), counter (env, step_lo, step_hi, TAG) under the handle's key;
//            with y_i = x_i >> 1:
//              s'  = #{i < S : y0 >= trans_thr[s][a][i]}
//              obs = #{i < O : y1 >= obs_thr[a][s'][i]}                      if the episode goes on
//              s0  = #{i < S : y2 >= start_thr[i]}, obs = #{i < O : y3 >= reset_obs_thr[s0][i]}   if the step ended it
//            gp_reset takes y2, y3 from the block at its own step index. Counts are clamped to S - 1 / O - 1, so a
//            padding entry is never named.
//   step     reward = reward[s][a][s'], terminated = terminal[s'], truncated = elapsed + 1 >= time_limit (gymnasium
//            TimeLimit), independent of terminated; on either the env resets in the same step from the same block, and
//            the step's obs is the reset obs
// Geometry (that of hh_rollout): a persistent grid-stride loop over 1,024-env tiles, 256 threads, 4 consecutive envs per
// thread with their state word, obs and node in registers across the K steps, actions loaded one step ahead, 16-B /
// 4-B quad accesses with an element-wise fallback. The three row searches of a step are ctrl_search (gp_ctrl.h) on the
// padded rows. TL: the model blob is copied into dynamic LDS at block start (it fits the pomdp_lds_max budget), else
// its rows are read from global memory through the caches.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "gp_ctrl.h"
#include "gp_internal.h"

namespace {

constexpr int TPB = 256;
constexpr int EPT = 4;
constexpr int EPB = TPB * EPT;
constexpr int WAVES = TPB / 64;
constexpr int MAX_STATES = 65536, MAX_ACTIONS = 64, MAX_OBS = 65536;
constexpr size_t MAX_TABLE = (size_t)1 << 28;  // entries of a padded table: 32 bits hold every index
constexpr uint32_t TAG = 0x706f6d64u;          // 'pomd'
constexpr uint32_t TOP = 1u << 31;

struct PdDev {
  int32_t B, ntiles, S, A, O, Sp, Op;
  int32_t time_limit;
  uint32_t key0, key1;
  // the model blob, 4-byte words: trans [S A][Sp] | obs [A S][Op] | start [Sp] | reset obs [S][Op] | reward [S A S] |
  // terminal bytes [S]; every section padded to 16 B
  const uint32_t* blob;
  uint32_t off_obs, off_start, off_robs, off_rew, off_term;  // in words
  int32_t blob_bytes;                                        // (only read on the TL path: at most 60 KB there)
  uint32_t* st;  // [B] s | elapsed << 16
  int32_t* ob;   // [B] the last observation
  MetricSlot* mslot;
  uint32_t* derr;  // device error word (GP_DERR_*)
};

__device__ __forceinline__ Philox4 pd_block(const PdDev& p, int env, uint64_t step, uint32_t tag) {
  return philox4x32_10((uint32_t)env, (uint32_t)step, (uint32_t)(step >> 32), tag, p.key0, p.key1);
}

// The reset: s0 by y2 from the start law, the first obs by y3 from reset_obs_thr[s0]. `m`: the blob (LDS or global).
__device__ __forceinline__ uint32_t pd_start(const PdDev& p, const uint32_t* m, uint32_t x2) {
  return min(ctrl_search(m + p.off_start, p.Sp, x2 >> 1), (uint32_t)p.S - 1u);
}

// Every index is in bounds by construction: a in [0, A) by the clamp, s < S by the state word's provenance (a clamped
// count, set_state's clamp, or word 0 of a padding lane), s' < S and obs < O by the clamp of the counts.
__device__ __forceinline__ StepOut pd_env_step(const PdDev& p, const uint32_t* m, uint32_t& st, int32_t& ob, int a,
                                               int env, bool live, uint64_t step, float& rsum, uint32_t& eps,
                                               uint32_t& lens) {
  const uint32_t S = (uint32_t)p.S, A = (uint32_t)p.A, O = (uint32_t)p.O;
  const int Sp = p.Sp, Op = p.Op;
  const uint32_t s = st & 0xFFFFu, e1 = (st >> 16) + 1u;
  // an action outside [-A, A) is flagged as numpy indexing would raise, then clamped
  if (live && action_out_of_range(a, (int)A)) flag_bad_action(p.derr);
  if (a < 0) a += (int)A;
  a = min(max(a, 0), (int)A - 1);
  const Philox4 z = pd_block(p, env, step, TAG);
  const uint32_t row = s * A + (uint32_t)a;
  const uint32_t s1 = min(ctrl_search(m + row * (uint32_t)Sp, Sp, z.x[0] >> 1), S - 1u);
  StepOut o;
  o.rew = __builtin_bit_cast(float, m[p.off_rew + row * S + s1]);
  o.term = reinterpret_cast<const uint8_t*>(m + p.off_term)[s1] ? 1 : 0;
  o.trunc = e1 >= (uint32_t)p.time_limit ? 1 : 0;
  if (!live) return o;  // a padding lane: its word is never stored and counts for nothing
  rsum += o.rew;
  // one obs search for both ends of the step: the row and the draw are chosen first
  const uint32_t* orow = m + p.off_obs + ((uint32_t)a * S + s1) * (uint32_t)Op;
  uint32_t y = z.x[1] >> 1;
  if (o.term | o.trunc) {
    eps += 1u;
    lens += e1;
    const uint32_t s0 = pd_start(p, m, z.x[2]);
    orow = m + p.off_robs + s0 * (uint32_t)Op;
    y = z.x[3] >> 1;
    st = s0;
  } else {
    st = s1 | (e1 << 16);
  }
  ob = (int32_t)min(ctrl_search(orow, Op, y), O - 1u);
  return o;
}

// K steps of every env. CTRL = false: the actions come from `act` [K, B], loaded one step ahead. CTRL = true
// (gp_rollout_controller): each action is drawn by the installed controller from the env's stored obs and node
// (gp_ctrl.h); `aout` / `nodes` receive the actions and nodes. TL: the model blob is staged in the dynamic LDS, else read
// from global memory. CL: the controller table is staged in the dynamic LDS behind the env's bytes (c.lds_off = the
// blob size, or 0 without TL); otherwise its rows are read from global memory. Rows of the controller hold c.L entries,
// A M padded to whole quads. Every output pointer may be null (not stored; block-uniform branches).
template <bool CTRL, bool TL, bool CL>
__global__ __launch_bounds__(TPB) void pd_rollout(PdDev p, CtrlDev c, int K, uint64_t step0,
                                                  const int32_t* __restrict__ act, int32_t* __restrict__ obs,
                                                  int32_t* __restrict__ aout, uint8_t* __restrict__ nodes,
                                                  float* __restrict__ rew, uint8_t* __restrict__ term,
                                                  uint8_t* __restrict__ trunc) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  if constexpr (TL) {
    const uint4* src = (const uint4*)p.blob;
    uint4* dst = (uint4*)lds;
    for (int i = threadIdx.x; i < p.blob_bytes / 16; i += TPB) dst[i] = src[i];
  }
  if constexpr (CL) {
    const uint4* src = (const uint4*)c.thr;
    uint4* dst = (uint4*)(lds + c.lds_off);
    for (int i = threadIdx.x; i < c.bytes / 16; i += TPB) dst[i] = src[i];
  }
  if constexpr (TL || CL) __syncthreads();
  const uint32_t* m = TL ? reinterpret_cast<const uint32_t*>(lds) : p.blob;
  const uint32_t* cthr = CL ? reinterpret_cast<const uint32_t*>(lds + c.lds_off) : c.thr;
  const uint32_t lreal = (uint32_t)(p.A * c.M);  // a controller row's entries before its padding
  float rsum = 0.f;
  uint32_t eps = 0, lens = 0, nst = 0;
  for (int tile = blockIdx.x; tile < p.ntiles; tile += gridDim.x) {
    const int env0 = tile * EPB + threadIdx.x * EPT;
    uint32_t st[EPT];
    int32_t ob[EPT];
    load4<uint32_t>(p.st, env0, p.B, st);  // (padding lanes: word 0, state 0, obs 0: in bounds of every table)
    load4<int32_t>(p.ob, env0, p.B, ob);
    uint8_t nd[EPT] = {0, 0, 0, 0};
    int a_nxt[EPT] = {0, 0, 0, 0};
    if constexpr (CTRL) {
      load4<uint8_t>(c.node, env0, p.B, nd);
#pragma unroll
      for (int i = 0; i < EPT; ++i) ctrl_clamp_node(nd[i], c.M, env0 + i < p.B, p.derr);
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
          const uint32_t y = env < p.B ? pd_block(p, env, step, CTRL_TAG).x[0] >> 1 : 0u;
          jj[i] = ctrl_pick<uint32_t>(cthr, nd[i], c.n_obs, c.L, lreal, (uint32_t)ob[i], y, env < p.B, p.derr);
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
        const StepOut o = pd_env_step(p, m, st[i], ob[i], a[i], env0 + i, live, step, rsum, eps, lens);
        r[i] = o.rew;
        tm[i] = o.term;
        tr[i] = o.trunc;
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
    store4<int32_t>(p.ob, env0, p.B, ob);
    if constexpr (CTRL) store4<uint8_t>(c.node, env0, p.B, nd);
  }
  block_metrics<WAVES>(p, rsum, eps, lens, nst);
}

__global__ __launch_bounds__(TPB) void pd_reset(PdDev p, uint64_t step, int32_t* __restrict__ obs) {
  for (int env = blockIdx.x * TPB + threadIdx.x; env < p.B; env += gridDim.x * TPB) {
    const Philox4 z = pd_block(p, env, step, TAG);
    const uint32_t s0 = pd_start(p, p.blob, z.x[2]);
    const int32_t o =
        (int32_t)min(ctrl_search(p.blob + p.off_robs + s0 * (uint32_t)p.Op, p.Op, z.x[3] >> 1), (uint32_t)p.O - 1u);
    p.st[env] = s0;
    p.ob[env] = o;
    obs[env] = o;
  }
}

__global__ void pd_get_state(PdDev p, int32_t* state, int32_t* el, int32_t* ob) {
  const int env = blockIdx.x * TPB + threadIdx.x;
  if (env >= p.B) return;
  const uint32_t st = p.st[env];
  if (state) state[env] = (int32_t)(st & 0xFFFFu);
  if (el) el[env] = (int32_t)(st >> 16);
  if (ob) ob[env] = p.ob[env];
}
// A null pointer leaves its field alone. The state is clamped to [0, S), elapsed to [0, 65535], the obs to [0, O).
__global__ void pd_set_state(PdDev p, const int32_t* state, const int32_t* el, const int32_t* ob) {
  const int env = blockIdx.x * TPB + threadIdx.x;
  if (env >= p.B) return;
  uint32_t st = p.st[env];
  if (state) st = (st & ~0xFFFFu) | (uint32_t)min(max(state[env], 0), p.S - 1);
  if (el) st = (st & 0xFFFFu) | ((uint32_t)min(max(el[env], 0), 65535) << 16);
  p.st[env] = st;
  if (ob) p.ob[env] = min(max(ob[env], 0), p.O - 1);
}

// ------------------------------------------------------------------ host backend ----
// ctrl_validate_rows' rule for the model's tables: every row nondecreasing within [0, 2^31] and ending at 2^31, else
// GP_E_INVALID naming the table and the row (rows are indexed (i / inner, i % inner) under the two given names; inner
// == 0: a single row). The rows are copied to `dst` [rows][Lp], each filled up to Lp entries with 2^31.
int pd_validate_rows(const char* table, const char* outer, const char* inner_name, size_t inner, const uint32_t* thr,
                     size_t rows, int L, int Lp, uint32_t* dst) {
  for (size_t r = 0; r < rows; ++r) {
    const uint32_t* t = thr + r * (size_t)L;
    char where[96];
    if (inner) snprintf(where, sizeof where, "row (%s %zu, %s %zu)", outer, r / inner, inner_name, r % inner);
    else if (rows > 1) snprintf(where, sizeof where, "row (%s %zu)", outer, r);
    else snprintf(where, sizeof where, "row");
    uint32_t prev = 0;
    for (int i = 0; i < L; ++i) {
      if (t[i] < prev || t[i] > TOP) {
        gp_set_error("pomdp: %s %s is not nondecreasing within [0, 2^31] at entry %d", table, where, i);
        return GP_E_INVALID;
      }
      prev = t[i];
    }
    if (prev != TOP) {
      gp_set_error("pomdp: %s %s ends at %u, not 2^31", table, where, prev);
      return GP_E_INVALID;
    }
    for (int i = 0; i < Lp; ++i) dst[r * (size_t)Lp + i] = i < L ? t[i] : TOP;
  }
  return GP_OK;
}

struct PomdpBackend : EnvBackend {
  PdDev d{};
  CtrlHost ctrl;
  bool model_lds = false;  // TL: the blob fits the pomdp_lds_max budget
  int grid = 1, grid_ctrl = 1, cus = 1;
  size_t lds_env = 0, lds_ctrl = 0;  // dynamic LDS of the open-loop and of the closed-loop launches
  uint64_t philox_step = 0;
  DevBuf b_blob, b_st, b_ob, b_slot;
  DevErr derr;

  int build(const gp_pomdp_config* cfg);
  int seed(const RngHost& r, const uint32_t key[2]) override {
    rng = r;
    d.key0 = key[0];
    d.key1 = key[1];
    philox_step = 0;
    return derr.clear();
  }
  int check() override { return derr.check("pomdp"); }
  int set_rng_state(const RngHost&) override {
    gp_set_error("pomdp: no numpy stream (build-defined env; philox mode)");
    return GP_E_UNSUPPORTED;
  }
  int get_rng_state(RngHost*) override {
    gp_set_error("pomdp: no numpy stream (build-defined env; philox mode)");
    return GP_E_UNSUPPORTED;
  }
  int query(const char* key, int64_t* v) const override {
    if (!strcmp(key, "philox_step")) *v = (int64_t)philox_step;
    else if (!strcmp(key, "controller_nodes")) *v = ctrl.dev.M;  // node count of the installed controller (0 = none)
    else if (!strcmp(key, "controller_lds")) *v = ctrl.dev.M && ctrl.dev.lds_off >= 0;  // its table is staged in LDS
    else if (!strcmp(key, "pomdp_lds")) *v = model_lds;             // the model blob is staged in LDS
    else if (!strcmp(key, "pomdp_model_bytes")) *v = d.blob_bytes;  // its size (compared with pomdp_lds_max)
    else return EnvBackend::query(key, v);
    return GP_OK;
  }
  int reset(void* obs, hipStream_t s) override {
    GP_HIP_CHECK(hipMemsetAsync(d.mslot, 0, sizeof(MetricSlot) * grid, s));
    if (int e = ctrl.reset_nodes(B, s)) return e;
    const unsigned nb = (unsigned)std::min<int64_t>((B + TPB - 1) / TPB, 65536);
    hipLaunchKernelGGL(pd_reset, dim3(nb), dim3(TPB), 0, s, d, philox_step, (int32_t*)obs);
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
    if (model_lds)
      hipLaunchKernelGGL((pd_rollout<false, true, false>), dim3(grid), dim3(TPB), lds_env, s, d, CtrlDev{}, K,
                         philox_step, (const int32_t*)act, (int32_t*)obs, (int32_t*)nullptr, (uint8_t*)nullptr, rew,
                         term, trunc);
    else
      hipLaunchKernelGGL((pd_rollout<false, false, false>), dim3(grid), dim3(TPB), lds_env, s, d, CtrlDev{}, K,
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
    hipLaunchKernelGGL(pd_get_state, dim3((unsigned)((B + TPB - 1) / TPB)), dim3(TPB), 0, s, d, (int32_t*)a,
                       (int32_t*)b, (int32_t*)c);
    GP_HIP_CHECK(hipGetLastError());
    return GP_OK;
  }
  int set_state(const void* a, const void* b, const void* c, const void*, hipStream_t s) override {
    hipLaunchKernelGGL(pd_set_state, dim3((unsigned)((B + TPB - 1) / TPB)), dim3(TPB), 0, s, d, (const int32_t*)a,
                       (const int32_t*)b, (const int32_t*)c);
    GP_HIP_CHECK(hipGetLastError());
    has_reset = true;
    return GP_OK;
  }
  int controller_shape(CtrlShape* out) const override {
    return ctrl_shape_of(ctrl.dev.M, ctrl.dev.n_obs, d.A, 0, 0, derr.ptr(), out);
  }
  // the closed-loop instance of the handle's two memory choices
  const void* ctrl_kernel() const {
    const bool cl = ctrl.dev.lds_off >= 0;
    if (model_lds) return cl ? (const void*)pd_rollout<true, true, true> : (const void*)pd_rollout<true, true, false>;
    return cl ? (const void*)pd_rollout<true, false, true> : (const void*)pd_rollout<true, false, false>;
  }
  int set_controller(int n_nodes, int n_obs, const uint32_t* thr_host) override;
  int rollout_controller(int K, void* obs, int32_t* act, uint8_t* nodes, float* rew, uint8_t* term, uint8_t* trunc,
                         hipStream_t s) override {
    if (int e = ctrl.ready(has_reset)) return e;
    timer.begin(s);
    const bool cl = ctrl.dev.lds_off >= 0;
#define PD_LAUNCH_CTRL(TL_, CL_)                                                                                   \
  hipLaunchKernelGGL((pd_rollout<true, TL_, CL_>), dim3(grid_ctrl), dim3(TPB), lds_ctrl, s, d, ctrl.dev, K,        \
                     philox_step, (const int32_t*)nullptr, (int32_t*)obs, act, nodes, rew, term, trunc)
    if (model_lds && cl) PD_LAUNCH_CTRL(true, true);
    else if (model_lds) PD_LAUNCH_CTRL(true, false);
    else if (cl) PD_LAUNCH_CTRL(false, true);
    else PD_LAUNCH_CTRL(false, false);
#undef PD_LAUNCH_CTRL
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

// Rows hold L = A M entries, padded to 16-B quads by CtrlHost::install where L is no multiple of 4. The table is staged
// behind the env's LDS bytes (the blob, or nothing on the global path). The closed-loop grid is sized from the kernel's
// occupancy at the launch's dynamic-LDS size and never exceeds the open loop's (one set of metric slots).
int PomdpBackend::set_controller(int n_nodes, int n_obs, const uint32_t* thr_host) {
  if (!thr_host) return ctrl.clear();
  if (int e = ctrl.install("gp_set_controller", d.A, n_nodes, n_obs, thr_host, B)) return e;
  lds_ctrl = ctrl.stage(lds_env, true);
  int occ = 0;
  const hipError_t he = hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, ctrl_kernel(), TPB, lds_ctrl);
  if (he != hipSuccess) ctrl.dev = CtrlDev{};  // (no controller, as after a failed allocation)
  GP_HIP_CHECK(he);
  grid_ctrl = std::min(persistent_grid(d.ntiles, cus, occ), grid);
  return GP_OK;
}

int PomdpBackend::build(const gp_pomdp_config* cfg) {
  const int S = cfg->n_states, A = cfg->n_actions, O = cfg->n_obs;
  if (S < 1 || S > MAX_STATES || A < 1 || A > MAX_ACTIONS || O < 1 || O > MAX_OBS) {
    gp_set_error("pomdp: sizes (S %d, A %d, O %d) outside [1, %d] x [1, %d] x [1, %d]", S, A, O, MAX_STATES,
                 MAX_ACTIONS, MAX_OBS);
    return GP_E_INVALID;
  }
  if (cfg->time_limit < 1 || cfg->time_limit > 65535) {
    gp_set_error("pomdp: time_limit %d outside [1, 65535] (elapsed is kept in 16 bits)", cfg->time_limit);
    return GP_E_INVALID;
  }
  if (!cfg->trans_thr || !cfg->obs_thr || !cfg->start_thr || !cfg->reset_obs_thr || !cfg->reward || !cfg->terminal) {
    gp_set_error("pomdp: trans_thr, obs_thr, start_thr, reset_obs_thr, reward and terminal are required");
    return GP_E_INVALID;
  }
  const size_t Sp = ((size_t)S + 3) & ~(size_t)3, Op = ((size_t)O + 3) & ~(size_t)3;
  const size_t n_trans = (size_t)S * A * Sp, n_obs = (size_t)A * S * Op;
  if (n_trans > MAX_TABLE || n_obs > MAX_TABLE) {
    gp_set_error("pomdp: padded tables of %zu (trans_thr) and %zu (obs_thr) entries are too large (max 2^28 each)",
                 n_trans, n_obs);
    return GP_E_INVALID;
  }
  const size_t n_robs = (size_t)S * Op, n_rew = ((size_t)S * A * S + 3) & ~(size_t)3;
  const size_t n_term = (((size_t)S + 15) & ~(size_t)15) / 4;
  const size_t off_obs = n_trans, off_start = off_obs + n_obs, off_robs = off_start + Sp, off_rew = off_robs + n_robs,
               off_term = off_rew + n_rew, n_words = off_term + n_term;  // < 2^30 + 2^17: 32 bits hold every offset
  std::vector<uint32_t> blob(n_words, 0);
  int e;
  if ((e = pd_validate_rows("trans_thr", "s", "a", (size_t)A, cfg->trans_thr, (size_t)S * A, S, (int)Sp, blob.data())) ||
      (e = pd_validate_rows("obs_thr", "a", "s'", (size_t)S, cfg->obs_thr, (size_t)A * S, O, (int)Op,
                            blob.data() + off_obs)) ||
      (e = pd_validate_rows("start_thr", "", "", 0, cfg->start_thr, 1, S, (int)Sp, blob.data() + off_start)) ||
      (e = pd_validate_rows("reset_obs_thr", "s", "", 0, cfg->reset_obs_thr, (size_t)S, O, (int)Op,
                            blob.data() + off_robs)))
    return e;
  memcpy(blob.data() + off_rew, cfg->reward, (size_t)S * A * S * sizeof(float));
  uint8_t* tb = reinterpret_cast<uint8_t*>(blob.data() + off_term);
  for (int s = 0; s < S; ++s) tb[s] = cfg->terminal[s] ? 1 : 0;
  if ((e = b_blob.upload(blob))) return e;
  d.blob = b_blob.as<uint32_t>();
  d.off_obs = (uint32_t)off_obs;
  d.off_start = (uint32_t)off_start;
  d.off_robs = (uint32_t)off_robs;
  d.off_rew = (uint32_t)off_rew;
  d.off_term = (uint32_t)off_term;
  d.blob_bytes = (int32_t)std::min(n_words * 4, (size_t)INT32_MAX);
  d.B = (int32_t)B;
  d.ntiles = (int32_t)((B + EPB - 1) / EPB);
  d.S = S;
  d.A = A;
  d.O = O;
  d.Sp = (int32_t)Sp;
  d.Op = (int32_t)Op;
  d.time_limit = cfg->time_limit;
  obs_dtype = GP_DTYPE_I32;
  obs_width = 1;
  // the blob goes into LDS when it fits the budget (knob pomdp_lds_max, at most 60 KB: with block_metrics' static LDS a
  // launch stays below 64 KB)
  const int knob = gp_debug_knobs().pomdp_lds_max;
  const size_t budget = knob >= 0 ? std::min((size_t)knob, (size_t)60 * 1024) : (size_t)CTRL_LDS_BUDGET;
  model_lds = n_words * 4 <= budget;
  lds_env = model_lds ? n_words * 4 : 0;
  lds_ctrl = lds_env;
  if ((e = b_st.alloc((size_t)B * 4 + 16)) || (e = b_ob.alloc((size_t)B * 4 + 16))) return e;
  d.st = b_st.as<uint32_t>();
  d.ob = b_ob.as<int32_t>();
  hipDeviceProp_t prop;
  GP_HIP_CHECK(hipGetDeviceProperties(&prop, device));
  cus = prop.multiProcessorCount;
  int occ = 0;
  if (model_lds) GP_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, pd_rollout<false, true, false>, TPB, lds_env));
  else GP_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, pd_rollout<false, false, false>, TPB, lds_env));
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

std::unique_ptr<EnvBackend> make_pomdp_backend(const gp_pomdp_config* cfg, int64_t B, int device, int rng_mode,
                                               int* err) {
  if (rng_mode != GP_RNG_PHILOX) {
    gp_set_error("pomdp: rng_mode %s does not exist for this build-defined env (no reference stream); use philox",
                 rng_mode == GP_RNG_NUMPY ? "numpy" : "replay");
    *err = GP_E_UNSUPPORTED;
    return nullptr;
  }
  if (B < 1 || B > (int64_t)1 << 30) {
    gp_set_error("pomdp: num_envs %lld out of range", (long long)B);
    *err = GP_E_INVALID;
    return nullptr;
  }
  if (hipSetDevice(device) != hipSuccess) {
    gp_set_error("pomdp: hipSetDevice(%d) failed", device);
    *err = GP_E_HIP;
    return nullptr;
  }
  auto be = std::make_unique<PomdpBackend>();
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
