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
#include "pomdp_backup.h"
#include "pomdp_expand.h"

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
                                               int env, bool live, uint64_t step, double& rsum, uint32_t& eps,
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
  rsum += (double)o.rew;
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
  double rsum = 0.0;
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

// ------------------------------------------------------------------ belief filter ----
// The exact Bayes filter of the model, one belief b[S] per env, and a piecewise-linear (alpha-vector) policy over it
// (pinned bit for bit to tests/belief_oracle.py).
//
// Float laws. The laws the filter multiplies are the handle's integer thresholds as float32: for a threshold row thr,
//   p[i] = (float)(uint32)(thr[i] - thr[i-1]) * 2^-31, thr[-1] = 0
// (one round-to-nearest conversion, then an exact scale): Tf[s][a][s'] from trans_thr, Zf[a][s'][o] from obs_thr,
// Rf[s][o] from reset_obs_thr, and the default prior from start_thr. Zf and Rf are formed on the spot from the two
// neighbouring thresholds of the blob; Tf is kept as compressed columns (per (a, s') the nonzero (s, Tf) pairs, s
// ascending), built by the host at gp_belief_enable.
//
// Arithmetic. float32, every product and every sum rounded on its own (no FMA: contraction is off from here to the
// end of the file), denormals kept, sums sequential in ascending index from +0, division correctly rounded.
//
// Filter step. Belief b, action a (wrapped / clamped as pd_env_step does), the stored obs o after the step,
// ended = term | trunc.
//   not ended: acc(s') = sum_s fl(b[s] Tf[s][a][s']);  u(s') = terminal[s'] ? +0 : fl(Zf[a][s'][o] acc(s'))  (a step
//              that did not end tells the agent that s' is not terminal)
//   ended:     u(s) = fl(prior[s] Rf[s][o])  (the stored obs is the reset obs)
//   both:      n = sum_s u(s);  b'(s) = fl(u(s) / n);  if !(n > 0) or n is not finite: b' = prior and GP_DERR_BELIEF
// gp_reset and gp_belief_enable set b by the ended rule from each env's stored obs.
// Zero skipping: all operands are >= 0 and the accumulators start at +0, so leaving out the entries with Tf == 0 and
// the whole columns with Zf == 0 or a terminal s' gives the bits of the dense loop (for finite beliefs).
//
// Policy. N vectors alpha[N][S] with an action each: v_j = sum_s fl(b[s] alpha[j][s]), j* the first j that attains the
// maximum (replaced only on a strict >), action = vec_action[j*], chosen from the belief before the step. No draw is
// spent: the env's Philox blocks are those of gp_rollout.
//
// Placement. Beliefs live in two global planes [S][B] (double buffer; which one is current is host state). On chip: a
// block's 1,024 envs keep both buffers in LDS for the K steps of a launch, laid out [s][i][thread] (i = the thread's
// env 0..3) so that the 64 lanes of a wave read 64 consecutive words; loaded once and stored once per tile. Global:
// the planes themselves, rows of B floats, any S up to the limit. Both run pd_filter_step, so their bits are equal.
#pragma clang fp contract(off)

constexpr int MAX_BELIEF_STATES = 4096, MAX_VECTORS = 4096;
constexpr size_t MAX_ALPHA = (size_t)1 << 22;

struct BfDev {
  float* bel[2];           // [S][B] each
  const float* prior;      // [S]
  const uint32_t* colptr;  // [A S + 1] column (a, s') of Tf: entries colptr[a S + s'] .. colptr[a S + s' + 1]
  const uint2* ent;        // (s, bits of Tf[s][a][s']), s ascending within a column
  const float* alpha;      // [N][S]
  const int32_t* vact;     // [N] in [0, A)
  int32_t N;
};

// A belief of one env in LDS ([s][i][thread]: stride EPB words) or in a global plane ([S][B]: stride B).
struct BelLds {
  float* p;
  __device__ __forceinline__ float get(int s) const { return p[s * EPB]; }
  __device__ __forceinline__ void set(int s, float v) const { p[s * EPB] = v; }
};
struct BelGlb {
  float* p;
  size_t B;
  __device__ __forceinline__ float get(int s) const { return p[(size_t)s * B]; }
  __device__ __forceinline__ void set(int s, float v) const { p[(size_t)s * B] = v; }
};

// p[i] of a padded threshold row (i below the row's real length: in bounds by the caller's clamp)
__device__ __forceinline__ float pd_law(const uint32_t* row, uint32_t i) {
  const uint32_t d = row[i] - (i ? row[i - 1] : 0u);
  return (float)d * 0x1p-31f;
}

// One filter step of one env: cur -> nxt. a in [0, A) and o in [0, O) by the callers' clamps; every s read from `ent`
// is below S by the host's construction.
template <class BR>
__device__ __forceinline__ void pd_filter_step(const PdDev& p, const BfDev& f, const uint32_t* m, const BR cur,
                                               const BR nxt, uint32_t a, uint32_t o, bool ended) {
  const uint32_t S = (uint32_t)p.S, Op = (uint32_t)p.Op;
  float n = 0.f;
  if (ended) {
    for (uint32_t s = 0; s < S; ++s) {
      const float u = f.prior[s] * pd_law(m + p.off_robs + s * Op, o);
      nxt.set((int)s, u);
      n = n + u;
    }
  } else {
    const uint8_t* tb = reinterpret_cast<const uint8_t*>(m + p.off_term);
    const uint32_t* cp = f.colptr + a * S;
    for (uint32_t s1 = 0; s1 < S; ++s1) {
      float u = 0.f;
      const uint32_t* zrow = m + p.off_obs + (a * S + s1) * Op;
      const uint32_t zd = zrow[o] - (o ? zrow[o - 1] : 0u);
      if (!tb[s1] && zd) {
        float acc = 0.f;
        for (uint32_t e = cp[s1], e1 = cp[s1 + 1]; e < e1; ++e) {
          const uint2 q = f.ent[e];
          acc = acc + cur.get((int)q.x) * __builtin_bit_cast(float, q.y);
        }
        u = ((float)zd * 0x1p-31f) * acc;
      }
      nxt.set((int)s1, u);
      n = n + u;
    }
  }
  if (n > 0.f && n <= 3.402823466e38f) {
    for (uint32_t s = 0; s < S; ++s) nxt.set((int)s, nxt.get((int)s) / n);
  } else {
    for (uint32_t s = 0; s < S; ++s) nxt.set((int)s, f.prior[s]);
    atomicOr(p.derr, GP_DERR_BELIEF);
  }
}

// The policy's choice on one belief: the first maximiser and its value.
template <class BR>
__device__ __forceinline__ void pd_belief_pick(const PdDev& p, const BfDev& f, const BR cur, int32_t& jbest,
                                               float& vbest) {
  const int S = p.S;
  jbest = 0;
  vbest = 0.f;
  // four vectors per pass over the belief (each v_j still its own ascending sum): a quarter of the belief reads
  for (int j0 = 0; j0 < f.N; j0 += 4) {
    const int nj = min(4, f.N - j0);
    const float* al = f.alpha + (size_t)j0 * S;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < S; ++s) {
      const float b = cur.get(s);
      if (b != 0.f) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (i < nj) v[i] = v[i] + b * al[(size_t)i * S + s];
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (i < nj && (j0 + i == 0 || v[i] > vbest)) {
        vbest = v[i];
        jbest = j0 + i;
      }
  }
}

// A tile's beliefs between the current plane and LDS buffer `buf` (on chip only).
__device__ __forceinline__ void pd_belief_load(const float* plane, float* buf, int S, int env0, int B) {
  for (int s = 0; s < S; ++s) {
    float v[EPT];
    load4<float>(plane + (size_t)s * B, env0, B, v);
#pragma unroll
    for (int i = 0; i < EPT; ++i) buf[s * EPB + i * TPB + threadIdx.x] = v[i];
  }
}
__device__ __forceinline__ void pd_belief_store(float* plane, const float* buf, int S, int env0, int B) {
  for (int s = 0; s < S; ++s) {
    float v[EPT];
#pragma unroll
    for (int i = 0; i < EPT; ++i) v[i] = buf[s * EPB + i * TPB + threadIdx.x];
    store4<float>(plane + (size_t)s * B, env0, B, v);
  }
}

// gp_belief_filter: the stored beliefs advanced over K stored steps of planes [K, B]. OC: the tile's beliefs stay in
// LDS (2 S EPB floats of dynamic LDS). cur0: the current plane. Actions are wrapped and clamped as pd_env_step does
// (GP_DERR_ACTION), obs values clamped to [0, O) (GP_DERR_CTRL). The model's rows are read from global memory.
template <bool OC>
__global__ __launch_bounds__(TPB) void pd_belief_filter(PdDev p, BfDev f, int K, int cur0,
                                                        const int32_t* __restrict__ act,
                                                        const int32_t* __restrict__ obs,
                                                        const uint8_t* __restrict__ term,
                                                        const uint8_t* __restrict__ trunc) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  float* lb = reinterpret_cast<float*>(lds);
  const uint32_t* m = p.blob;
  const size_t half = (size_t)p.S * EPB;
  for (int tile = blockIdx.x; tile < p.ntiles; tile += gridDim.x) {
    const int env0 = tile * EPB + threadIdx.x * EPT;
    if constexpr (OC) pd_belief_load(f.bel[cur0], lb + (size_t)cur0 * half, p.S, env0, p.B);
    for (int k = 0; k < K; ++k) {
      const size_t off = (size_t)k * p.B;
      const int cur = (cur0 + k) & 1;
      int32_t a[EPT], o[EPT];
      uint8_t tm[EPT], tr[EPT];
      load4<int32_t>(act + off, env0, p.B, a);
      load4<int32_t>(obs + off, env0, p.B, o);
      load4<uint8_t>(term + off, env0, p.B, tm);
      load4<uint8_t>(trunc + off, env0, p.B, tr);
#pragma unroll
      for (int i = 0; i < EPT; ++i) {
        if (env0 + i >= p.B) continue;
        int ai = a[i], oi = o[i];
        if (action_out_of_range(ai, p.A)) flag_bad_action(p.derr);
        if (ai < 0) ai += p.A;
        ai = min(max(ai, 0), p.A - 1);
        if ((uint32_t)oi >= (uint32_t)p.O) atomicOr(p.derr, GP_DERR_CTRL);
        oi = min(max(oi, 0), p.O - 1);
        const bool ended = (tm[i] | tr[i]) != 0;
        if constexpr (OC) {
          const int slot = i * TPB + threadIdx.x;
          pd_filter_step(p, f, m, BelLds{lb + (size_t)cur * half + slot}, BelLds{lb + (size_t)(cur ^ 1) * half + slot},
                         (uint32_t)ai, (uint32_t)oi, ended);
        } else {
          pd_filter_step(p, f, m, BelGlb{f.bel[cur] + env0 + i, (size_t)p.B},
                         BelGlb{f.bel[cur ^ 1] + env0 + i, (size_t)p.B}, (uint32_t)ai, (uint32_t)oi, ended);
        }
      }
    }
    if constexpr (OC) {
      const int last = (cur0 + K) & 1;
      pd_belief_store(f.bel[last], lb + (size_t)last * half, p.S, env0, p.B);
    }
  }
}

// gp_rollout_belief: K closed-loop steps of every env in one launch: the policy's choice on the belief, pd_env_step,
// pd_filter_step. TL: the model blob is staged in dynamic LDS (as in pd_rollout); OC: the tile's beliefs stay in LDS
// behind it (at byte bel_off). `vec` / `value` receive j* and v_j*. Every output pointer may be null.
template <bool TL, bool OC>
__global__ __launch_bounds__(TPB) void pd_rollout_belief(PdDev p, BfDev f, int K, uint64_t step0, int cur0,
                                                         uint32_t bel_off, int32_t* __restrict__ obs,
                                                         int32_t* __restrict__ aout, int32_t* __restrict__ vec,
                                                         float* __restrict__ value, float* __restrict__ rew,
                                                         uint8_t* __restrict__ term, uint8_t* __restrict__ trunc) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  if constexpr (TL) {
    const uint4* src = (const uint4*)p.blob;
    uint4* dst = (uint4*)lds;
    for (int i = threadIdx.x; i < p.blob_bytes / 16; i += TPB) dst[i] = src[i];
    __syncthreads();
  }
  const uint32_t* m = TL ? reinterpret_cast<const uint32_t*>(lds) : p.blob;
  float* lb = reinterpret_cast<float*>(lds + bel_off);
  const size_t half = (size_t)p.S * EPB;
  double rsum = 0.0;
  uint32_t eps = 0, lens = 0, nst = 0;
  for (int tile = blockIdx.x; tile < p.ntiles; tile += gridDim.x) {
    const int env0 = tile * EPB + threadIdx.x * EPT;
    uint32_t st[EPT];
    int32_t ob[EPT];
    load4<uint32_t>(p.st, env0, p.B, st);
    load4<int32_t>(p.ob, env0, p.B, ob);
    if constexpr (OC) pd_belief_load(f.bel[cur0], lb + (size_t)cur0 * half, p.S, env0, p.B);
    for (int k = 0; k < K; ++k) {
      const size_t off = (size_t)k * p.B;
      const uint64_t step = step0 + (uint64_t)k;
      const int cur = (cur0 + k) & 1;
      int32_t a[EPT], jj[EPT];
      float vv[EPT], r[EPT];
      uint8_t tm[EPT], tr[EPT];
#pragma unroll
      for (int i = 0; i < EPT; ++i) {
        const bool live = env0 + i < p.B;
        a[i] = 0;
        jj[i] = 0;
        vv[i] = 0.f;
        if (live) {
          if constexpr (OC) pd_belief_pick(p, f, BelLds{lb + (size_t)cur * half + i * TPB + threadIdx.x}, jj[i], vv[i]);
          else pd_belief_pick(p, f, BelGlb{f.bel[cur] + env0 + i, (size_t)p.B}, jj[i], vv[i]);
          a[i] = f.vact[jj[i]];
        }
        const StepOut o = pd_env_step(p, m, st[i], ob[i], a[i], env0 + i, live, step, rsum, eps, lens);
        r[i] = o.rew;
        tm[i] = o.term;
        tr[i] = o.trunc;
        nst += live ? 1u : 0u;
        if (live) {
          const bool ended = (o.term | o.trunc) != 0;
          const uint32_t ai = (uint32_t)min(max(a[i], 0), p.A - 1);  // (vec_action is validated: a no-op)
          if constexpr (OC) {
            const int slot = i * TPB + threadIdx.x;
            pd_filter_step(p, f, m, BelLds{lb + (size_t)cur * half + slot},
                           BelLds{lb + (size_t)(cur ^ 1) * half + slot}, ai, (uint32_t)ob[i], ended);
          } else {
            pd_filter_step(p, f, m, BelGlb{f.bel[cur] + env0 + i, (size_t)p.B},
                           BelGlb{f.bel[cur ^ 1] + env0 + i, (size_t)p.B}, ai, (uint32_t)ob[i], ended);
          }
        }
      }
      if (aout) store4<int32_t>(aout + off, env0, p.B, a);
      if (vec) store4<int32_t>(vec + off, env0, p.B, jj);
      if (value) store4<float>(value + off, env0, p.B, vv);
      if (rew) store4<float>(rew + off, env0, p.B, r);
      if (term) store4<uint8_t>(term + off, env0, p.B, tm);
      if (trunc) store4<uint8_t>(trunc + off, env0, p.B, tr);
      if (obs) store4<int32_t>(obs + off, env0, p.B, ob);
    }
    store4<uint32_t>(p.st, env0, p.B, st);
    store4<int32_t>(p.ob, env0, p.B, ob);
    if constexpr (OC) {
      const int last = (cur0 + K) & 1;
      pd_belief_store(f.bel[last], lb + (size_t)last * half, p.S, env0, p.B);
    }
  }
  block_metrics<WAVES>(p, rsum, eps, lens, nst);
}

// gp_reset / gp_belief_enable: every belief by the ended rule from the env's stored obs, into plane `cur`.
__global__ __launch_bounds__(TPB) void pd_belief_reset(PdDev p, BfDev f, int cur) {
  for (int env = blockIdx.x * TPB + threadIdx.x; env < p.B; env += gridDim.x * TPB) {
    const BelGlb b{f.bel[cur] + env, (size_t)p.B};
    pd_filter_step(p, f, p.blob, b, b, 0u, (uint32_t)min(max(p.ob[env], 0), p.O - 1), true);
  }
}

// gp_belief_get / gp_belief_set: plane [S][B] <-> the caller's [B][S], values as they are.
template <bool GET>
__global__ __launch_bounds__(TPB) void pd_belief_copy(float* plane, float* user, int S, int B) {
  const size_t n = (size_t)S * (size_t)B;
  for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (size_t)gridDim.x * TPB) {
    const size_t s = i / (size_t)B, env = i % (size_t)B;
    if constexpr (GET) user[env * S + s] = plane[i];
    else plane[i] = user[env * S + s];
  }
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
  // the belief filter (gp_belief_enable) and its policy (gp_set_belief_policy)
  BfDev bf{};
  bool belief_on = false, belief_oc = false;  // enabled; the beliefs of a launch stay in LDS
  int bel_cur = 0;                            // which of the two planes holds the beliefs
  int grid_bel = 1, grid_filt = 1;
  DevBuf b_bel[2], b_prior, b_cp, b_ent, b_alpha, b_vact;
  PbHost pb;  // the point-based backup's tables, vectors and scratch (gp_belief_backup; pomdp_backup.hip)
  PxHost px;  // the expansion's scratch beside it (gp_belief_expand; pomdp_expand.hip)

  int build(const gp_pomdp_config* cfg);
  int belief_enable(const float* prior) override;
  int belief_disable() override {
    belief_on = belief_oc = false;
    pb.release();
    px.release();
    for (DevBuf* b : {&b_bel[0], &b_bel[1], &b_prior, &b_cp, &b_ent}) (void)b->alloc(0);
    bf.bel[0] = bf.bel[1] = nullptr;
    bf.prior = nullptr;
    bf.colptr = nullptr;
    bf.ent = nullptr;
    return GP_OK;
  }
  int belief_ready(const char* what) const {
    if (!belief_on) {
      gp_set_error("%s without a belief filter (gp_belief_enable)", what);
      return GP_E_STATE;
    }
    return GP_OK;
  }
  size_t belief_lds() const { return belief_oc ? (size_t)2 * d.S * EPB * sizeof(float) : 0; }
  int belief_reset(hipStream_t s) {
    const unsigned nb = (unsigned)std::min<int64_t>((B + TPB - 1) / TPB, 65536);
    hipLaunchKernelGGL(pd_belief_reset, dim3(nb), dim3(TPB), 0, s, d, bf, bel_cur);
    GP_HIP_CHECK(hipGetLastError());
    return GP_OK;
  }
  int belief_get(float* out, hipStream_t s) override {
    if (int e = belief_ready("gp_belief_get")) return e;
    const unsigned nb = (unsigned)std::min<size_t>(((size_t)B * d.S + TPB - 1) / TPB, 65536);
    hipLaunchKernelGGL(pd_belief_copy<true>, dim3(nb), dim3(TPB), 0, s, bf.bel[bel_cur], out, d.S, d.B);
    GP_HIP_CHECK(hipGetLastError());
    return GP_OK;
  }
  int belief_set(const float* in, hipStream_t s) override {
    if (int e = belief_ready("gp_belief_set")) return e;
    const unsigned nb = (unsigned)std::min<size_t>(((size_t)B * d.S + TPB - 1) / TPB, 65536);
    hipLaunchKernelGGL(pd_belief_copy<false>, dim3(nb), dim3(TPB), 0, s, bf.bel[bel_cur], const_cast<float*>(in), d.S,
                       d.B);
    GP_HIP_CHECK(hipGetLastError());
    return GP_OK;
  }
  int belief_filter(int K, const int32_t* act, const int32_t* obs, const uint8_t* term, const uint8_t* trunc,
                    hipStream_t s) override {
    if (int e = belief_ready("gp_belief_filter")) return e;
    if (K == 0) return GP_OK;
    timer.begin(s);  // (gp_set_profiling times this launch as it times the rollouts)
    if (belief_oc)
      hipLaunchKernelGGL(pd_belief_filter<true>, dim3(grid_filt), dim3(TPB), belief_lds(), s, d, bf, K, bel_cur, act,
                         obs, term, trunc);
    else
      hipLaunchKernelGGL(pd_belief_filter<false>, dim3(grid_filt), dim3(TPB), 0, s, d, bf, K, bel_cur, act, obs, term,
                         trunc);
    timer.end(s);
    bel_cur = (bel_cur + K) & 1;
    GP_HIP_CHECK(hipGetLastError());
    return GP_OK;
  }
  int set_belief_policy(int n_vec, const float* alpha, const int32_t* vec_action) override;
  // gp_belief_backup: reads the model and the filter's float laws, writes only its outputs
  PbModel backup_model() const {
    PbModel m;
    m.S = d.S, m.A = d.A, m.O = d.O, m.Sp = d.Sp, m.Op = d.Op;
    m.blob = d.blob;
    m.off_obs = d.off_obs, m.off_rew = d.off_rew, m.off_term = d.off_term;
    m.colptr = bf.colptr;
    m.ent = bf.ent;
    return m;
  }
  int belief_backup(int P, const float* points, int N, const float* alpha, float gamma, float* alpha_out,
                    int32_t* act_out, float* value_out, hipStream_t s) override {
    if (int e = belief_ready("gp_belief_backup")) return e;
    return pb.backup(backup_model(), P, points, N, alpha, gamma, alpha_out, act_out, value_out, s);
  }
  // gp_belief_expand: as the backup, reads the model and writes only its outputs
  int belief_expand(int P, const float* points, int Q, const float* ref, float* succ_out, float* dist_out,
                    int32_t* act_out, int32_t* obs_out, float* mass_out, hipStream_t s) override {
    if (int e = belief_ready("gp_belief_expand")) return e;
    return px.expand(pb, backup_model(), P, points, Q, ref, succ_out, dist_out, act_out, obs_out, mass_out, s);
  }
  int rollout_belief(int K, void* obs, int32_t* act, int32_t* vec, float* value, float* rew, uint8_t* term,
                     uint8_t* trunc, hipStream_t s) override {
    if (!has_reset) {
      gp_set_error("gp_rollout_belief before reset()");
      return GP_E_STATE;
    }
    if (int e = belief_ready("gp_rollout_belief")) return e;
    if (!bf.N) {
      gp_set_error("gp_rollout_belief without a policy (gp_set_belief_policy)");
      return GP_E_STATE;
    }
    if (K == 0) return GP_OK;
    timer.begin(s);
    const size_t lds_bytes = lds_env + belief_lds();
#define PD_LAUNCH_BEL(TL_, OC_)                                                                                     \
  hipLaunchKernelGGL((pd_rollout_belief<TL_, OC_>), dim3(grid_bel), dim3(TPB), lds_bytes, s, d, bf, K, philox_step, \
                     bel_cur, (uint32_t)lds_env, (int32_t*)obs, act, vec, value, rew, term, trunc)
    if (model_lds && belief_oc) PD_LAUNCH_BEL(true, true);
    else if (model_lds) PD_LAUNCH_BEL(true, false);
    else if (belief_oc) PD_LAUNCH_BEL(false, true);
    else PD_LAUNCH_BEL(false, false);
#undef PD_LAUNCH_BEL
    timer.end(s);
    philox_step += (uint64_t)K;
    bel_cur = (bel_cur + K) & 1;
    GP_HIP_CHECK(hipGetLastError());
    return GP_OK;
  }
  // the launch grids of the two belief kernels at the handle's placements (never above the open loop's: one set of
  // metric slots)
  int belief_grids() {
    int occ = 0;
    const void* k = model_lds ? (belief_oc ? (const void*)pd_rollout_belief<true, true> : (const void*)pd_rollout_belief<true, false>)
                              : (belief_oc ? (const void*)pd_rollout_belief<false, true> : (const void*)pd_rollout_belief<false, false>);
    GP_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, k, TPB, lds_env + belief_lds()));
    grid_bel = std::min(persistent_grid(d.ntiles, cus, occ), grid);
    k = belief_oc ? (const void*)pd_belief_filter<true> : (const void*)pd_belief_filter<false>;
    GP_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, k, TPB, belief_lds()));
    grid_filt = persistent_grid(d.ntiles, cus, occ);
    return GP_OK;
  }
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
    else if (!strcmp(key, "belief")) *v = belief_on;                // the belief filter is enabled
    else if (!strcmp(key, "belief_onchip")) *v = belief_oc;         // its beliefs stay in LDS across a launch
    else if (!strcmp(key, "belief_onchip_bytes")) *v = (int64_t)2 * d.S * EPB * 4;  // (compared with belief_onchip_max)
    else if (!strcmp(key, "belief_vectors")) *v = bf.N;             // vectors of the installed policy (0 = none)
    else if (!strcmp(key, "backup_scratch_bytes")) *v = (int64_t)pb.scratch_bytes();  // gp_belief_backup's scratch
    else if (!strcmp(key, "backup_tables")) *v = pb.built;          // its compressed tables are built
    else if (!strcmp(key, "expand_scratch_bytes")) *v = (int64_t)(pb.b_acc.n + px.own_bytes());  // gp_belief_expand's (acc is the backup's)
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
    if (belief_on) return belief_reset(s);
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

// The float laws the filter needs beyond the blob: the prior (given, used as it is; else the start law) and Tf as
// compressed columns, from the thresholds the handle was built with (read back from the device: the host keeps no
// copy). Everything is built and uploaded into buffers of its own first: a failure installs nothing.
int PomdpBackend::belief_enable(const float* prior) {
  const int S = d.S, A = d.A, Sp = d.Sp;
  if (S > MAX_BELIEF_STATES) {
    gp_set_error("gp_belief_enable: %d states, the belief filter takes at most %d", S, MAX_BELIEF_STATES);
    return GP_E_INVALID;
  }
  GP_HIP_CHECK(hipDeviceSynchronize());
  std::vector<uint32_t> thr((size_t)S * A * Sp + Sp);
  GP_HIP_CHECK(hipMemcpy(thr.data(), d.blob, (size_t)S * A * Sp * 4, hipMemcpyDeviceToHost));
  GP_HIP_CHECK(hipMemcpy(thr.data() + (size_t)S * A * Sp, d.blob + d.off_start, (size_t)Sp * 4, hipMemcpyDeviceToHost));
  auto law = [](const uint32_t* row, int i) { return (float)(uint32_t)(row[i] - (i ? row[i - 1] : 0u)) * 0x1p-31f; };
  std::vector<float> pr(S);
  for (int s = 0; s < S; ++s) pr[s] = prior ? prior[s] : law(thr.data() + (size_t)S * A * Sp, s);
  std::vector<uint32_t> cp((size_t)A * S + 1, 0);
  for (int s = 0; s < S; ++s)
    for (int a = 0; a < A; ++a) {
      const uint32_t* row = thr.data() + ((size_t)s * A + a) * Sp;
      for (int s1 = 0; s1 < S; ++s1)
        if (row[s1] != (s1 ? row[s1 - 1] : 0u)) ++cp[(size_t)a * S + s1 + 1];
    }
  for (size_t c = 0; c < (size_t)A * S; ++c) cp[c + 1] += cp[c];
  std::vector<uint2> ent(cp.back());
  std::vector<uint32_t> fill(cp.begin(), cp.end() - 1);
  for (int s = 0; s < S; ++s)  // s ascending within every column
    for (int a = 0; a < A; ++a) {
      const uint32_t* row = thr.data() + ((size_t)s * A + a) * Sp;
      for (int s1 = 0; s1 < S; ++s1)
        if (row[s1] != (s1 ? row[s1 - 1] : 0u)) {
          const float t = law(row, s1);
          ent[fill[(size_t)a * S + s1]++] = make_uint2((uint32_t)s, __builtin_bit_cast(uint32_t, t));
        }
    }
  DevBuf n_bel[2], n_prior, n_cp, n_ent;
  int e;
  if ((e = n_bel[0].alloc((size_t)S * B * 4 + 16)) || (e = n_bel[1].alloc((size_t)S * B * 4 + 16)) ||
      (e = n_prior.upload(pr)) || (e = n_cp.upload(cp)) || (e = n_ent.upload(ent)))
    return e;
  auto take = [](DevBuf& dst, DevBuf& src) {
    std::swap(dst.p, src.p);
    std::swap(dst.n, src.n);
  };
  take(b_bel[0], n_bel[0]);
  take(b_bel[1], n_bel[1]);
  take(b_prior, n_prior);
  take(b_cp, n_cp);
  take(b_ent, n_ent);
  bf.bel[0] = b_bel[0].as<float>();
  bf.bel[1] = b_bel[1].as<float>();
  bf.prior = b_prior.as<float>();
  bf.colptr = b_cp.as<uint32_t>();
  bf.ent = b_ent.as<uint2>();
  bel_cur = 0;
  // on chip when both LDS buffers of a block fit the knob and, with the model blob, 60 KB
  const size_t need = (size_t)2 * S * EPB * sizeof(float);
  const int knob = gp_debug_knobs().belief_onchip_max;
  belief_oc = lds_env + need <= (size_t)60 * 1024 && (knob < 0 || need <= (size_t)knob);
  belief_on = true;
  if ((e = belief_grids()) || (e = belief_reset(nullptr))) {
    belief_disable();
    return e;
  }
  GP_HIP_CHECK(hipDeviceSynchronize());
  return GP_OK;
}

// N = 0 removes the policy. The vectors and their actions are validated, then uploaded into buffers of their own
// before anything is replaced.
int PomdpBackend::set_belief_policy(int n_vec, const float* alpha, const int32_t* vec_action) {
  if (n_vec == 0) {
    GP_HIP_CHECK(hipDeviceSynchronize());
    (void)b_alpha.alloc(0);
    (void)b_vact.alloc(0);
    bf.alpha = nullptr;
    bf.vact = nullptr;
    bf.N = 0;
    return GP_OK;
  }
  const int S = d.S;
  if (S > MAX_BELIEF_STATES) {
    gp_set_error("gp_set_belief_policy: %d states, the belief filter takes at most %d", S, MAX_BELIEF_STATES);
    return GP_E_INVALID;
  }
  if (n_vec < 0 || n_vec > MAX_VECTORS || (size_t)n_vec * S > MAX_ALPHA) {
    gp_set_error("gp_set_belief_policy: %d vectors over %d states (%zu entries): at most %d vectors and 2^22 entries",
                 n_vec, S, (size_t)(n_vec < 0 ? 0 : n_vec) * S, MAX_VECTORS);
    return GP_E_INVALID;
  }
  if (!alpha || !vec_action) {
    gp_set_error("gp_set_belief_policy: alpha and vec_action are required");
    return GP_E_INVALID;
  }
  for (size_t i = 0; i < (size_t)n_vec * S; ++i)
    if (!(alpha[i] >= -1e30f && alpha[i] <= 1e30f)) {
      gp_set_error("gp_set_belief_policy: alpha[%zu][%zu] = %g is not a finite value within +-1e30", i / S, i % S,
                   (double)alpha[i]);
      return GP_E_INVALID;
    }
  for (int j = 0; j < n_vec; ++j)
    if (vec_action[j] < 0 || vec_action[j] >= d.A) {
      gp_set_error("gp_set_belief_policy: vec_action[%d] = %d outside [0, %d)", j, vec_action[j], d.A);
      return GP_E_INVALID;
    }
  DevBuf n_alpha, n_vact;
  int e;
  if ((e = n_alpha.upload(std::vector<float>(alpha, alpha + (size_t)n_vec * S))) ||
      (e = n_vact.upload(std::vector<int32_t>(vec_action, vec_action + n_vec))))
    return e;
  GP_HIP_CHECK(hipDeviceSynchronize());
  std::swap(b_alpha.p, n_alpha.p);
  std::swap(b_alpha.n, n_alpha.n);
  std::swap(b_vact.p, n_vact.p);
  std::swap(b_vact.n, n_vact.n);
  bf.alpha = b_alpha.as<float>();
  bf.vact = b_vact.as<int32_t>();
  bf.N = n_vec;
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
