// carflag.hip — Car-Flag (GP_KIND_CARFLAG): the 1-D heaven/hell POMDP of gym_po/envs/car_flag.py
// (CarVecEnv :50-144, DiscreteActionCarVecEnv :286-303), restated.
//
// Rules (DESIGN.md §"Car-Flag", tests/carflag_oracle.py restates them in numpy):
//   state   s = (position, velocity, direction) f32, heaven +-1, priest +-0.5, elapsed
//   step    elapsed += 1; force = clip(a, +-1); v' = clip(v + force * 0.0015, +-0.07); x' = clip(x + v', +-1.1);
//           terminated = |x'| >= 1, reward +1 when sign(x') is the heaven side, -1 on the hell side, else 0;
//           truncated = elapsed >= time_limit; direction = heaven while priest - 0.2 <= x' <= priest + 0.2
//           (float64 compare), else 0; a non-terminated env stores (x', v', direction); terminated | truncated
//           envs reset in the same step and the observation is the state after that reset
//   reset   x = -0.2 + 0.4 * (k53 * 2^-53) in float64 (two roundings) rounded to f32, v = direction = 0,
//           heaven = (-1, 1)[bit], priest = (-0.5, 0.5)[bit]
//   arithmetic  float32 actions: every operation in float32 (the constants rounded to f32 first, NEP 50);
//           float64 actions and the discrete table (np.linspace, f64): v', x' in float64 from the f32 state,
//           rounded to f32 only when stored. Never a fused multiply-add: the reference rounds twice.
// State per env: ONE 16-B word (x, v, direction, heaven bit | priest bit << 1 | elapsed << 2), in registers
// across a rollout.
// RNG: philox (one block per (key, env, step): words 0-1 the 53-bit uniform, the top bits of words 2 / 3 the
// heaven / priest choice), replay (caller-decided k53 / indices), numpy (the PCG64 stream in numpy's order: a
// reset of b envs, ascending env index, takes b words for uniform() and then 2 b 32-bit halves, low half
// first, for the two choice(., b) calls; see cf_resolve).
#include <vector>

#include "gp_internal.h"

// The reference rounds after every multiply and add, so nothing in this file may contract into a fused
// multiply-add. Plain operators under this pragma, not the __fmul_rn / __dadd_rn forms: those are ordinary
// operators in a runtime header compiled with contraction on, and after inlining they did fuse here
// (v_fmac_f64 in the reset's -0.2 + 0.4 u).
#pragma clang fp contract(off)

namespace {

constexpr int TPB = 256;
constexpr int EPT = 4;
constexpr int EPB = TPB * EPT;
constexpr int WAVES = TPB / 64;
constexpr uint32_t TAG = 0x63666c31u;       // 'cfl1'
constexpr uint32_t EL_PENDING = 0x3FFFFFFFu;  // elapsed field of an env whose numpy-mode reset is not resolved yet
constexpr int MAX_TIME_LIMIT = 1 << 29;

enum { ACT_F32 = 0, ACT_F64 = 1, ACT_DISC = 2 };
enum { M_PHILOX = 0, M_REPLAY = 1, M_NUMPY = 2 };

// numpy's PCG64 position on the device (the increment stays on the host: the jump tables carry it)
struct alignas(32) CfRng {
  uint64_t s_hi, s_lo;
  uint32_t has_u32, uinteger;
  uint64_t pad;
};

struct CfDev {
  int32_t B, ntiles, time_limit, nact;
  uint32_t key0, key1;
  float4* st;               // [B] x, v, direction, bits(heaven | priest << 1 | elapsed << 2)
  const double* table;      // [nact] discrete action table (np.linspace(-1, 1, n))
  MetricSlot* mslot;
  uint32_t* derr;
  uint32_t* tile_cnt;       // numpy mode: pending resets per tile of the current step
  const PcgJump* jt;        // numpy mode: radix-64 jump tables of the stream's increment
  CfRng* rng;               // numpy mode: [2], the live one chosen by the launch's parity
  const uint64_t* rp_u;     // replay: k53 of the reset uniform [B]
  const int32_t* rp_h;      // replay: heaven index [B]
  const int32_t* rp_p;      // replay: priest index [B]
};

struct CfEnv {
  float x, v, dir;
  uint32_t w;
};

template <int ACT> struct ActT { typedef float type; };
template <> struct ActT<ACT_F64> { typedef double type; };
template <> struct ActT<ACT_DISC> { typedef int32_t type; };

__device__ __forceinline__ float clipf(float x, float lo, float hi) { return x < lo ? lo : (x > hi ? hi : x); }
__device__ __forceinline__ double clipd(double x, double lo, double hi) { return x < lo ? lo : (x > hi ? hi : x); }

// uniform(-0.2, 0.2): loc + scale * next_double, float64 without contraction, stored as f32
__device__ __forceinline__ float reset_x(uint64_t k53) {
  const double u = (double)k53 * 0x1.0p-53;
  return (float)(-0.2 + 0.4 * u);
}
__device__ __forceinline__ void set_reset(CfEnv& e, uint64_t k53, uint32_t hbit, uint32_t pbit) {
  e.x = reset_x(k53);
  e.v = 0.f;
  e.dir = 0.f;
  e.w = (hbit & 1u) | ((pbit & 1u) << 1);
}

// One env, one step (reset excluded). F64: the float64-action arithmetic.
template <bool F64>
__device__ __forceinline__ StepOut cf_dyn(const CfDev& p, CfEnv& e, double a64, float a32) {
  const float heaven = (e.w & 1u) ? 1.f : -1.f;
  const double priest = (e.w & 2u) ? 0.5 : -0.5;
  float xs, vs;
  double xd;
  bool term;
  if constexpr (F64) {
    const double f = clipd(a64, -1.0, 1.0);
    const double nv = clipd((double)e.v + f * 0.0015, -0.07, 0.07);
    const double nx = clipd((double)e.x + nv, -1.1, 1.1);
    term = fabs(nx) >= 1.0;
    xd = nx;
    xs = (float)nx;
    vs = (float)nv;
  } else {
    const float f = clipf(a32, -1.f, 1.f);
    const float nv = clipf(e.v + f * 0.0015f, -0.07f, 0.07f);
    const float nx = clipf(e.x + nv, -1.1f, 1.1f);
    term = fabsf(nx) >= 1.0f;
    xd = (double)nx;
    xs = nx;
    vs = nv;
  }
  const float sgn = xd > 0.0 ? 1.f : (xd < 0.0 ? -1.f : 0.f);
  StepOut o;
  o.term = term ? 1 : 0;
  o.rew = term ? (sgn == heaven ? 1.f : -1.f) : 0.f;
  const uint32_t el = min((e.w >> 2) + 1u, EL_PENDING - 1u);
  o.trunc = el >= (uint32_t)p.time_limit ? 1 : 0;
  const bool zone = xd >= priest - 0.2 && xd <= priest + 0.2;
  if (!term) {
    e.x = xs;
    e.v = vs;
    e.dir = zone ? heaven : 0.f;
  }
  e.w = (e.w & 3u) | (el << 2);
  return o;
}

__device__ __forceinline__ bool al16(const void* q) { return (((uintptr_t)q) & 15) == 0; }

// Four actions of one thread: 16-B loads where the address allows, scalars at the ragged end.
template <int ACT>
__device__ __forceinline__ void load_act(const typename ActT<ACT>::type* __restrict__ act, size_t off, int env0, int B,
                                         typename ActT<ACT>::type (&a)[EPT]) {
  typedef typename ActT<ACT>::type T;
  const T* q = act + off + env0;
  if (env0 + EPT - 1 < B && al16(q)) {
    if constexpr (sizeof(T) == 8) {
      const double2 lo = reinterpret_cast<const double2*>(q)[0], hi = reinterpret_cast<const double2*>(q)[1];
      a[0] = lo.x; a[1] = lo.y; a[2] = hi.x; a[3] = hi.y;
    } else if constexpr (ACT == ACT_F32) {
      const float4 v = *reinterpret_cast<const float4*>(q);
      a[0] = v.x; a[1] = v.y; a[2] = v.z; a[3] = v.w;
    } else {
      const int4 v = *reinterpret_cast<const int4*>(q);
      a[0] = v.x; a[1] = v.y; a[2] = v.z; a[3] = v.w;
    }
  } else {
#pragma unroll
    for (int i = 0; i < EPT; ++i) a[i] = env0 + i < B ? q[i] : (T)0;
  }
}

// K steps of every tile with the tile's state in registers. MODE numpy runs with K = 1: an env that has to
// reset is only marked (EL_PENDING) and counted per tile; cf_resolve gives it its draws.
template <int ACT, int MODE>
__global__ __launch_bounds__(TPB) void cf_rollout(CfDev p, int K, uint64_t step0,
                                                  const typename ActT<ACT>::type* __restrict__ act,
                                                  float* __restrict__ obs, float* __restrict__ rew,
                                                  uint8_t* __restrict__ term, uint8_t* __restrict__ trunc) {
  typedef typename ActT<ACT>::type T;
  __shared__ float4 s_obs[TPB * 3];  // per-wave obs transpose: 4 envs x 3 f32 per lane -> lane-contiguous 16-B stores
  __shared__ uint32_t s_cnt[WAVES];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  float4* wv = s_obs + wid * 64 * 3;
  double rsum = 0.0;
  uint32_t eps = 0, nst = 0;
  // lens is 64-bit from the thread on: one episode can be 2^29 steps long (MAX_TIME_LIMIT), so four envs of a thread
  // that end together already sum to 2^31 and two such threads wrapped a 32-bit wave sum to 0 (block_metrics' LT)
  unsigned long long lens = 0;
  for (int tile = blockIdx.x; tile < p.ntiles; tile += gridDim.x) {
    const int env0 = tile * EPB + threadIdx.x * EPT;
    CfEnv e[EPT];
#pragma unroll
    for (int i = 0; i < EPT; ++i) {
      const float4 q = env0 + i < p.B ? p.st[env0 + i] : make_float4(0.f, 0.f, 0.f, 0.f);
      e[i].x = q.x; e[i].v = q.y; e[i].dir = q.z; e[i].w = __float_as_uint(q.w);
    }
    T a_nxt[EPT];
    if (K > 0) load_act<ACT>(act, 0, env0, p.B, a_nxt);
    for (int k = 0; k < K; ++k) {
      const size_t off = (size_t)k * p.B;
      T a[EPT];
#pragma unroll
      for (int i = 0; i < EPT; ++i) a[i] = a_nxt[i];
      if (k + 1 < K) load_act<ACT>(act, off + p.B, env0, p.B, a_nxt);  // one step ahead
      float r[EPT];
      uint8_t tm[EPT], tr[EPT];
#pragma unroll
      for (int i = 0; i < EPT; ++i) {
        const int env = env0 + i;
        const bool live = env < p.B;
        StepOut o;
        if constexpr (ACT == ACT_F32) {
          o = cf_dyn<false>(p, e[i], 0.0, a[i]);
        } else if constexpr (ACT == ACT_F64) {
          o = cf_dyn<true>(p, e[i], a[i], 0.f);
        } else {
          int ai = a[i];
          if (live && action_out_of_range(ai, p.nact)) flag_bad_action(p.derr);
          if (ai < 0) ai += p.nact;
          ai = min(max(ai, 0), p.nact - 1);
          o = cf_dyn<true>(p, e[i], p.table[ai], 0.f);
        }
        r[i] = o.rew;
        tm[i] = o.term;
        tr[i] = o.trunc;
        if (live) {
          nst += 1u;
          rsum += (double)o.rew;
          if (o.term | o.trunc) {
            eps += 1u;
            lens += (unsigned long long)(e[i].w >> 2);
            if constexpr (MODE == M_NUMPY) {
              e[i].w = (e[i].w & 3u) | (EL_PENDING << 2);
            } else if constexpr (MODE == M_REPLAY) {
              set_reset(e[i], p.rp_u[env] & ((1ull << 53) - 1), p.rp_h[env] != 0, p.rp_p[env] != 0);
            } else {
              const uint64_t step = step0 + (uint64_t)k;
              const Philox4 g = philox4x32_10((uint32_t)env, (uint32_t)step, (uint32_t)(step >> 32), TAG, p.key0, p.key1);
              set_reset(e[i], (((uint64_t)g.x[1] << 32) | g.x[0]) >> 11, g.x[2] >> 31, g.x[3] >> 31);
            }
          }
        }
      }
      float* rw = rew + off + env0;
      uint8_t* tmp = term + off + env0;
      uint8_t* trp = trunc + off + env0;
      if (env0 + EPT - 1 < p.B && al16(rw) && ((((uintptr_t)tmp) | ((uintptr_t)trp)) & 3) == 0) {
        *reinterpret_cast<float4*>(rw) = make_float4(r[0], r[1], r[2], r[3]);
        *reinterpret_cast<uint32_t*>(tmp) =
            (uint32_t)tm[0] | ((uint32_t)tm[1] << 8) | ((uint32_t)tm[2] << 16) | ((uint32_t)tm[3] << 24);
        *reinterpret_cast<uint32_t*>(trp) =
            (uint32_t)tr[0] | ((uint32_t)tr[1] << 8) | ((uint32_t)tr[2] << 16) | ((uint32_t)tr[3] << 24);
      } else {
#pragma unroll
        for (int i = 0; i < EPT; ++i)
          if (env0 + i < p.B) { rw[i] = r[i]; tmp[i] = tm[i]; trp[i] = tr[i]; }
      }
      // obs: a lane's 4 envs are 48 contiguous bytes; through LDS each store instruction writes 1 KB of the
      // wave's 3 KB instead of 16 B at a 48-B stride
      wv[lane * 3 + 0] = make_float4(e[0].x, e[0].v, e[0].dir, e[1].x);
      wv[lane * 3 + 1] = make_float4(e[1].v, e[1].dir, e[2].x, e[2].v);
      wv[lane * 3 + 2] = make_float4(e[2].dir, e[3].x, e[3].v, e[3].dir);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
      const int wenv0 = tile * EPB + wid * 64 * EPT;
      const int nvalid = 3 * min(max(p.B - wenv0, 0), 64 * EPT);  // floats of this wave that exist
      float* ow = obs + (off + (size_t)wenv0) * 3;
      if (al16(ow)) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const int q = j * 64 + lane;
          if (4 * q + 4 <= nvalid) {
            reinterpret_cast<float4*>(ow)[q] = wv[q];
          } else {
            const float* wf = reinterpret_cast<const float*>(wv);
            for (int c = 4 * q; c < nvalid; ++c) ow[c] = wf[c];
          }
        }
      } else {
        const float* wf = reinterpret_cast<const float*>(wv);
#pragma unroll
        for (int j = 0; j < 12; ++j) {
          const int c = j * 64 + lane;
          if (c < nvalid) ow[c] = wf[c];
        }
      }
    }
#pragma unroll
    for (int i = 0; i < EPT; ++i)
      if (env0 + i < p.B) p.st[env0 + i] = make_float4(e[i].x, e[i].v, e[i].dir, __uint_as_float(e[i].w));
    if constexpr (MODE == M_NUMPY) {
      uint32_t c = 0;
#pragma unroll
      for (int i = 0; i < EPT; ++i) c += (env0 + i < p.B && (e[i].w >> 2) == EL_PENDING) ? 1u : 0u;
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d, 64);
      if (lane == 0) s_cnt[wid] = c;
      __syncthreads();
      if (threadIdx.x == 0) p.tile_cnt[tile] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
      __syncthreads();
    }
  }
  block_metrics<WAVES>(p, rsum, eps, lens, nst);
}

// Numpy-mode resets of one step (ALL: of reset(), every env). One block per tile. With b the number of
// resetting envs and r an env's rank among them in env order, from stream position s (word j = output of s
// advanced j + 1 times): uniform <- word r; the 2 b halves that follow (a buffered half first when the stream
// holds one, then words b .., low half before high) give heaven <- half r and priest <- half b + r. The stream
// moves 2 b words; the last word's high half stays in `uinteger`, buffered iff one was buffered before.
template <bool ALL>
__global__ __launch_bounds__(TPB) void cf_resolve(CfDev p, int par, float* __restrict__ obs) {
  __shared__ uint32_t s_a[WAVES], s_b[WAVES];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int tile = blockIdx.x;
  uint32_t pre = 0, tot = 0;
  if constexpr (ALL) {
    pre = (uint32_t)tile * EPB;
    tot = (uint32_t)p.B;
  } else {
    for (int i = threadIdx.x; i < p.ntiles; i += TPB) {
      const uint32_t c = p.tile_cnt[i];
      tot += c;
      pre += i < tile ? c : 0u;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      pre += __shfl_xor(pre, d, 64);
      tot += __shfl_xor(tot, d, 64);
    }
    if (lane == 0) { s_a[wid] = pre; s_b[wid] = tot; }
    __syncthreads();
    pre = s_a[0] + s_a[1] + s_a[2] + s_a[3];
    tot = s_b[0] + s_b[1] + s_b[2] + s_b[3];
    __syncthreads();
  }
  const CfRng g = p.rng[par];
  const u128 s = mk128(g.s_hi, g.s_lo);
  if (tile == 0 && threadIdx.x == 0) {
    CfRng n = g;
    if (tot) {
      const u128 s2 = pcg_jump(p.jt, s, 2u * tot);
      n.s_hi = hi64(s2);
      n.s_lo = lo64(s2);
      n.uinteger = (uint32_t)(pcg_output(s2) >> 32);
    }
    p.rng[par ^ 1] = n;
  }
  if (tot == 0) return;
  const int env0 = tile * EPB + threadIdx.x * EPT;
  float4 q[EPT];
  bool f[EPT];
  uint32_t c = 0;
#pragma unroll
  for (int i = 0; i < EPT; ++i) {
    const bool live = env0 + i < p.B;
    q[i] = live ? p.st[env0 + i] : make_float4(0.f, 0.f, 0.f, 0.f);
    f[i] = live && (ALL || (__float_as_uint(q[i].w) >> 2) == EL_PENDING);
    c += f[i] ? 1u : 0u;
  }
  uint32_t inc = c;  // inclusive scan over the wave, then over the block's waves
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t t = __shfl_up(inc, d, 64);
    if (lane >= d) inc += t;
  }
  if (lane == 63) s_a[wid] = inc;
  __syncthreads();
  uint32_t rank = pre + inc - c;
  for (int w = 0; w < wid; ++w) rank += s_a[w];
  auto half = [&](uint32_t k) -> uint32_t {  // the k-th 32-bit draw after the b uniform words
    if (g.has_u32) {
      if (k == 0) return g.uinteger;
      k -= 1u;
    }
    const uint64_t w = pcg_output(pcg_jump(p.jt, s, tot + (k >> 1) + 1u));
    return (k & 1u) ? (uint32_t)(w >> 32) : (uint32_t)w;
  };
#pragma unroll
  for (int i = 0; i < EPT; ++i) {
    if (!f[i]) continue;
    const uint32_t r = rank++;
    const uint64_t wu = pcg_output(pcg_jump(p.jt, s, r + 1u));
    CfEnv e;
    set_reset(e, wu >> 11, half(r) >> 31, half(tot + r) >> 31);
    const int env = env0 + i;
    p.st[env] = make_float4(e.x, e.v, e.dir, __uint_as_float(e.w));
    obs[(size_t)env * 3 + 0] = e.x;
    obs[(size_t)env * 3 + 1] = e.v;
    obs[(size_t)env * 3 + 2] = e.dir;
  }
}

// reset() of the philox / replay modes
template <bool REPLAY>
__global__ __launch_bounds__(TPB) void cf_reset(CfDev p, uint64_t step, float* __restrict__ obs) {
  const int env = blockIdx.x * TPB + threadIdx.x;
  if (env >= p.B) return;
  CfEnv e;
  if constexpr (REPLAY) {
    set_reset(e, p.rp_u[env] & ((1ull << 53) - 1), p.rp_h[env] != 0, p.rp_p[env] != 0);
  } else {
    const Philox4 g = philox4x32_10((uint32_t)env, (uint32_t)step, (uint32_t)(step >> 32), TAG, p.key0, p.key1);
    set_reset(e, (((uint64_t)g.x[1] << 32) | g.x[0]) >> 11, g.x[2] >> 31, g.x[3] >> 31);
  }
  p.st[env] = make_float4(e.x, e.v, e.dir, __uint_as_float(e.w));
  obs[(size_t)env * 3 + 0] = e.x;
  obs[(size_t)env * 3 + 1] = e.v;
  obs[(size_t)env * 3 + 2] = e.dir;
}

__global__ void cf_get_state(CfDev p, float* s3, int32_t* el, float* heavens, float* priests) {
  const int env = blockIdx.x * TPB + threadIdx.x;
  if (env >= p.B) return;
  const float4 q = p.st[env];
  const uint32_t w = __float_as_uint(q.w);
  if (s3) { s3[(size_t)env * 3] = q.x; s3[(size_t)env * 3 + 1] = q.y; s3[(size_t)env * 3 + 2] = q.z; }
  if (el) el[env] = (int32_t)(w >> 2);
  if (heavens) heavens[env] = (w & 1u) ? 1.f : -1.f;
  if (priests) priests[env] = (w & 2u) ? 0.5f : -0.5f;
}
// heavens / priests are taken by sign; elapsed is clamped to [0, MAX_TIME_LIMIT]
__global__ void cf_set_state(CfDev p, const float* s3, const int32_t* el, const float* heavens, const float* priests) {
  const int env = blockIdx.x * TPB + threadIdx.x;
  if (env >= p.B) return;
  float4 q = p.st[env];
  uint32_t w = __float_as_uint(q.w);
  if (s3) { q.x = s3[(size_t)env * 3]; q.y = s3[(size_t)env * 3 + 1]; q.z = s3[(size_t)env * 3 + 2]; }
  if (el) w = (w & 3u) | ((uint32_t)min(max(el[env], 0), MAX_TIME_LIMIT) << 2);
  if (heavens) w = (w & ~1u) | (heavens[env] > 0.f ? 1u : 0u);
  if (priests) w = (w & ~2u) | (priests[env] > 0.f ? 2u : 0u);
  q.w = __uint_as_float(w);
  p.st[env] = q;
}

// ------------------------------------------------------------------ host backend ----
struct CarFlagBackend : EnvBackend {
  CfDev d{};
  int act = ACT_F32;
  int grid = 1;
  int par = 0;  // which of the two device stream records is live (numpy mode)
  uint64_t philox_step = 0;
  DevBuf b_st, b_slot, b_table, b_cnt, b_jt, b_rng;
  DevErr derr;

  int build(const gp_carflag_config* cfg);

  int upload_rng() {
    const std::vector<PcgJump> jt = build_jump_tables(rng.inc);
    GP_HIP_CHECK(hipDeviceSynchronize());
    GP_HIP_CHECK(hipMemcpy(b_jt.p, jt.data(), jt.size() * sizeof(PcgJump), hipMemcpyHostToDevice));
    CfRng g{hi64(rng.state), lo64(rng.state), rng.has_u32 ? 1u : 0u, rng.uinteger, 0};
    par = 0;
    GP_HIP_CHECK(hipMemcpy(b_rng.p, &g, sizeof(g), hipMemcpyHostToDevice));
    return GP_OK;
  }
  int seed(const RngHost& r, const uint32_t key[2]) override {
    rng = r;
    d.key0 = key[0];
    d.key1 = key[1];
    philox_step = 0;
    if (rng_mode == GP_RNG_NUMPY) {
      int e = upload_rng();
      if (e) return e;
    }
    return derr.clear();
  }
  int check() override { return derr.check("carflag"); }
  int set_rng_state(const RngHost& r) override {
    if (rng_mode != GP_RNG_NUMPY) {
      gp_set_error("carflag: the PCG64 stream is used on the device only with rng_mode numpy");
      return GP_E_UNSUPPORTED;
    }
    rng = r;
    return upload_rng();
  }
  int get_rng_state(RngHost* r) override {
    if (rng_mode != GP_RNG_NUMPY) {
      gp_set_error("carflag: the PCG64 stream is used on the device only with rng_mode numpy");
      return GP_E_UNSUPPORTED;
    }
    GP_HIP_CHECK(hipDeviceSynchronize());
    CfRng g;
    GP_HIP_CHECK(hipMemcpy(&g, b_rng.as<CfRng>() + par, sizeof(g), hipMemcpyDeviceToHost));
    rng.state = mk128(g.s_hi, g.s_lo);
    rng.has_u32 = g.has_u32;
    rng.uinteger = g.uinteger;
    *r = rng;
    return check();
  }
  bool replay_ready() const { return d.rp_u && d.rp_h && d.rp_p; }
  int reset(void* obs, hipStream_t s) override {
    GP_HIP_CHECK(hipMemsetAsync(d.mslot, 0, sizeof(MetricSlot) * grid, s));
    const unsigned nb = (unsigned)((B + TPB - 1) / TPB);
    if (rng_mode == GP_RNG_NUMPY) {
      hipLaunchKernelGGL(cf_resolve<true>, dim3(d.ntiles), dim3(TPB), 0, s, d, par, (float*)obs);
      par ^= 1;
    } else if (rng_mode == GP_RNG_REPLAY) {
      if (!replay_ready()) {
        gp_set_error("carflag replay reset needs the uniform k53 (u), heaven (i0) and priest (i1) draws");
        return GP_E_STATE;
      }
      hipLaunchKernelGGL(cf_reset<true>, dim3(nb), dim3(TPB), 0, s, d, (uint64_t)0, (float*)obs);
    } else {
      hipLaunchKernelGGL(cf_reset<false>, dim3(nb), dim3(TPB), 0, s, d, philox_step, (float*)obs);
      ++philox_step;
    }
    GP_HIP_CHECK(hipGetLastError());
    has_reset = true;
    return GP_OK;
  }
  template <int MODE>
  void launch(int K, uint64_t step0, const void* a, void* obs, float* rew, uint8_t* term, uint8_t* trunc, hipStream_t s) {
    if (act == ACT_F32)
      hipLaunchKernelGGL((cf_rollout<ACT_F32, MODE>), dim3(grid), dim3(TPB), 0, s, d, K, step0, (const float*)a,
                         (float*)obs, rew, term, trunc);
    else if (act == ACT_F64)
      hipLaunchKernelGGL((cf_rollout<ACT_F64, MODE>), dim3(grid), dim3(TPB), 0, s, d, K, step0, (const double*)a,
                         (float*)obs, rew, term, trunc);
    else
      hipLaunchKernelGGL((cf_rollout<ACT_DISC, MODE>), dim3(grid), dim3(TPB), 0, s, d, K, step0, (const int32_t*)a,
                         (float*)obs, rew, term, trunc);
  }
  int rollout(int K, const void* a, void* obs, float* rew, uint8_t* term, uint8_t* trunc, hipStream_t s) override {
    if (!has_reset) {
      gp_set_error("step() before reset()");
      return GP_E_STATE;
    }
    if (rng_mode == GP_RNG_PHILOX) {
      timer.begin(s);
      launch<M_PHILOX>(K, philox_step, a, obs, rew, term, trunc, s);
      timer.end(s);
      philox_step += (uint64_t)K;
    } else {
      if (K > 1) return EnvBackend::rollout(K, a, obs, rew, term, trunc, s);  // K step launches
      if (rng_mode == GP_RNG_REPLAY) {
        if (!replay_ready()) {
          gp_set_error("carflag replay step needs the uniform k53 (u), heaven (i0) and priest (i1) draws");
          return GP_E_STATE;
        }
        timer.begin(s);
        launch<M_REPLAY>(1, 0, a, obs, rew, term, trunc, s);
        timer.end(s);
      } else {
        timer.begin(s);
        launch<M_NUMPY>(1, 0, a, obs, rew, term, trunc, s);
        timer.end(s);
        GP_HIP_CHECK(hipGetLastError());
        timer2.begin(s);
        hipLaunchKernelGGL(cf_resolve<false>, dim3(d.ntiles), dim3(TPB), 0, s, d, par, (float*)obs);
        timer2.end(s);
        par ^= 1;
      }
    }
    GP_HIP_CHECK(hipGetLastError());
    return GP_OK;
  }
  int step(const void* a, void* obs, float* rew, uint8_t* term, uint8_t* trunc, hipStream_t s) override {
    return rollout(1, a, obs, rew, term, trunc, s);
  }
  size_t rollout_action_bytes_per_env() const override { return act == ACT_F64 ? 8 : 4; }
  int get_state(void* a, void* b, void* c, void* dd, hipStream_t s) override {
    hipLaunchKernelGGL(cf_get_state, dim3((unsigned)((B + TPB - 1) / TPB)), dim3(TPB), 0, s, d, (float*)a, (int32_t*)b,
                       (float*)c, (float*)dd);
    GP_HIP_CHECK(hipGetLastError());
    return GP_OK;
  }
  int set_state(const void* a, const void* b, const void* c, const void* dd, hipStream_t s) override {
    hipLaunchKernelGGL(cf_set_state, dim3((unsigned)((B + TPB - 1) / TPB)), dim3(TPB), 0, s, d, (const float*)a,
                       (const int32_t*)b, (const float*)c, (const float*)dd);
    GP_HIP_CHECK(hipGetLastError());
    has_reset = true;
    return GP_OK;
  }
  // replay: u -> k53 of the reset uniform (uint64 [B]), i0 -> heaven index, i1 -> priest index (int32 [B])
  int set_replay(const void* u, const void* i0, const void* i1, const void*, const void*) override {
    if (rng_mode != GP_RNG_REPLAY) {
      gp_set_error("gp_set_replay requires GP_RNG_REPLAY");
      return GP_E_STATE;
    }
    d.rp_u = (const uint64_t*)u;
    d.rp_h = (const int32_t*)i0;
    d.rp_p = (const int32_t*)i1;
    return GP_OK;
  }
  int metrics(double out[4]) override {
    GP_HIP_CHECK(hipDeviceSynchronize());
    std::vector<MetricSlot> m(grid);
    GP_HIP_CHECK(hipMemcpy(m.data(), d.mslot, sizeof(MetricSlot) * grid, hipMemcpyDeviceToHost));
    sum_metric_slots(m.data(), m.size(), out);
    return check();
  }
};

int CarFlagBackend::build(const gp_carflag_config* cfg) {
  if (cfg->time_limit < 1 || cfg->time_limit > MAX_TIME_LIMIT) {
    gp_set_error("carflag: time_limit %d outside [1, %d]", cfg->time_limit, MAX_TIME_LIMIT);
    return GP_E_INVALID;
  }
  if (cfg->action_kind < 0 || (cfg->action_kind >= 2 && !cfg->action_table)) {
    gp_set_error("carflag: action_kind %d needs 0 (float32), 1 (float64) or n >= 2 with an n-entry action_table",
                 cfg->action_kind);
    return GP_E_INVALID;
  }
  act = cfg->action_kind == 0 ? ACT_F32 : (cfg->action_kind == 1 ? ACT_F64 : ACT_DISC);
  int e;
  d.nact = 0;
  if (act == ACT_DISC) {
    d.nact = cfg->action_kind;
    std::vector<double> t(cfg->action_table, cfg->action_table + d.nact);
    if ((e = b_table.upload(t))) return e;
    d.table = b_table.as<double>();
  }
  d.B = (int32_t)B;
  d.ntiles = (int32_t)((B + EPB - 1) / EPB);
  d.time_limit = cfg->time_limit;
  obs_dtype = GP_DTYPE_F32;
  obs_width = 3;
  if ((e = b_st.alloc((size_t)B * sizeof(float4)))) return e;
  d.st = b_st.as<float4>();
  hipDeviceProp_t prop;
  GP_HIP_CHECK(hipGetDeviceProperties(&prop, device));
  int occ = 0;
  GP_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, cf_rollout<ACT_F32, M_PHILOX>, TPB, 0));
  grid = persistent_grid(d.ntiles, prop.multiProcessorCount, occ);
  persist_grid = grid;
  persist_occ = occ;
  if ((e = b_slot.alloc(sizeof(MetricSlot) * grid))) return e;
  d.mslot = b_slot.as<MetricSlot>();
  if ((e = derr.alloc())) return e;
  d.derr = derr.ptr();
  if (rng_mode == GP_RNG_NUMPY) {
    if ((e = b_cnt.alloc((size_t)d.ntiles * 4))) return e;
    d.tile_cnt = b_cnt.as<uint32_t>();
    if ((e = b_jt.alloc((size_t)JT_LEVELS * JT_RADIX * sizeof(PcgJump)))) return e;
    d.jt = b_jt.as<PcgJump>();
    if ((e = b_rng.alloc(2 * sizeof(CfRng)))) return e;
    d.rng = b_rng.as<CfRng>();
  }
  return GP_OK;
}

}  // namespace

std::unique_ptr<EnvBackend> make_carflag_backend(const gp_carflag_config* cfg, int64_t B, int device, int rng_mode,
                                                 int* err) {
  // numpy mode jumps the stream by up to 2 B + 1 words with the 2^30-step tables
  const int64_t bmax = rng_mode == GP_RNG_NUMPY ? (int64_t)1 << 28 : (int64_t)1 << 30;
  if (B < 1 || B > bmax) {
    gp_set_error("carflag: num_envs %lld out of range [1, %lld]", (long long)B, (long long)bmax);
    *err = GP_E_INVALID;
    return nullptr;
  }
  if (hipSetDevice(device) != hipSuccess) {
    gp_set_error("carflag: hipSetDevice(%d) failed", device);
    *err = GP_E_HIP;
    return nullptr;
  }
  auto be = std::make_unique<CarFlagBackend>();
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
