// gp_common.h — shared host/device helpers: 128-bit PCG64 arithmetic (numpy-compatible),
// Philox4x32-10, status packing for the decoupled-lookback reset scan, the tile plumbing of the env kernels (metric
// slots and their block reduction, StepOut, the 4-env quad accesses), error plumbing.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef unsigned __int128 u128;

#define GP_HD __host__ __device__ __forceinline__

// ---------------------------------------------------------------- PCG64 (XSL-RR 128/64) ----
// numpy/random/src/pcg64/pcg64.h: state = state * MULT + inc; out = rotr64(hi ^ lo, state >> 122).
static constexpr uint64_t PCG_MULT_HI = 0x2360ED051FC65DA4ULL;
static constexpr uint64_t PCG_MULT_LO = 0x4385DF649FCCF645ULL;

GP_HD u128 pcg_mult() { return ((u128)PCG_MULT_HI << 64) | PCG_MULT_LO; }
GP_HD u128 mk128(uint64_t hi, uint64_t lo) { return ((u128)hi << 64) | lo; }
GP_HD uint64_t hi64(u128 x) { return (uint64_t)(x >> 64); }
GP_HD uint64_t lo64(u128 x) { return (uint64_t)x; }

GP_HD uint64_t pcg_output(u128 s) {
  uint64_t x = hi64(s) ^ lo64(s);
  unsigned r = (unsigned)(s >> 122);
  return (x >> r) | (x << ((64u - r) & 63u));
}

// An affine jump s -> A*s + C (mod 2^128). Jumps compose: (A2,C2)o(A1,C1) = (A2*A1, A2*C1 + C2).
struct PcgJump {
  uint64_t a_hi, a_lo, c_hi, c_lo;
};

GP_HD u128 apply_jump(const PcgJump& j, u128 s) { return mk128(j.a_hi, j.a_lo) * s + mk128(j.c_hi, j.c_lo); }

// pcg_advance_lcg_128: (A, C) for `delta` LCG steps with increment `inc`.
static inline PcgJump pcg_jump_params(u128 delta, u128 inc) {
  u128 acc_mult = 1, acc_plus = 0, cur_mult = pcg_mult(), cur_plus = inc;
  while (delta > 0) {
    if (delta & 1) {
      acc_mult *= cur_mult;
      acc_plus = acc_plus * cur_mult + cur_plus;
    }
    cur_plus = (cur_mult + 1) * cur_plus;
    cur_mult *= cur_mult;
    delta >>= 1;
  }
  return PcgJump{hi64(acc_mult), lo64(acc_mult), hi64(acc_plus), lo64(acc_plus)};
}

// Radix-64 jump tables: level L, digit d -> jump by d * 64^L. JT_LEVELS levels cover 2^30 steps.
#define JT_LEVELS 5
#define JT_RADIX_BITS 6
#define JT_RADIX 64

// Jump state s by n (< 2^30) LCG steps using the tables (gathers from global memory, L1/L2 hot), one level's
// entry at a time (few live registers: the grid kernels' rare paths call this inside register-tight loops).
__device__ __forceinline__ u128 pcg_jump(const PcgJump* __restrict__ jt, u128 s, uint32_t n) {
#pragma unroll
  for (int L = 0; L < JT_LEVELS; ++L) {
    const uint32_t d = (n >> (JT_RADIX_BITS * L)) & (JT_RADIX - 1);
    if (d) s = apply_jump(jt[L * JT_RADIX + d], s);
  }
  return s;
}
// The same with every level's entry loaded up front (independent loads in flight together, then applied in
// order): for kernels with registers to spare (the C-ROOMS exact mode's draw calls). In the fused grid kernel
// the 40 extra live VGPRs of this form made every step ~40% slower (K = 128: 4.72 -> 6.67 us/step).
__device__ __forceinline__ u128 pcg_jump_ilp(const PcgJump* __restrict__ jt, u128 s, uint32_t n) {
  PcgJump e[JT_LEVELS];
#pragma unroll
  for (int L = 0; L < JT_LEVELS; ++L) e[L] = jt[L * JT_RADIX + ((n >> (JT_RADIX_BITS * L)) & (JT_RADIX - 1))];
#pragma unroll
  for (int L = 0; L < JT_LEVELS; ++L)
    if ((n >> (JT_RADIX_BITS * L)) & (JT_RADIX - 1)) s = apply_jump(e[L], s);
  return s;
}

__device__ __forceinline__ u128 pcg_step(u128 s, u128 inc) { return s * pcg_mult() + inc; }

// Lemire 32-bit bounded draw acceptance (numpy distributions.c buffered_bounded_lemire_uint32):
// rejected iff (word * n mod 2^32) < (2^32 - n) % n.
GP_HD bool lemire_rejected(uint32_t word, uint32_t n, uint32_t threshold) {
  return (uint32_t)((uint64_t)word * n) < threshold;
}
GP_HD uint32_t lemire_value(uint32_t word, uint32_t n) { return (uint32_t)(((uint64_t)word * n) >> 32); }
static inline uint32_t lemire_threshold(uint32_t n) { return (uint32_t)((0xFFFFFFFFu - (n - 1)) % n); }

// ---------------------------------------------------------------- Philox4x32-10 ----
struct Philox4 {
  uint32_t x[4];
};
// a ^ b ^ c: ONE gfx950 v_bitop3_b32 (truth table 0x96) on the device, where the compiler emits two v_xor_b32
// (gfx950 has no v_xor3_b32); Philox4x32-10 spends 2 of its 3 VALU ops per output word per round here.
GP_HD uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);
#else
  return a ^ b ^ c;
#endif
}
// Philox4x32-R (Salmon et al. 2011, "Parallel random numbers: as easy as 1, 2, 3"); R = 10 is Random123's default
// (every philox-mode kernel), R = 7 the fewest rounds the paper reports Crush-resistant (a C-ROOMS build option,
// csrc/crooms.hip CR_PHILOX_ROUNDS).
template <int R>
GP_HD Philox4 philox4x32(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
  const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    uint64_t p0 = (uint64_t)M0 * c0, p1 = (uint64_t)M1 * c2;
    uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0, hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
    uint32_t n0 = xor3(hi1, c1, k0), n2 = xor3(hi0, c3, k1);
    c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
    k0 += W0; k1 += W1;
  }
  Philox4 r; r.x[0] = c0; r.x[1] = c1; r.x[2] = c2; r.x[3] = c3;
  return r;
}
GP_HD Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
  return philox4x32<10>(c0, c1, c2, c3, k0, k1);
}

// ---------------------------------------------------------------- lookback status words ----
// 64-bit status per block: [63:62] flag (0 = not ready, 1 = aggregate, 2 = inclusive prefix),
// [61] rejection-seen bit, [31:0] reset count. Written/read as agent-scope atomics: the word IS
// the hand-off (MI355X_MICROARCH.md, Guideline 16 R2 granule form: one aligned 8-B sc1 store).
#define ST_FLAG_X 0ull
#define ST_FLAG_A 1ull
#define ST_FLAG_P 2ull
GP_HD uint64_t st_pack(uint64_t flag, uint32_t rej, uint32_t count) {
  return (flag << 62) | ((uint64_t)(rej & 1u) << 61) | (uint64_t)count;
}
GP_HD uint64_t st_flag(uint64_t s) { return s >> 62; }
GP_HD uint32_t st_rej(uint64_t s) { return (uint32_t)(s >> 61) & 1u; }
GP_HD uint32_t st_count(uint64_t s) { return (uint32_t)s; }

// ---------------------------------------------------------------- tile plumbing of the env kernels ----
// Per-block metric accumulators (each persistent block owns one slot); every kind's XxDev::mslot.
struct alignas(32) MetricSlot {
  double return_sum;
  unsigned long long episodes, length_sum, env_steps;
};
// The sum of n slots as gp_metrics reports it: episodes, return, length, env-steps.
inline void sum_metric_slots(const MetricSlot* m, size_t n, double out[4]) {
  out[0] = out[1] = out[2] = out[3] = 0;
  for (size_t i = 0; i < n; ++i) {
    out[0] += (double)m[i].episodes;
    out[1] += m[i].return_sum;
    out[2] += (double)m[i].length_sum;
    out[3] += (double)m[i].env_steps;
  }
}

// What one env-step hands back to its rollout kernel.
struct StepOut {
  float rew;
  uint8_t term, trunc;
};

// A block's metrics into its own slot p.mslot[blockIdx.x] (no other block writes it), p being the kind's XxDev: wave
// shuffles, the waves' partials through LDS, thread 0 adds them up. The law of gp_metrics (include/gym_po_amd.h):
// rsum is the thread's float64 sum of its float32 rewards and stays float64 through the shuffles, the LDS partials
// and the slot's +=; the three counters are 32-bit per thread (LT: Car-Flag's length sum is 64-bit) and 64-bit from
// the wave shuffle on, so a block's totals do not wrap at 2^32 env-steps a launch.
template <int NW, class Dev, class LT>
__device__ void block_metrics(const Dev& p, double rsum, uint32_t eps32, LT lens_t, uint32_t nst32) {
  __shared__ double s_r[NW];
  __shared__ unsigned long long s_e[NW], s_l[NW], s_n[NW];
  unsigned long long eps = eps32, lens = lens_t, nst = nst32;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    rsum += __shfl_xor(rsum, d, 64);
    eps += __shfl_xor(eps, d, 64);
    lens += __shfl_xor(lens, d, 64);
    nst += __shfl_xor(nst, d, 64);
  }
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0) { s_r[wid] = rsum; s_e[wid] = eps; s_l[wid] = lens; s_n[wid] = nst; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double r = 0.0;
    unsigned long long e = 0, l = 0, n = 0;
    for (int w = 0; w < NW; ++w) { r += s_r[w]; e += s_e[w]; l += s_l[w]; n += s_n[w]; }
    MetricSlot& m = p.mslot[blockIdx.x];
    m.return_sum += r;
    m.episodes += e;
    m.length_sum += l;
    m.env_steps += n;
  }
}

// A thread's 4 consecutive envs as one access (16 B of 4-byte elements, 8 B of 2-byte ones, 4 B of flags) when all 4
// are live and the address is aligned to it; else element by element (the ragged tail, caller buffers off their
// boundary): chosen per buffer and per step.
__device__ __forceinline__ bool quad_ok(const void* p, int env0, int B, int esz) {
  return env0 + 3 < B && ((((uintptr_t)p) + (size_t)env0 * esz) & (size_t)(4 * esz - 1)) == 0;
}
template <class T>
__device__ __forceinline__ void load4(const T* __restrict__ p, int env0, int B, T (&v)[4]) {
  if (quad_ok(p, env0, B, sizeof(T))) {
    if constexpr (sizeof(T) == 4) {
      uint4 q = *reinterpret_cast<const uint4*>(p + env0);
      v[0] = __builtin_bit_cast(T, q.x); v[1] = __builtin_bit_cast(T, q.y);
      v[2] = __builtin_bit_cast(T, q.z); v[3] = __builtin_bit_cast(T, q.w);
    } else if constexpr (sizeof(T) == 2) {
      uint2 q = *reinterpret_cast<const uint2*>(p + env0);
      v[0] = (T)(q.x & 0xFFFF); v[1] = (T)(q.x >> 16); v[2] = (T)(q.y & 0xFFFF); v[3] = (T)(q.y >> 16);
    } else {
      uint32_t q = *reinterpret_cast<const uint32_t*>(p + env0);
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = (T)((q >> (8 * i)) & 0xFFu);
    }
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = (env0 + i < B) ? p[env0 + i] : (T)0;
  }
}
template <class T>
__device__ __forceinline__ void store4(T* __restrict__ p, int env0, int B, const T (&v)[4]) {
  if (quad_ok(p, env0, B, sizeof(T))) {
    if constexpr (sizeof(T) == 4) {
      uint4 q;
      q.x = __builtin_bit_cast(uint32_t, v[0]); q.y = __builtin_bit_cast(uint32_t, v[1]);
      q.z = __builtin_bit_cast(uint32_t, v[2]); q.w = __builtin_bit_cast(uint32_t, v[3]);
      *reinterpret_cast<uint4*>(p + env0) = q;
    } else if constexpr (sizeof(T) == 2) {
      uint2 q;
      q.x = (uint32_t)(uint16_t)v[0] | ((uint32_t)(uint16_t)v[1] << 16);
      q.y = (uint32_t)(uint16_t)v[2] | ((uint32_t)(uint16_t)v[3] << 16);
      *reinterpret_cast<uint2*>(p + env0) = q;
    } else {
      uint32_t q = (uint32_t)(uint8_t)v[0] | ((uint32_t)(uint8_t)v[1] << 8) | ((uint32_t)(uint8_t)v[2] << 16) |
                   ((uint32_t)(uint8_t)v[3] << 24);
      *reinterpret_cast<uint32_t*>(p + env0) = q;
    }
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (env0 + i < B) p[env0 + i] = v[i];
  }
}

// ---------------------------------------------------------------- error plumbing ----
// Per-handle device error word (GridCtl::err, the other kinds' `derr`): kernels OR bits into it,
// gp_check / gp_metrics turn a nonzero word into GP_E_DEVICE. Sticky until the handle is re-seeded.
#define GP_DERR_TIMEOUT 1u  // a persistent kernel's cross-block wait gave up (blocks not co-resident)
#define GP_DERR_ACTION 2u   // an action outside [-n, n): the reference raises IndexError
                            // (msrooms.py:400 action_matrix[action], extended_taxi.py:248 ACTIONS_YX[actions])
#define GP_DERR_STREAM 4u   // C-ROOMS exact mode: a numpy normal needed more words than one window holds
#define GP_DERR_OVERFLOW 8u // windowed grid kernel slow path: more rejected choice() words than it can list
#define GP_DERR_BTPE 16u    // Taxi numpy mode: a multinomial reset needed numpy's BTPE binomial (p n > 30) or an
                            // inversion did not end, neither of which the device walker restates
#define GP_DERR_CTRL 32u    // closed-loop rollout: an obs outside the controller table's n_obs, or a node >= its
                            // node count (set through gp_controller_nodes): the device clamped it
#define GP_DERR_STATS 64u   // gp_controller_stats: a visit whose node, obs, action or next node lies outside the table,
                            // or whose return-to-go is not below 2^31 in magnitude (NaN included): the visit was skipped
#define GP_DERR_BELIEF 128u // POMDP belief filter: a step whose normaliser was not a positive finite number (the obs has
                            // probability zero under the stored belief): the belief was replaced by the prior
// numpy indexing of an n-row table accepts a in [-n, n) (negatives wrap); anything else raises.
__device__ __forceinline__ bool action_out_of_range(int a, int n) { return (uint32_t)(a + n) >= (uint32_t)(2 * n); }
__device__ __forceinline__ void flag_bad_action(uint32_t* derr) { atomicOr(derr, GP_DERR_ACTION); }
const char* gp_derr_text(uint32_t flags);  // api.hip: human-readable description of the set bits
void gp_set_error(const char* fmt, ...);
#define GP_HIP_CHECK(x)                                                                        \
  do {                                                                                         \
    hipError_t e_ = (x);                                                                       \
    if (e_ != hipSuccess) {                                                                    \
      gp_set_error("%s:%d %s -> %s", __FILE__, __LINE__, #x, hipGetErrorString(e_));           \
      return GP_E_HIP;                                                                         \
    }                                                                                          \
  } while (0)
