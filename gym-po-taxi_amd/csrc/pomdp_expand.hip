// pomdp_expand.hip — the belief-set expansion of the tabular POMDP (gp_belief_expand): for every belief
// point the successor under the filter that lies farthest, in L1, from a reference set (Pineau, Gordon & Thrun 2003,
// "stochastic simulation with exploratory action", taken over every (action, obs) instead of one sampled obs per
// action). Build-defined; pinned bit for bit to tests/expand_oracle.py.
//
// Rule. The float laws Tf, Zf, terminal and the arithmetic are the belief filter's (pomdp.hip): float32, every
// product, difference, quotient and sum rounded on its own (contraction is off in this file: no FMA), sums sequential
// in ascending index from +0, the first maximiser wins (replaced only on a strict >). Points b[P][S] and a reference
// set q[Q][S] (NULL: the points themselves, Q = P) are finite and >= 0 and are used as given, not normalised. For
// every point, action a and obs o:
//   1. acc_a(s') = sum_s fl(b[s] Tf[s][a][s'])                                     (pb_acc, the backup's step 1)
//   2. u(s') = terminal[s'] ? +0 : fl(Zf[a][s'][o] acc_a(s'));  n(a, o) = sum_s' u(s'). The candidate (a, o) is live
//      iff n > 0 and n is finite; its successor is b'(s') = fl(u(s') / n): pd_filter_step's not-ended branch, so a
//      live successor is the filter's belief bit for bit. Successors through an episode end are no candidates (they
//      are the reset beliefs, which depend on no point).
//   3. dist(a, o) = min over q of L1(b', q),  L1 = sum_s |fl(b'[s] - q[s])|, s ascending from +0. All values are
//      finite and >= 0, so the minimum is exact whatever its order.
//   4. (a*, o*) = the first live candidate of the largest dist, a ascending, then o ascending.
// Outputs per point: succ = b' of (a*, o*), dist, act = a*, obs = o*, mass = n(a*, o*). A point without a live
// candidate: act = obs = -1, dist = mass = +0, a row of +0.
//
// Zero skipping. u >= 0 and the accumulator starts at +0, so n over the backup's (a, o) list (the non-terminal s' with
// Zf != 0, ascending) has the bits of the dense loop, and b'(s') is +0 off the list (for points whose acc is finite,
// as in §6s). The L1 sums are dense. The oracle is dense throughout.
//
// Kernels. No sum is split: the parallelism is across (p, a, s'), (p, a, o) and q; only the min and the argmax are
// reduced.
//   pb_acc   (pomdp_backup.hip, unchanged) step 1 into the backup's scratch acc [P][A][S]
//   px_mass  one thread per (p, a, o): n over the (a, o) list into scratch n [P][A][O]; an empty list answers +0
//   px_tr    the reference set into scratch [S][Q]: the 64 lanes of a wave then read 64 consecutive q per s
//   px_far   one workgroup per (p, a): for each live o ascending, b' into dynamic LDS [S]; each thread runs the
//            sequential L1 sums of four q at a time (each its own ascending sum; b'[s] is an LDS broadcast),
//            grid-stride over Q; a workgroup min (wave shuffles, then LDS); thread 0 keeps the first maximiser over o
//            into scratch best [P][A] = (dist, o)
//   px_best  one wave per p: the first maximiser over a, then b' of (a*, o*) again by the same operations on the same
//            operands (the same bits), the row and the scalars
// Every index read from a table is in bounds by the host's construction (s' < S); o* < O and a* < A by px_far.
#include <algorithm>
#include <cstdio>

#include "pomdp_expand.h"

#pragma clang fp contract(off)

namespace {

constexpr int TPB = 256;
constexpr int QPT = 4;  // reference rows per thread and pass of px_far

struct PxDev {
  int32_t S, A, O, P, Q;
  const uint32_t* zcptr;  // [A O + 1]
  const uint2* zcent;     // (s', bits of Zf[a][s'][o])
  const float* ref;       // [Q][S]
  const float* acc;       // [P][A][S]
  float* nn;              // [P][A][O]
  float2* best;           // [P][A]
  float* qt;              // [S][Q]
};

__device__ __forceinline__ bool px_live(float n) { return n > 0.f && n <= 3.402823466e38f; }

__global__ __launch_bounds__(TPB) void px_mass(PxDev d) {
  // (P A O <= 2^28 and P A S <= 2^28 by the scratch limit: 32 bits hold the flat index)
  const uint32_t S = (uint32_t)d.S, O = (uint32_t)d.O, AO = (uint32_t)d.A * O;
  const uint32_t i = blockIdx.x * TPB + threadIdx.x;
  if (i >= (uint32_t)d.P * AO) return;
  const uint32_t lst = i % AO;                    // a O + o
  const float* ac = d.acc + (size_t)(i / O) * S;  // acc of (p, a)
  float n = 0.f;
  for (uint32_t e = d.zcptr[lst], e1 = d.zcptr[lst + 1]; e < e1; ++e) {
    const uint2 q = d.zcent[e];
    n = n + __builtin_bit_cast(float, q.y) * ac[q.x];
  }
  d.nn[i] = n;
}

__global__ __launch_bounds__(TPB) void px_tr(PxDev d) {
  // (4 S Q <= 2^30: 32 bits hold the flat index) one thread per entry of the output: the stores are coalesced
  const uint32_t S = (uint32_t)d.S, Q = (uint32_t)d.Q;
  const uint32_t i = blockIdx.x * TPB + threadIdx.x;
  if (i >= S * Q) return;
  const uint32_t s = i / Q, q = i % Q;
  d.qt[i] = d.ref[(size_t)q * S + s];
}

// b' of the candidate (a, o) of one point into LDS bp[S], by every thread of the block: +0 everywhere, then the
// entries of the (a, o) list. Ends with a barrier.
__device__ __forceinline__ void px_successor(const PxDev& d, const float* ac, uint32_t lst, float n, float* bp) {
  const uint32_t S = (uint32_t)d.S;
  for (uint32_t s = threadIdx.x; s < S; s += blockDim.x) bp[s] = 0.f;
  __syncthreads();
  for (uint32_t e = d.zcptr[lst] + threadIdx.x, e1 = d.zcptr[lst + 1]; e < e1; e += blockDim.x) {
    const uint2 q = d.zcent[e];
    const float u = __builtin_bit_cast(float, q.y) * ac[q.x];
    bp[q.x] = u / n;
  }
  __syncthreads();
}

__global__ __launch_bounds__(TPB) void px_far(PxDev d) {
  extern __shared__ __attribute__((aligned(16))) float bp[];  // [S]
  __shared__ float wmin[TPB / 64];
  const uint32_t S = (uint32_t)d.S, O = (uint32_t)d.O, Q = (uint32_t)d.Q;
  const size_t pa = blockIdx.x;  // p A + a
  const uint32_t a = (uint32_t)(pa % (uint32_t)d.A);
  const float* ac = d.acc + pa * S;
  const float* nn = d.nn + pa * O;
  float dbest = 0.f;
  int obest = -1;
  for (uint32_t o = 0; o < O; ++o) {
    const float n = nn[o];  // (the same for every thread: the branch is uniform)
    if (!px_live(n)) continue;
    px_successor(d, ac, a * O + o, n, bp);
    float m = 3.402823466e38f;  // (every distance is finite: at most this)
    for (uint32_t q0 = threadIdx.x; q0 < Q; q0 += TPB * QPT) {
      float l[QPT];
      const float* col[QPT];
#pragma unroll
      for (int k = 0; k < QPT; ++k) {
        l[k] = 0.f;
        // (a lane past the end reads column Q - 1 again: in bounds, and the minimum is unchanged)
        col[k] = d.qt + min(q0 + (uint32_t)k * TPB, Q - 1);
      }
      for (uint32_t s = 0; s < S; ++s) {
        const float b = bp[s];
#pragma unroll
        for (int k = 0; k < QPT; ++k) l[k] = l[k] + fabsf(b - col[k][(size_t)s * Q]);
      }
#pragma unroll
      for (int k = 0; k < QPT; ++k) m = l[k] < m ? l[k] : m;
    }
#pragma unroll
    for (int w = 32; w >= 1; w >>= 1) {
      const float t = __shfl_xor(m, w, 64);
      m = t < m ? t : m;
    }
    if ((threadIdx.x & 63) == 0) wmin[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
      for (int w = 1; w < TPB / 64; ++w) m = wmin[w] < m ? wmin[w] : m;
      if (obest < 0 || m > dbest) {
        dbest = m;
        obest = (int)o;
      }
    }
    // (the next pass clears bp at once: safe behind the barrier above, which every thread reaches after its L1 sums.
    // wmin is rewritten only behind px_successor's two barriers, which thread 0 reaches after reading it here)
  }
  if (threadIdx.x == 0) d.best[pa] = make_float2(dbest, __builtin_bit_cast(float, obest));
}

__global__ __launch_bounds__(64) void px_best(PxDev d, float* __restrict__ succ_out, float* __restrict__ dist_out,
                                              int32_t* __restrict__ act_out, int32_t* __restrict__ obs_out,
                                              float* __restrict__ mass_out) {
  extern __shared__ __attribute__((aligned(16))) float bp[];  // [S]
  const uint32_t S = (uint32_t)d.S, A = (uint32_t)d.A, O = (uint32_t)d.O;
  const size_t p = blockIdx.x;
  int abest = -1, obest = -1;
  float dbest = 0.f;
  for (uint32_t a = 0; a < A; ++a) {  // (uniform: every lane walks the same A entries)
    const float2 c = d.best[p * A + a];
    const int o = __builtin_bit_cast(int, c.y);
    if (o >= 0 && (abest < 0 || c.x > dbest)) {
      dbest = c.x;
      abest = (int)a;
      obest = o;
    }
  }
  float n = 0.f;
  if (abest >= 0) {
    const size_t pa = p * A + (uint32_t)abest;
    n = d.nn[pa * O + (uint32_t)obest];
    if (succ_out) px_successor(d, d.acc + pa * S, (uint32_t)abest * O + (uint32_t)obest, n, bp);
  } else if (succ_out) {
    for (uint32_t s = threadIdx.x; s < S; s += 64) bp[s] = 0.f;
    __syncthreads();
  }
  if (succ_out)
    for (uint32_t s = threadIdx.x; s < S; s += 64) succ_out[p * S + s] = bp[s];
  if (threadIdx.x == 0) {
    if (dist_out) dist_out[p] = dbest;
    if (act_out) act_out[p] = abest;
    if (obs_out) obs_out[p] = obest;
    if (mass_out) mass_out[p] = n;
  }
}

}  // namespace

void PxHost::release() {
  for (DevBuf* b : {&b_n, &b_best, &b_qt}) (void)b->alloc(0);
}

// Validates, grows the scratch if this call needs more, and launches the five kernels on `s`. Nothing is copied and
// nothing is waited for unless a buffer grows (a buffer is freed only once the device is idle).
int PxHost::expand(PbHost& pb, const PbModel& m, int P, const float* points, int Q, const float* ref, float* succ_out,
                   float* dist_out, int32_t* act_out, int32_t* obs_out, float* mass_out, hipStream_t s) {
  const int S = m.S, A = m.A, O = m.O;
  if (P < 0 || P > PX_MAX_POINTS) {
    gp_set_error("gp_belief_expand: %d points outside [0, %d]", P, PX_MAX_POINTS);
    return GP_E_INVALID;
  }
  if (ref && (Q < 1 || Q > PX_MAX_POINTS)) {
    gp_set_error("gp_belief_expand: %d reference rows outside [1, %d]", Q, PX_MAX_POINTS);
    return GP_E_INVALID;
  }
  if (!ref) Q = P;
  const size_t need_acc = (size_t)P * A * S * sizeof(float), need_n = (size_t)P * A * O * sizeof(float),
               need_best = (size_t)P * A * sizeof(float2), need_qt = (size_t)S * Q * sizeof(float);
  if (need_acc + need_n + need_best + need_qt > PX_MAX_SCRATCH) {
    gp_set_error("gp_belief_expand: %d points and %d reference rows need %zu bytes of scratch (4 P A S + 4 P A O + "
                 "8 P A + 4 S Q), at most 2^30", P, Q, need_acc + need_n + need_best + need_qt);
    return GP_E_INVALID;
  }
  if (P == 0) return GP_OK;
  if (!points) {
    gp_set_error("gp_belief_expand: points are required");
    return GP_E_INVALID;
  }
  int e;
  if (b_n.n < need_n || b_best.n < need_best || b_qt.n < need_qt) {
    // (earlier calls queued on any stream may still use the buffers: freed only once the device is idle, and the new
    // ones are cleared before anything is queued behind)
    GP_HIP_CHECK(hipDeviceSynchronize());
    if (b_n.n < need_n && (e = b_n.alloc(need_n))) return e;
    if (b_best.n < need_best && (e = b_best.alloc(need_best))) return e;
    if (b_qt.n < need_qt && (e = b_qt.alloc(need_qt))) return e;
    GP_HIP_CHECK(hipDeviceSynchronize());
  }
  if ((e = pb.acc_points(m, P, points, s))) return e;
  PxDev d{};
  d.S = S;
  d.A = A;
  d.O = O;
  d.P = P;
  d.Q = Q;
  d.zcptr = pb.b_zcptr.as<uint32_t>();
  d.zcent = pb.b_zcent.as<uint2>();
  d.ref = ref ? ref : points;
  d.acc = pb.b_acc.as<float>();
  d.nn = b_n.as<float>();
  d.best = b_best.as<float2>();
  d.qt = b_qt.as<float>();
  // (P A S, P A O and S Q <= 2^28 by the scratch limit: the block counts fit 32 bits)
  const unsigned pa = (unsigned)P * (unsigned)A;
  const size_t lds = (size_t)S * sizeof(float);  // S <= 4,096 (the filter's limit): at most 16 KB
  hipLaunchKernelGGL(px_mass, dim3((unsigned)(((size_t)pa * O + TPB - 1) / TPB)), dim3(TPB), 0, s, d);
  hipLaunchKernelGGL(px_tr, dim3((unsigned)(((size_t)S * Q + TPB - 1) / TPB)), dim3(TPB), 0, s, d);
  hipLaunchKernelGGL(px_far, dim3(pa), dim3(TPB), lds, s, d);
  hipLaunchKernelGGL(px_best, dim3((unsigned)P), dim3(64), lds, s, d, succ_out, dist_out, act_out, obs_out, mass_out);
  GP_HIP_CHECK(hipGetLastError());
  return GP_OK;
}
