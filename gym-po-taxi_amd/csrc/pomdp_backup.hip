// pomdp_backup.hip — the point-based value backup of the tabular POMDP (gp_belief_backup): from belief
// points b[P][S] and a set of alpha-vectors alpha[N][S], one new vector, its action and its value per point (Pineau,
// Gordon & Thrun 2003). Build-defined; pinned bit for bit to tests/pbvi_oracle.py.
//
// Rule. The float laws and the arithmetic are the belief filter's (pomdp.hip): Tf, Zf from the handle's integer
// thresholds, p[i] = (float)(uint32)(thr[i] - thr[i-1]) * 2^-31; reward[s][a][s'] and terminal[s'] from the model blob;
// float32, every product and every sum rounded on its own (contraction is off in this file: no FMA), sums sequential
// in ascending index from +0, the first maximiser wins (replaced only on a strict >). For a point b, the set alpha and
// float32 gamma, for every action a:
//   1. acc_a(s') = sum_s fl(b[s] Tf[s][a][s'])                                     (pd_filter_step's acc)
//   2. for every obs o: u(s') = terminal[s'] ? +0 : fl(Zf[a][s'][o] acc_a(s'));  score_j = sum_s' fl(u(s') alpha[j][s']);
//      j*(a, o) = the first maximiser over j
//   3. w_a(s') = terminal[s'] ? +0 : sum_o fl(Zf[a][s'][o] alpha[j*(a, o)][s']),  o ascending
//   4. for every s: r_a(s) = sum_s' fl(Tf[s][a][s'] reward[s][a][s']);  h_a(s) = sum_s' fl(Tf[s][a][s'] w_a(s'));
//      beta_a(s) = fl(r_a(s) + fl(gamma h_a(s)))
//   5. v_a = sum_s fl(b[s] beta_a(s));  a* = the first maximiser over a
// Outputs per point: beta_a*, a*, v_a*. A terminal s' is absorbing with value 0 (qmdp_vectors' convention, the filter's
// "a step that did not end" rule); the time limit is not part of the value.
//
// Zero skipping. With finite points, alpha and reward, a term with Tf == 0 or Zf == 0 is +-0, and so is every term of
// step 2 at a terminal s'. An accumulator that starts at +0 is never -0 (x + -0 = x, and an exact zero sum rounds to
// +0), so leaving those terms out gives the bits of the dense loop. Steps 1 and 4 walk compressed columns and rows of
// Tf, steps 2 and 3 compressed lists of Zf by (a, o) and by (a, s'); step 5 is dense. The oracle is dense throughout.
//
// Kernels. No sum is split: the parallelism is across (p, a, s'), (p, a, o) and (p, a, s).
//   pb_acc   one thread per (p, a, s'): step 1 into scratch acc [P][A][S]
//   pb_pick  one thread per (p, a, o): step 2, four vectors per pass over the obs list (each score still its own
//            ascending sum), j* into scratch [P][A][O] (uint16: N <= 4,096)
//   pb_beta  one workgroup per (p, a): step 3 into LDS w[S], then step 4; beta_a overwrites acc_a (dead by then)
//   pb_best  one wave per p: lane a sums v_a (step 5), then all lanes copy beta_a*
// Every index read from a table is in bounds by the host's construction (s, s' < S, o < O); j* < N by pb_pick.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "pomdp_backup.h"

#pragma clang fp contract(off)

namespace {

constexpr int TPB = 256;
constexpr int MAX_VECTORS = 4096;  // the policy's limits (pomdp.hip)
constexpr size_t MAX_ALPHA = (size_t)1 << 22;

struct PbDev {
  int32_t S, A, O, N, P;
  const uint32_t *colptr, *rowptr, *zcptr, *zrptr;
  const uint2 *ent, *rent, *zcent, *zrent;
  const float* reward;  // [S][A][S]
  const float* alpha;   // [N][S]
  const float* points;  // [P][S]
  float* acc;           // [P][A][S]
  uint16_t* jst;        // [P][A][O]
};

__global__ __launch_bounds__(TPB) void pb_acc(PbDev d) {
  // (P A S <= 2^28 and P A O <= 2^29 by the scratch limit: 32 bits hold the flat indices of pb_acc and pb_pick)
  const uint32_t S = (uint32_t)d.S, AS = (uint32_t)d.A * S;
  const uint32_t i = blockIdx.x * TPB + threadIdx.x;
  if (i >= (uint32_t)d.P * AS) return;
  const uint32_t col = i % AS;  // a S + s'
  const float* b = d.points + (size_t)(i / AS) * S;
  float acc = 0.f;
  for (uint32_t e = d.colptr[col], e1 = d.colptr[col + 1]; e < e1; ++e) {
    const uint2 q = d.ent[e];
    acc = acc + b[q.x] * __builtin_bit_cast(float, q.y);
  }
  d.acc[i] = acc;
}

__global__ __launch_bounds__(TPB) void pb_pick(PbDev d) {
  const uint32_t S = (uint32_t)d.S, O = (uint32_t)d.O, AO = (uint32_t)d.A * O;
  const uint32_t i = blockIdx.x * TPB + threadIdx.x;
  if (i >= (uint32_t)d.P * AO) return;
  const uint32_t lst = i % AO;                    // a O + o
  const float* ac = d.acc + (size_t)(i / O) * S;  // acc of (p, a)
  const uint32_t e0 = d.zcptr[lst], e1 = d.zcptr[lst + 1];
  int jbest = 0;
  float vbest = 0.f;
  // (an empty list: every score is +0 and vector 0 is the first maximiser)
  for (int j0 = 0; e0 < e1 && j0 < d.N; j0 += 4) {
    const int nj = min(4, d.N - j0);
    const float* al = d.alpha + (size_t)j0 * S;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    for (uint32_t e = e0; e < e1; ++e) {
      const uint2 q = d.zcent[e];
      const float u = __builtin_bit_cast(float, q.y) * ac[q.x];
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < nj) v[k] = v[k] + u * al[(size_t)k * S + q.x];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < nj && (j0 + k == 0 || v[k] > vbest)) {
        vbest = v[k];
        jbest = j0 + k;
      }
  }
  d.jst[i] = (uint16_t)jbest;
}

__global__ __launch_bounds__(TPB) void pb_beta(PbDev d, float gamma) {
  extern __shared__ __attribute__((aligned(16))) float w[];  // [S]
  const uint32_t S = (uint32_t)d.S, A = (uint32_t)d.A;
  const size_t pa = blockIdx.x;  // p A + a
  const uint32_t a = (uint32_t)(pa % A);
  const uint16_t* js = d.jst + pa * (size_t)d.O;
  for (uint32_t s1 = threadIdx.x; s1 < S; s1 += blockDim.x) {
    float acc = 0.f;  // (a terminal s' has an empty list: +0)
    for (uint32_t e = d.zrptr[a * S + s1], e1 = d.zrptr[a * S + s1 + 1]; e < e1; ++e) {
      const uint2 q = d.zrent[e];
      acc = acc + __builtin_bit_cast(float, q.y) * d.alpha[(size_t)js[q.x] * S + s1];
    }
    w[s1] = acc;
  }
  __syncthreads();
  float* beta = d.acc + pa * S;
  for (uint32_t s = threadIdx.x; s < S; s += blockDim.x) {
    const uint32_t row = s * A + a;
    const float* rw = d.reward + (size_t)row * S;
    float r = 0.f, h = 0.f;
    for (uint32_t e = d.rowptr[row], e1 = d.rowptr[row + 1]; e < e1; ++e) {
      const uint2 q = d.rent[e];
      const float t = __builtin_bit_cast(float, q.y);
      r = r + t * rw[q.x];
      h = h + t * w[q.x];
    }
    beta[s] = r + gamma * h;
  }
}

__global__ __launch_bounds__(64) void pb_best(PbDev d, float* __restrict__ alpha_out, int32_t* __restrict__ act_out,
                                              float* __restrict__ value_out) {
  __shared__ float va[64];  // A <= 64
  const int S = d.S, A = d.A;
  const size_t p = blockIdx.x;
  const float* b = d.points + p * S;
  if ((int)threadIdx.x < A) {
    const float* beta = d.acc + (p * A + threadIdx.x) * S;
    float v = 0.f;
    for (int s = 0; s < S; ++s) v = v + b[s] * beta[s];
    va[threadIdx.x] = v;
  }
  __syncthreads();
  int abest = 0;
  float vbest = va[0];
  for (int a = 1; a < A; ++a)
    if (va[a] > vbest) {
      vbest = va[a];
      abest = a;
    }
  if (alpha_out) {
    const float* beta = d.acc + (p * A + abest) * S;
    for (int s = threadIdx.x; s < S; s += 64) alpha_out[p * S + s] = beta[s];
  }
  if (threadIdx.x == 0) {
    if (act_out) act_out[p] = abest;
    if (value_out) value_out[p] = vbest;
  }
}

}  // namespace

void PbHost::release() {
  for (DevBuf* b : {&b_rowptr, &b_rent, &b_zcptr, &b_zcent, &b_zrptr, &b_zrent, &b_alpha, &b_acc, &b_jst})
    (void)b->alloc(0);
  built = false;
}

// The three compressed tables, from the thresholds the handle was built with (read back from the device, as
// gp_belief_enable does). Built and uploaded into buffers of their own first: a failure installs nothing.
int PbHost::build(const PbModel& m) {
  const int S = m.S, A = m.A, O = m.O, Sp = m.Sp, Op = m.Op;
  GP_HIP_CHECK(hipDeviceSynchronize());
  std::vector<uint32_t> tt((size_t)S * A * Sp), zt((size_t)A * S * Op), tw(((size_t)S + 15) / 16 * 4);
  GP_HIP_CHECK(hipMemcpy(tt.data(), m.blob, tt.size() * 4, hipMemcpyDeviceToHost));
  GP_HIP_CHECK(hipMemcpy(zt.data(), m.blob + m.off_obs, zt.size() * 4, hipMemcpyDeviceToHost));
  GP_HIP_CHECK(hipMemcpy(tw.data(), m.blob + m.off_term, tw.size() * 4, hipMemcpyDeviceToHost));
  const uint8_t* term = reinterpret_cast<const uint8_t*>(tw.data());
  auto diff = [](const uint32_t* row, int i) { return (uint32_t)(row[i] - (i ? row[i - 1] : 0u)); };
  auto law = [](uint32_t d) { return __builtin_bit_cast(uint32_t, (float)d * 0x1p-31f); };
  // rows (s, a) of Tf
  std::vector<uint32_t> rp((size_t)S * A + 1, 0);
  std::vector<uint2> re;
  for (size_t r = 0; r < (size_t)S * A; ++r) {
    const uint32_t* row = tt.data() + r * Sp;
    for (int s1 = 0; s1 < S; ++s1)
      if (const uint32_t d = diff(row, s1)) re.push_back(make_uint2((uint32_t)s1, law(d)));
    rp[r + 1] = (uint32_t)re.size();
  }
  // Zf by (a, s') over o, and by (a, o) over s'; terminal s' left out of both
  std::vector<uint32_t> zrp((size_t)A * S + 1, 0), zcp((size_t)A * O + 1, 0);
  std::vector<uint2> zre;
  for (int a = 0; a < A; ++a)
    for (int s1 = 0; s1 < S; ++s1) {
      const uint32_t* row = zt.data() + ((size_t)a * S + s1) * Op;
      if (!term[s1])
        for (int o = 0; o < O; ++o)
          if (const uint32_t d = diff(row, o)) {
            zre.push_back(make_uint2((uint32_t)o, law(d)));
            ++zcp[(size_t)a * O + o + 1];
          }
      zrp[(size_t)a * S + s1 + 1] = (uint32_t)zre.size();
    }
  for (size_t c = 0; c < (size_t)A * O; ++c) zcp[c + 1] += zcp[c];
  std::vector<uint2> zce(zre.size());
  std::vector<uint32_t> fill(zcp.begin(), zcp.end() - 1);
  for (int a = 0; a < A; ++a)
    for (int s1 = 0; s1 < S; ++s1)  // s' ascending within every list
      for (uint32_t e = zrp[(size_t)a * S + s1], e1 = zrp[(size_t)a * S + s1 + 1]; e < e1; ++e)
        zce[fill[(size_t)a * O + zre[e].x]++] = make_uint2((uint32_t)s1, zre[e].y);
  DevBuf n[6];
  int e;
  if ((e = n[0].upload(rp)) || (e = n[1].upload(re)) || (e = n[2].upload(zcp)) || (e = n[3].upload(zce)) ||
      (e = n[4].upload(zrp)) || (e = n[5].upload(zre)))
    return e;
  DevBuf* dst[6] = {&b_rowptr, &b_rent, &b_zcptr, &b_zcent, &b_zrptr, &b_zrent};
  for (int i = 0; i < 6; ++i) {
    std::swap(dst[i]->p, n[i].p);
    std::swap(dst[i]->n, n[i].n);
  }
  built = true;
  return GP_OK;
}

// The caller has validated P (>= 1) and the scratch size.
int PbHost::acc_points(const PbModel& m, int P, const float* points, hipStream_t s) {
  int e;
  if (!built && (e = build(m))) return e;
  const size_t need_acc = (size_t)P * m.A * m.S * sizeof(float);
  if (b_acc.n < need_acc) {  // (an earlier call queued on any stream may still use it: freed once the device is idle)
    GP_HIP_CHECK(hipDeviceSynchronize());
    if ((e = b_acc.alloc(need_acc))) return e;
    GP_HIP_CHECK(hipDeviceSynchronize());
  }
  PbDev d{};
  d.S = m.S;
  d.A = m.A;
  d.O = m.O;
  d.P = P;
  d.colptr = m.colptr;
  d.ent = m.ent;
  d.points = points;
  d.acc = b_acc.as<float>();
  hipLaunchKernelGGL(pb_acc, dim3((unsigned)(((size_t)P * m.A * m.S + TPB - 1) / TPB)), dim3(TPB), 0, s, d);
  GP_HIP_CHECK(hipGetLastError());
  return GP_OK;
}

// Validates, copies the vectors to the device (after the stream's earlier work: an earlier call may still read the
// handle's copy), grows the scratch if this call needs more, and launches the four kernels on `s`.
int PbHost::backup(const PbModel& m, int P, const float* points, int N, const float* alpha, float gamma,
                   float* alpha_out, int32_t* act_out, float* value_out, hipStream_t s) {
  const int S = m.S, A = m.A, O = m.O;
  if (N < 1 || N > MAX_VECTORS || (size_t)N * S > MAX_ALPHA) {
    gp_set_error("gp_belief_backup: %d vectors over %d states (%zu entries): from 1 to %d vectors and at most 2^22 entries",
                 N, S, (size_t)(N < 0 ? 0 : N) * S, MAX_VECTORS);
    return GP_E_INVALID;
  }
  if (!(gamma >= 0.0f && gamma <= 1.0f)) {
    gp_set_error("gp_belief_backup: gamma must be in [0, 1] (got %g)", (double)gamma);
    return GP_E_INVALID;
  }
  if (P < 0 || P > PB_MAX_POINTS) {
    gp_set_error("gp_belief_backup: %d points outside [0, %d]", P, PB_MAX_POINTS);
    return GP_E_INVALID;
  }
  if (!alpha || (P > 0 && !points)) {
    gp_set_error("gp_belief_backup: points and alpha are required");
    return GP_E_INVALID;
  }
  for (size_t i = 0; i < (size_t)N * S; ++i)
    if (!(alpha[i] >= -1e30f && alpha[i] <= 1e30f)) {
      gp_set_error("gp_belief_backup: alpha[%zu][%zu] = %g is not a finite value within +-1e30", i / S, i % S,
                   (double)alpha[i]);
      return GP_E_INVALID;
    }
  const size_t need_acc = (size_t)P * A * S * sizeof(float), need_jst = (size_t)P * A * O * sizeof(uint16_t);
  if (need_acc + need_jst > PB_MAX_SCRATCH) {
    gp_set_error("gp_belief_backup: %d points need %zu bytes of scratch (4 P A S + 2 P A O), at most 2^30", P,
                 need_acc + need_jst);
    return GP_E_INVALID;
  }
  if (P == 0) return GP_OK;
  int e;
  if (!built && (e = build(m))) return e;
  GP_HIP_CHECK(hipStreamSynchronize(s));
  if (b_alpha.n < (size_t)N * S * sizeof(float) && (e = b_alpha.alloc((size_t)N * S * sizeof(float)))) return e;
  GP_HIP_CHECK(hipMemcpy(b_alpha.p, alpha, (size_t)N * S * sizeof(float), hipMemcpyHostToDevice));
  if (b_acc.n < need_acc && (e = b_acc.alloc(need_acc))) return e;
  if (b_jst.n < need_jst && (e = b_jst.alloc(need_jst))) return e;
  PbDev d{};
  d.S = S;
  d.A = A;
  d.O = O;
  d.N = N;
  d.P = P;
  d.colptr = m.colptr;
  d.ent = m.ent;
  d.rowptr = b_rowptr.as<uint32_t>();
  d.rent = b_rent.as<uint2>();
  d.zcptr = b_zcptr.as<uint32_t>();
  d.zcent = b_zcent.as<uint2>();
  d.zrptr = b_zrptr.as<uint32_t>();
  d.zrent = b_zrent.as<uint2>();
  d.reward = reinterpret_cast<const float*>(m.blob + m.off_rew);
  d.alpha = b_alpha.as<float>();
  d.points = points;
  d.acc = b_acc.as<float>();
  d.jst = b_jst.as<uint16_t>();
  // (P A S <= 2^28 and P A O <= 2^29 by the scratch limit: the block counts fit 32 bits)
  const unsigned pa = (unsigned)P * (unsigned)A;
  hipLaunchKernelGGL(pb_acc, dim3((unsigned)(((size_t)pa * S + TPB - 1) / TPB)), dim3(TPB), 0, s, d);
  hipLaunchKernelGGL(pb_pick, dim3((unsigned)(((size_t)pa * O + TPB - 1) / TPB)), dim3(TPB), 0, s, d);
  hipLaunchKernelGGL(pb_beta, dim3(pa), dim3(S > 64 ? TPB : 64), (size_t)S * sizeof(float), s, d, gamma);
  hipLaunchKernelGGL(pb_best, dim3((unsigned)P), dim3(64), 0, s, d, alpha_out, act_out, value_out);
  GP_HIP_CHECK(hipGetLastError());
  return GP_OK;
}
