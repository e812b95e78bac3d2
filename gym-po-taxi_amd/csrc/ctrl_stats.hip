// ctrl_stats.hip — gp_controller_stats (semantics in include/gym_po_amd.h): the sufficient statistics
// of K stored closed-loop steps per controller table cell (node, obs, action, next node): how often the choice was
// made, and the sum of the discounted returns that followed it, as exact integers. One launch: a backward scan per env
// over the planes gp_rollout_controller wrote (the float32 return-to-go recursion, two roundings per step) feeding a
// histogram. The call reads nothing of the env but the shape of the installed controller, so it is the same for all
// six kinds with closed-loop rollouts.
//
// Integers only in the accumulation: counts += 1 and ret_q += rint(G * 2^20) as int64. Integer sums do not depend on
// the order of the adds (two's-complement wrap-around included), so the result is bit-reproducible and the two paths
// below give identical bits, whatever the launch geometry. No float or double atomics.
//   LDS path     one controller's tables (8 B sum + 4 B count per cell) fit the budget: each block keeps a private
//                histogram in dynamic LDS, updated with LDS integer atomics, and at its end adds the non-zero cells to
//                the global tables with 64-bit integer atomics. The 32-bit LDS counts bound a block's visits to
//                below 2^32: launches of K >= 2^22 steps take the global path.
//   global path  64-bit integer atomics straight to the global tables.
// Geometry (that of the rollouts that wrote the planes): one block per 1,024-env tile, 256 threads, 4 consecutive envs
// per thread, so that a block serves exactly one controller of a population (groups are multiples of 1,024 envs);
// 16-B / 4-B quad accesses with an element-wise fallback for the ragged tail and for rows off their boundary; the rows
// of step k - 1 are loaded while step k is processed.
#include <algorithm>

#include "gp_internal.h"

// G_k = rew + gamma * G_{k+1} rounds twice, as the numpy restatement does: nothing here contracts into an FMA. Plain
// operators under this pragma (the __fmul_rn forms are ordinary operators in a runtime header and fuse after inlining).
#pragma clang fp contract(off)

namespace {

constexpr int TPB = 256;
constexpr int EPT = 4;
constexpr int EPB = TPB * EPT;
// Default LDS budget of the histogram: 40 KiB per block (3,413 cells: a memoryless FourRooms Hansen-4 policy, 405 obs x
// 4 actions x 2 columns = 3,240 cells = 38 KiB, still fits) leaves 4 blocks = 16 waves per CU of the 160 KiB; the knob
// stats_lds_max raises it to at most 60 KB (2 blocks per CU), the most a launch holds without opting in.
constexpr int STATS_LDS_BUDGET = 40 * 1024;
constexpr int STATS_LDS_CAP = 60 * 1024;
constexpr int CELL_LDS_BYTES = 12;  // one 64-bit fixed-point sum and one 32-bit count

struct StDev {
  int32_t B, K, M, n_obs, A, P;
  int64_t G;              // envs per group of a population (P > 1)
  unsigned long long T;   // cells of one controller: M * n_obs * A * (M + 1)
  const int32_t *obs0, *obs, *act;
  const uint8_t *nodes, *next_nodes;
  const float* rew;
  const uint8_t *term, *trunc;
  const float* boot;      // may be null: 0
  float gamma;
  unsigned long long *counts, *ret_q;  // int64 tables, added into as two's-complement words
  uint32_t* derr;
};

// The planes' values of one step for a thread's 4 envs. o: the obs the choice was conditioned on (obs0 for step 0,
// else the obs after step k - 1).
struct Row {
  int32_t o[EPT], a[EPT];
  float r[EPT];
  uint8_t n[EPT], tm[EPT], tr[EPT];
};
__device__ __forceinline__ void load_row(const StDev& p, int k, int env0, Row& w) {
  const size_t off = (size_t)k * (size_t)p.B;
  load4<int32_t>(k ? p.obs + (off - (size_t)p.B) : p.obs0, env0, p.B, w.o);
  load4<int32_t>(p.act + off, env0, p.B, w.a);
  load4<float>(p.rew + off, env0, p.B, w.r);
  load4<uint8_t>(p.nodes + off, env0, p.B, w.n);
  load4<uint8_t>(p.term + off, env0, p.B, w.tm);
  load4<uint8_t>(p.trunc + off, env0, p.B, w.tr);
}

template <bool LDS>
__global__ __launch_bounds__(TPB) void ctrl_stats(StDev p) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  unsigned long long* hq = reinterpret_cast<unsigned long long*>(lds);  // [T] sums, then [T] counts
  uint32_t* hc = reinterpret_cast<uint32_t*>(lds + 8 * (size_t)p.T);
  if constexpr (LDS) {
    const uint32_t words = 3u * (uint32_t)p.T;
    for (uint32_t i = threadIdx.x; i < words; i += TPB) reinterpret_cast<uint32_t*>(lds)[i] = 0u;
    __syncthreads();
  }
  const int tile = blockIdx.x, env0 = tile * EPB + threadIdx.x * EPT;
  // the block's controller: groups are multiples of EPB envs, so a tile never straddles two
  const size_t base = p.P > 1 ? (size_t)(((int64_t)tile * EPB) / p.G) * (size_t)p.T : 0;
  const uint32_t M = (uint32_t)p.M, n_obs = (uint32_t)p.n_obs, A = (uint32_t)p.A;
  const float gamma = p.gamma;
  uint8_t nn[EPT];  // the node after the step in hand: next_nodes, then the nodes plane of the step after it
  load4<uint8_t>(p.next_nodes, env0, p.B, nn);
  float g[EPT] = {0.f, 0.f, 0.f, 0.f};
  if (p.boot) load4<float>(p.boot, env0, p.B, g);
  Row cur;
  load_row(p, p.K - 1, env0, cur);
  for (int k = p.K - 1; k >= 0; --k) {
    Row nxt = cur;
    if (k > 0) load_row(p, k - 1, env0, nxt);  // one step ahead of the scan
#pragma unroll
    for (int i = 0; i < EPT; ++i) {
      const bool ended = (cur.tm[i] | cur.tr[i]) != 0;
      g[i] = ended ? cur.r[i] : cur.r[i] + gamma * g[i];  // two roundings (no contraction in this file)
      const uint32_t n = cur.n[i], o = (uint32_t)cur.o[i], a = (uint32_t)cur.a[i];
      const bool ok = n < M && o < n_obs && a < A && (ended || nn[i] < M) && fabsf(g[i]) < 0x1p31f;  // (NaN: false)
      if (env0 + i < p.B) {
        if (ok) {
          const uint32_t nx = ended ? M : (uint32_t)nn[i];  // column M: the choice ended the episode
          const unsigned long long q = (unsigned long long)__float2ll_rn(g[i] * 0x1p20f);  // exact scaling, one rint
          if constexpr (LDS) {
            const uint32_t c = ((n * n_obs + o) * A + a) * (M + 1u) + nx;  // < T, which fits the LDS
            atomicAdd(&hc[c], 1u);
            atomicAdd(&hq[c], q);
          } else {
            const size_t c = base + (((size_t)n * n_obs + o) * A + a) * (size_t)(M + 1u) + nx;
            atomicAdd(&p.counts[c], 1ull);
            atomicAdd(&p.ret_q[c], q);
          }
        } else {
          atomicOr(p.derr, GP_DERR_STATS);  // skipped, never clamped into another cell; the G chain goes on
        }
      }
      nn[i] = cur.n[i];
    }
    cur = nxt;
  }
  if constexpr (LDS) {
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < (uint32_t)p.T; i += TPB) {
      const uint32_t c = hc[i];
      if (c) {  // (a cell without visits has no sum either)
        atomicAdd(&p.counts[base + i], (unsigned long long)c);
        const unsigned long long q = hq[i];
        if (q) atomicAdd(&p.ret_q[base + i], q);
      }
    }
  }
}

}  // namespace

int ctrl_stats_launch(const CtrlShape& c, int64_t B, int K, const int32_t* obs0, const int32_t* obs,
                      const int32_t* actions, const uint8_t* nodes, const uint8_t* next_nodes, const float* rew,
                      const uint8_t* term, const uint8_t* trunc, const float* bootstrap, float gamma, int64_t* counts,
                      int64_t* ret_q, int* lds_path, hipStream_t s) {
  StDev p{};
  p.B = (int32_t)B;
  p.K = K;
  p.M = c.M;
  p.n_obs = c.n_obs;
  p.A = c.A;
  p.P = c.P;
  p.G = c.G;
  p.T = (unsigned long long)c.M * (unsigned long long)c.n_obs * (unsigned long long)c.A * (unsigned long long)(c.M + 1);
  p.obs0 = obs0;
  p.obs = obs;
  p.act = actions;
  p.nodes = nodes;
  p.next_nodes = next_nodes;
  p.rew = rew;
  p.term = term;
  p.trunc = trunc;
  p.boot = bootstrap;
  p.gamma = gamma;
  p.counts = reinterpret_cast<unsigned long long*>(counts);
  p.ret_q = reinterpret_cast<unsigned long long*>(ret_q);
  p.derr = c.derr;
  const int knob = gp_debug_knobs().stats_lds_max;
  const unsigned long long budget = knob >= 0 ? (unsigned long long)std::min(knob, STATS_LDS_CAP) : STATS_LDS_BUDGET;
  const bool lds = p.T * CELL_LDS_BYTES <= budget && K < (1 << 22);
  const unsigned ntiles = (unsigned)((B + EPB - 1) / EPB);
  if (lds)
    hipLaunchKernelGGL(ctrl_stats<true>, dim3(ntiles), dim3(TPB), (size_t)(p.T * CELL_LDS_BYTES), s, p);
  else
    hipLaunchKernelGGL(ctrl_stats<false>, dim3(ntiles), dim3(TPB), 0, s, p);
  GP_HIP_CHECK(hipGetLastError());
  *lds_path = lds ? 1 : 0;
  return GP_OK;
}
