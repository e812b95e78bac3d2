// gp_ctrl.h — the tabular finite-state controller of the closed-loop rollouts (gp_set_controller; semantics in
// include/gym_po_amd.h), one copy for the kinds that run it (grid.hip with its populations, rocksample.hip, anttag.hip,
// taxi.hip, heavenhell.hip, crooms.hip, pomdp.hip, which also runs ctrl_search on its model's own rows). Per env-step one Philox block tagged CTRL_TAG picks j = action * M + next_node
// from the threshold row of (node, obs). Device side: the view of an installed table (CtrlDev), the node clamp
// (ctrl_clamp_node), the pick (ctrl_pick over ctrl_search) and the split of j (ctrl_action, ctrl_node). Host side: the
// validation of a table (ctrl_validate_rows) and the owner of an installed one (CtrlHost: install / clear, the LDS
// staging rule, the node plane, the rollout_controller precondition). What stays with a kind: which kernel's occupancy
// sizes its closed-loop grid, and the modes in which it refuses controllers.
#pragma once
#include "../../include/gym_po_amd.h"
#include <algorithm>

#include "gp_common.h"
#include "gp_internal.h"

// the env draws carry 0x67706f21 (grid) / 0x726f636b (rocksample) / 0x616e7431 (anttag) / 0x74617869 (taxi) /
// 0x6868656c (heavenhell) / 0x63726f6f and 0x6d733121 (crooms) / 0x706f6d64 (pomdp)
constexpr uint32_t CTRL_TAG = 0x67706f63u;
// Largest dynamic LDS per block (env tables + controller table) up to which the kinds that stage the table in LDS
// (grid.hip, taxi.hip, heavenhell.hip, crooms.hip, pomdp.hip) do so by default; the knob ctrl_lds_max overrides it, up
// to 60 KB (CtrlHost::stage). pomdp.hip's budget for its model blob (knob pomdp_lds_max) has the same default and cap.
constexpr int CTRL_LDS_BUDGET = 32 * 1024;
constexpr int CTRL_MAX_L = 64;  // A * M: j / M by the 16-bit magic multiply is exact for j < 64
struct CtrlDev {
  const uint32_t* thr;  // [M][n_obs][L]: nondecreasing rows, entries <= 2^31, last == 2^31 (validated on upload)
  uint8_t* node;        // [B] the controller node of each env
  int32_t M, n_obs, L;  // L: entries per stored row, a multiple of 4 (rows are 16-B aligned)
  uint32_t inv_m;       // ceil(2^16 / M): j / M == (j * inv_m) >> 16 for j < 64, M <= 8
  int32_t lds_off, bytes;  // lds_off >= 0: the table is staged at this offset of the dynamic LDS (CL launches); its size
};

__device__ __forceinline__ uint32_t ctrl_count4(const uint4 q, uint32_t y) {
  return (uint32_t)(y >= q.x) + (uint32_t)(y >= q.y) + (uint32_t)(y >= q.z) + (uint32_t)(y >= q.w);
}
// #{i < L : y >= row[i]} for a nondecreasing row whose last entry exceeds y (y < 2^31). Up to 16 entries: every
// 16-B quad is loaded (independent loads, one latency) and counted. Longer rows: a branch-free binary search over
// the quads' last entries for the first quad not entirely <= y (never past the last quad), then that quad's count.
__device__ __forceinline__ uint32_t ctrl_search(const uint32_t* __restrict__ row, int L, uint32_t y) {
  const uint4* q4 = reinterpret_cast<const uint4*>(row);
  const int nq = L >> 2;
  if (nq <= 4) {
    uint32_t j = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (q < nq) j += ctrl_count4(q4[q], y);
    return j;
  }
  int base = 0, len = nq;  // the number of full quads lies in [base, base + len - 1]
  while (len > 1) {
    const int half = len >> 1;
    base = (y >= row[4 * (base + half - 1) + 3]) ? base + half : base;
    len -= half;
  }
  return 4u * (uint32_t)base + ctrl_count4(q4[base], y);
}

// A node >= M (only through gp_controller_nodes) is flagged and clamped, so that its row stays inside the table.
template <class N>
__device__ __forceinline__ void ctrl_clamp_node(N& nd, int M, bool live, uint32_t* derr) {
  if (nd >= M) {
    if (live) atomicOr(derr, GP_DERR_CTRL);
    nd = (N)(M - 1);
  }
}
// j of (node nd, obs o) for the draw y < 2^31, out of the table at `thr` (global memory or its LDS copy). An obs
// >= n_obs (a table smaller than the obs space) is flagged and clamped. L: entries per stored row; lreal: those before
// its padding to 16-B quads (the result never names a padding entry; < lreal by the row's last entry, 2^31 > y).
// I: the type the row's entry index is computed in (a table holds at most 2^28 entries: 32 bits hold it).
template <class I = size_t, class NO>
__device__ __forceinline__ uint32_t ctrl_pick(const uint32_t* thr, uint32_t nd, NO n_obs, int L, uint32_t lreal,
                                              uint32_t o, uint32_t y, bool live, uint32_t* derr) {
  if (o >= (uint32_t)n_obs) {
    if (live) atomicOr(derr, GP_DERR_CTRL);
    o = (uint32_t)n_obs - 1u;
  }
  const uint32_t* row = thr + ((I)nd * (I)n_obs + o) * (I)L;
  return min(ctrl_search(row, L, y), lreal - 1u);
}
// j = action * M + next_node: the action j / M by CtrlDev::inv_m, and j % M, the next node unless the episode ended
// (then node 0: the caller's choice, stated where it has the step's flags).
__device__ __forceinline__ uint32_t ctrl_action(uint32_t j, uint32_t inv_m) { return (j * inv_m) >> 16; }
__device__ __forceinline__ uint32_t ctrl_node(uint32_t j, uint32_t a, int M) { return j - a * (uint32_t)M; }

// Host side of gp_set_controller: thr_host [rows][L] with rows = n_nodes * n_obs must be nondecreasing within
// [0, 2^31] and end at 2^31 (else GP_E_INVALID, naming the row). With `padded` ([rows][Lp], Lp >= L) the rows are
// copied there, each filled up to Lp entries with 2^31, which no y < 2^31 reaches (kinds whose L is no multiple of 4).
inline int ctrl_validate_rows(const uint32_t* thr_host, size_t rows, int n_obs, int L, int Lp = 0,
                              uint32_t* padded = nullptr) {
  constexpr uint32_t TOP = 1u << 31;
  for (size_t r = 0; r < rows; ++r) {
    const uint32_t* t = thr_host + r * L;
    uint32_t prev = 0;
    for (int i = 0; i < L; ++i) {
      if (t[i] < prev || t[i] > TOP) {
        gp_set_error("gp_set_controller: row (node %zu, obs %zu) is not nondecreasing within [0, 2^31] at entry %d",
                     r / (size_t)n_obs, r % (size_t)n_obs, i);
        return GP_E_INVALID;
      }
      prev = t[i];
    }
    if (prev != TOP) {
      gp_set_error("gp_set_controller: row (node %zu, obs %zu) ends at %u, not 2^31", r / (size_t)n_obs,
                   r % (size_t)n_obs, prev);
      return GP_E_INVALID;
    }
    if (padded)
      for (int i = 0; i < Lp; ++i) padded[r * Lp + i] = i < L ? t[i] : TOP;
  }
  return GP_OK;
}

// The host side of an installed controller, or of a GRID population of n_ctrl of them: the device table, the node
// plane [B] and the CtrlDev the kernels take.
struct CtrlHost {
  CtrlDev dev{};  // M == 0: nothing installed
  DevBuf b_thr, b_node;
  int bad_ctrl = -1;  // install() of a population: the controller whose row failed ctrl_validate_rows (-1: none did)

  // install()'s first check (the population states its own checks between this one and the rest)
  static int check_range(const char* what, int n_nodes, int n_obs) {
    if (n_nodes >= 1 && n_nodes <= 8 && n_obs >= 1 && n_obs <= (1 << 24)) return GP_OK;
    gp_set_error("%s: n_nodes must be in [1, 8] and n_obs in [1, 2^24] (got %d, %d)", what, n_nodes, n_obs);
    return GP_E_INVALID;
  }
  // gp_set_controller(NULL): nothing installed any more.
  int clear() {
    GP_HIP_CHECK(hipDeviceSynchronize());  // (an earlier launch may still read the table being replaced)
    dev = CtrlDev{};
    int e;
    if ((e = b_thr.alloc(0)) || (e = b_node.alloc(0))) return e;
    return GP_OK;
  }
  // Validates and uploads thr_host [n_ctrl][n_nodes][n_obs][A * n_nodes] for B envs of A actions; `what` names the API
  // call in the error texts, n_ctrl > 0 says it is a population. A refused table (GP_E_INVALID) leaves what was
  // installed; a failed allocation leaves nothing. Rows whose L = A * n_nodes is no multiple of 4 are padded with 2^31
  // to Lp entries, so that ctrl_search keeps its 16-B quads. dev.bytes is ONE controller's table; dev.lds_off = -1
  // (stage() decides otherwise) and every node is 0.
  int install(const char* what, int A, int n_nodes, int n_obs, const uint32_t* thr_host, int64_t B, int n_ctrl = 0) {
    GP_HIP_CHECK(hipDeviceSynchronize());  // (an earlier launch may still read the table being replaced)
    bad_ctrl = -1;
    if (int e = check_range(what, n_nodes, n_obs)) return e;
    const int L = A * n_nodes, Lp = (L + 3) & ~3;
    if (L > CTRL_MAX_L) {
      gp_set_error("%s: %d actions x %d nodes = %d joint choices, more than %d", what, A, n_nodes, L, CTRL_MAX_L);
      return GP_E_INVALID;
    }
    const int P = n_ctrl > 0 ? n_ctrl : 1;
    const size_t rows = (size_t)n_nodes * (size_t)n_obs, n1 = rows * (size_t)Lp, n = n1 * (size_t)P;
    if (n > ((size_t)1 << 28)) {
      if (n_ctrl > 0) gp_set_error("%s: tables of %zu entries in total are too large (max 2^28)", what, n);
      else gp_set_error("%s: a table of %zu entries is too large (max 2^28)", what, n);
      return GP_E_INVALID;
    }
    std::vector<uint32_t> padded(Lp != L ? n : 0);
    for (int c = 0; c < P; ++c)
      if (int e = ctrl_validate_rows(thr_host + (size_t)c * rows * (size_t)L, rows, n_obs, L, Lp,
                                     Lp != L ? padded.data() + (size_t)c * n1 : nullptr)) {
        bad_ctrl = n_ctrl > 0 ? c : -1;
        return e;
      }
    dev = CtrlDev{};  // (nothing installed if an allocation below fails)
    int e;
    if ((e = b_thr.alloc(n * sizeof(uint32_t) + 16)) || (e = b_node.alloc((size_t)B + 16))) return e;  // nodes zeroed
    GP_HIP_CHECK(hipMemcpy(b_thr.p, Lp != L ? padded.data() : thr_host, n * sizeof(uint32_t), hipMemcpyHostToDevice));
    dev.thr = b_thr.as<uint32_t>();
    dev.node = b_node.as<uint8_t>();
    dev.M = n_nodes;
    dev.n_obs = n_obs;
    dev.L = Lp;
    dev.inv_m = (65536u + (uint32_t)n_nodes - 1u) / (uint32_t)n_nodes;
    dev.bytes = (int32_t)std::min(n1 * sizeof(uint32_t), (size_t)INT32_MAX);
    dev.lds_off = -1;
    return GP_OK;
  }
  // The staging rule: the table goes into LDS behind the env's env_lds_bytes of tables when the kind can stage at all
  // and both fit CTRL_LDS_BUDGET (knob ctrl_lds_max, at most 60 KB: with a kernel's static LDS a launch stays below
  // 64 KB). Sets dev.lds_off and returns the dynamic LDS of a closed-loop launch.
  size_t stage(size_t env_lds_bytes, bool can_stage) {
    const int knob = gp_debug_knobs().ctrl_lds_max;
    const size_t budget = knob >= 0 ? std::min((size_t)knob, (size_t)60 * 1024) : (size_t)CTRL_LDS_BUDGET;
    const bool staged = can_stage && env_lds_bytes + (size_t)dev.bytes <= budget;
    dev.lds_off = staged ? (int32_t)env_lds_bytes : -1;
    return env_lds_bytes + (staged ? (size_t)dev.bytes : 0);
  }
  // gp_controller_nodes, and gp_reset's "every node back to 0"
  int nodes(uint8_t* get, const uint8_t* set, int64_t B, hipStream_t s) const {
    if (!dev.M) {
      gp_set_error("gp_controller_nodes without a controller (gp_set_controller)");
      return GP_E_STATE;
    }
    if (get) GP_HIP_CHECK(hipMemcpyAsync(get, dev.node, (size_t)B, hipMemcpyDeviceToDevice, s));
    if (set) GP_HIP_CHECK(hipMemcpyAsync(dev.node, set, (size_t)B, hipMemcpyDeviceToDevice, s));
    return GP_OK;
  }
  int reset_nodes(int64_t B, hipStream_t s) const {
    if (dev.M) GP_HIP_CHECK(hipMemsetAsync(dev.node, 0, (size_t)B, s));
    return GP_OK;
  }
  // gp_rollout_controller's precondition
  int ready(bool has_reset) const {
    if (has_reset && dev.M) return GP_OK;
    gp_set_error(!has_reset ? "rollout_controller() before reset()" : "rollout_controller() without a controller "
                                                                      "(gp_set_controller)");
    return GP_E_STATE;
  }
};
