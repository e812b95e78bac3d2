// gp_ctrl.h — the tabular finite-state controller of the closed-loop rollouts (gp_set_controller; semantics in
// include/gym_po_amd.h), shared by the kinds that run it (grid.hip, rocksample.hip, anttag.hip, taxi.hip, heavenhell.hip, crooms.hip): the device view of an
// installed table, the threshold-row search and the host-side validation of a table. Per env-step one Philox block tagged
// CTRL_TAG picks j = action * M + next_node from the threshold row of (node, obs).
#pragma once
#include "../../include/gym_po_amd.h"
#include "gp_common.h"

// the env draws carry 0x67706f21 (grid) / 0x726f636b (rocksample) / 0x616e7431 (anttag) / 0x74617869 (taxi) /
// 0x6868656c (heavenhell) / 0x63726f6f and 0x6d733121 (crooms)
constexpr uint32_t CTRL_TAG = 0x67706f63u;
// Largest dynamic LDS per block (env tables + controller table) up to which the kinds that stage the table in LDS
// (grid.hip, taxi.hip, heavenhell.hip, crooms.hip) do so by default; the knob ctrl_lds_max overrides it, up to 60 KB.
constexpr int CTRL_LDS_BUDGET = 32 * 1024;
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
