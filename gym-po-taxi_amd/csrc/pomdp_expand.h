// pomdp_expand.h — the belief-set expansion of the tabular POMDP (pomdp_expand.hip; gp_belief_expand):
// what PomdpBackend (pomdp.hip) keeps per handle and calls. Not part of the C ABI.
#pragma once
#include "pomdp_backup.h"

// Limits of one call: P points, Q reference rows, and the scratch they need.
constexpr int PX_MAX_POINTS = 1 << 20;
constexpr size_t PX_MAX_SCRATCH = (size_t)1 << 30;

// The expansion's scratch beside the backup's. acc [P][A][S] is the backup's own b_acc (PbHost::acc_points), and the
// (a, o) lists of Zf are the backup's tables. Everything here is freed by release() (gp_belief_disable, gp_destroy).
struct PxHost {
  DevBuf b_n;     // n(a, o), float [P][A][O]
  DevBuf b_best;  // per (p, a): (dist, o) of the first maximiser over the live o (o = -1: none), float2 [P][A]
  DevBuf b_qt;    // the reference set transposed, float [S][Q]
  size_t own_bytes() const { return b_n.n + b_best.n + b_qt.n; }
  void release();
  int expand(PbHost& pb, const PbModel& m, int P, const float* points, int Q, const float* ref, float* succ_out,
             float* dist_out, int32_t* act_out, int32_t* obs_out, float* mass_out, hipStream_t s);
};
