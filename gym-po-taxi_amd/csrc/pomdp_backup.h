// pomdp_backup.h — the point-based value backup of the tabular POMDP (pomdp_backup.hip; gp_belief_backup, DESIGN.md
// §6s): what PomdpBackend (pomdp.hip) keeps per handle and calls. Not part of the C ABI.
#pragma once
#include "gp_internal.h"

// What the backup reads of a handle with an enabled filter: the model blob and the filter's compressed columns of Tf.
struct PbModel {
  int S = 0, A = 0, O = 0, Sp = 0, Op = 0;
  const uint32_t* blob = nullptr;  // trans [S A][Sp] | obs [A S][Op] | ... | reward [S A S] | terminal bytes [S]
  uint32_t off_obs = 0, off_rew = 0, off_term = 0;  // in words
  const uint32_t* colptr = nullptr;                 // [A S + 1] column (a, s') of Tf (BfDev)
  const uint2* ent = nullptr;                       // (s, bits of Tf[s][a][s'])
};

// Limits of one call beyond the policy's (N <= 4,096, N S <= 2^22): P points and the scratch they need.
constexpr int PB_MAX_POINTS = 1 << 20;
constexpr size_t PB_MAX_SCRATCH = (size_t)1 << 30;

// The backup's own tables (built from the blob at the first call after gp_belief_enable), its copy of the caller's
// vectors and its scratch. Everything is freed by release() (gp_belief_disable, gp_destroy).
struct PbHost {
  bool built = false;
  DevBuf b_rowptr, b_rent;  // rows (s, a) of Tf: (s', bits of Tf), s' ascending
  DevBuf b_zcptr, b_zcent;  // per (a, o): (s', bits of Zf[a][s'][o]) of the non-terminal s' with Zf != 0, s' ascending
  DevBuf b_zrptr, b_zrent;  // per (a, s'), s' not terminal: (o, bits of Zf[a][s'][o]) with Zf != 0, o ascending
  DevBuf b_alpha;           // [N][S] of the running call
  DevBuf b_acc, b_jst;      // scratch: acc, then beta, float [P][A][S]; j* uint16 [P][A][O]
  size_t scratch_bytes() const { return b_acc.n + b_jst.n; }
  void release();
  int build(const PbModel& m);
  int backup(const PbModel& m, int P, const float* points, int N, const float* alpha, float gamma, float* alpha_out,
             int32_t* act_out, float* value_out, hipStream_t s);
  // Step 1 alone, for the expansion (pomdp_expand.hip): builds the tables if need be, grows b_acc to P points and
  // launches pb_acc on `s`. acc [P][A][S] is then b_acc.
  int acc_points(const PbModel& m, int P, const float* points, hipStream_t s);
};
