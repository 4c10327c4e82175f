// smx_train_step.h — one step of a merge train of any size, on either side of smx_compose
// (smx_train_stage, smx_train_land).
//
// k_compose_train (smx_train.h) runs a train inside one workgroup, and so stops at 2048 ops.  What
// leads from one compose to the next is a gather (§21), and smx_compose composes a merge of any
// size over the whole chip: a train of any size is therefore a host loop of
//   k_train_stage   the step's input columns: the accumulator's, gathered through src with the
//                   moves rewritten, and the log's behind them -- the staging loop of
//                   k_compose_train, entry by entry, by the same rule (train_staged)
//   smx_compose     on those columns (n_a = n_acc, n_b = log_n, b_gap = 0)
//   k_train_land    the landing loop of k_compose_train, or its conflict records, by the same
//                   rules (train_landed, train_conflict_record)
// over columns that stay on the device.  Both kernels are streaming gathers: a thread per entry
// on a grid-stride grid, coalesced writes, reads through src / order, no LDS, no barrier.  The
// entry points are in smx_batch.hip.
#pragma once

#include "smx_train.h"  // the step's per-entry rules: train_staged, train_landed, train_conflict_record

constexpr int TRAIN_STEP_T = 256;
// (enough workgroups to fill the chip several times over; longer steps stride)
constexpr i64 TRAIN_STEP_MAX_GRID = 8192;

static inline unsigned train_step_grid(i64 n) {
  const i64 g = SMX_CEIL_DIV(n, (i64)TRAIN_STEP_T);
  return (unsigned)(g < TRAIN_STEP_MAX_GRID ? g : TRAIN_STEP_MAX_GRID);
}

// status[0] was cleared ahead of the kernel (stream-ordered); a thread that meets a bad entry
// stores -1, whichever of them comes last.
__global__ void __launch_bounds__(TRAIN_STEP_T) k_train_stage(smx_train_step s) {
  const i64 n = s.n_acc + s.log_n;
  const i64 stride = (i64)gridDim.x * TRAIN_STEP_T;
  for (i64 e = (i64)blockIdx.x * TRAIN_STEP_T + threadIdx.x; e < n; e += stride) {
    i64 j = s.log_lo + (e - s.n_acc);
    i32 a = SMX_NONE, f = SMX_NONE;
    if (e < s.n_acc) {
      j = s.acc_src[e];
      a = s.acc_addr[e];
      f = s.acc_file[e];
    }
    if (j < 0 || j >= s.n_total) {  // a src outside the columns: not read through
      s.st_kind[e] = 0xFF;          // (and smx_compose, should it run, sees an invalid op)
      s.st_sym[e] = 0xFFFFFFFFu;
      s.status[0] = -1;
      continue;
    }
    const u8 k = s.kind[j];
    const u32 y = s.sym[j];
    if (k >= SMX_N_KINDS || (i64)y >= s.n_sym) s.status[0] = -1;  // (copied as it is: smx_compose refuses it too)
    i32 x0, x1;
    train_staged(k, s.v0[j], s.v1[j], a, f, s.empty_str, s.v1_alt, j, x0, x1);
    s.st_kind[e] = k;
    s.st_ts[e] = s.ts[j];
    s.st_oid_hi[e] = s.oid_hi[j];
    s.st_oid_lo[e] = s.oid_lo[j];
    s.st_sym[e] = y;
    s.st_v0[e] = x0;
    s.st_v1[e] = x1;
  }
}

// An element index of the compose result that does not name an entry of the step (a caller's
// buffer that smx_compose did not fill) is never read through.
__global__ void __launch_bounds__(TRAIN_STEP_T) k_train_land(smx_train_step s) {
  const i64 n = s.n_acc + s.log_n;
  const i64 stride = (i64)gridDim.x * TRAIN_STEP_T;
  const i64 first = (i64)blockIdx.x * TRAIN_STEP_T + threadIdx.x;
  const i64 k = s.counts[0], nc = s.counts[1];
  if (k < 0 || s.status[0] != 0) {
    if (first == 0) s.status[1] = -1;
    return;
  }
  if (nc > 0) {
    if (first == 0) {
      s.status[1] = nc;
      s.status[2] = s.n_acc;
    }
    i64 cap = nc < s.conflict_cap ? nc : s.conflict_cap;
    if (cap > s.record_cap) cap = s.record_cap;
    for (i64 q = first; q < cap; q += stride) {
      const i64 ea = s.conflicts[2 * q], eb = s.conflicts[2 * q + 1];
      if (ea < 0 || ea >= s.n_acc || eb < s.n_acc || eb >= n) continue;
      train_conflict_record(s.records + 4 * q, ea, eb, s.n_acc, s.log_lo, s.acc_src, s.acc_addr, s.acc_file);
    }
    return;
  }
  const i64 len = k < n ? k : n;
  if (first == 0) {
    s.status[1] = 0;
    s.status[2] = len;
  }
  for (i64 q = first; q < len; q += stride) {
    const i64 e = s.order[q];
    if (e < 0 || e >= n) continue;
    train_landed(e, s.n_acc, s.log_lo, s.acc_src, s.acc_addr, s.acc_file, s.acc_ctx, s.addr[q], s.file[q], s.ctx[q],
                 s.out_src, s.out_addr, s.out_file, s.out_ctx, q);
  }
}
