// smx_batch.h — many independent small merges in one call (smx_compose_batch).
//
// A merge of at most SMALL_N ops is one workgroup's work (smx_small.h), so a caller with
// many of them -- a merge queue, a rebase, a monorepo merged package by package -- wants
// them spread over the chip, not one launch, two copies and a sync each to keep one CU
// busy.  Here a pre-pass sorts the merges into size classes and one launch per class
// runs them: compose_small<N> at N = 256, 1024 and 2048 ops, N / 2 threads and ~64 N
// bytes of LDS per workgroup, so that a batch of 100-op merges puts several workgroups on
// each CU where the 2048-op instance alone fills it (DESIGN.md §11 has the resource table).
//
//   k_batch_classify  one workgroup reads every merge's bounds, checks them before any
//                     column is touched, and appends the merge to its class's list in
//                     the workspace (or fails it: counts -1 for bad bounds, -2 for a merge
//                     over SMALL_N ops, which the caller sends through smx_compose)
//   k_compose_batch<N> a grid capped by the class's residency; workgroup b runs the merges
//                     b, b + grid, ... of the class list one after another, a barrier
//                     between two (compose_small sets up all its LDS state per merge)
// Nothing here waits, allocates or reads back: four launches on the caller's stream.
//
// With SMX_BATCH_LARGE (smx_compose_batch_ex) the limit of SMALL_N ops is gone, in five launches:
//   k_batch_classify<.., true>  no -2; a merge over SMALL_N ops goes on a fourth list
//   k_compose_batch_large  after the three classes: one 1024-thread workgroup per merge of that
//                     list runs the same four steps through global memory (smx_batch_large.h)
//
// smx_compose_batch_shared is the same for merges that all have one log on one side (a merge
// queue against the target branch, a rebase against upstream): the shared log is stored once,
// ops [0, n_shared) of the columns, and every merge reads it from there (compose_small reads B
// op j at j + b_gap, so one copy serves every merge); only the results, n_shared + len_m
// entries per merge, are laid out per merge.
//
// smx_compose_pairs is the same for pairs of logs stored once, as smx_screen takes them
// (DESIGN.md §17): pair p is (log pair_a[p], log pair_b[p]), B op j read at j + b_gap with
// b_gap = log_off[b] - (log_off[a] + len_a), of either sign, and its results lie at res_off[p].
// Its pre-pass is two kernels, because tens of thousands of pairs are too many for one
// workgroup's loop:
//   k_pairs_offsets   one workgroup checks log_off and res_off with a running maximum each
//                     (smx_screen.h's screen_log_bounds) and clears the class counts
//   k_pairs_classify  a grid over the pairs, BATCH_CHUNK each: checks the pair, fails it or
//                     appends it to its class's list (k_screen_classify's shape)
// Five launches (six with SMX_BATCH_LARGE), nothing waited for, allocated or read back.
//
// All run the same two compose kernels, templates over the batch struct B; what differs between
// smx_batch, smx_batch_shared and smx_pairs is in two overloaded functions: batch_check (a
// merge's bounds and its length) and batch_merge (its smx_ops and smx_compose_out).  The entry
// points are in smx_batch.hip.
#pragma once

#include "smx_screen.h"
#include "smx_small.h"

#define BATCH_CLASSES 3
#define BATCH_HDR 256  // workspace: class counts (u32), then the class lists [BATCH_CLASSES][n_merges] (u32)
__host__ __device__ constexpr int batch_class_cap(int c) { return c == 0 ? 256 : c == 1 ? 1024 : SMALL_N; }
static_assert(batch_class_cap(BATCH_CLASSES - 1) == SMALL_N, "the last class holds every small merge");

static inline size_t batch_list_bytes(int64_t n_merges) { return ((size_t)n_merges * 4 + 255) & ~(size_t)255; }

// Merge m's bounds, checked before any column is touched: its length in ops (the shared
// log included), or -1 for bad bounds, -2 for a merge over SMALL_N ops.
__device__ __forceinline__ i64 batch_check(const smx_batch& b, i64 m) {
  const i64 o0 = b.off[m], o1 = b.off[m + 1], na = b.n_a[m], c0 = b.conf_off[m], c1 = b.conf_off[m + 1];
  const i64 len = o1 - o0;
  if (o0 < 0 || o1 < o0 || o1 > b.n_total || na < 0 || na > len || c0 < 0 || c1 < c0) return -1;
  return len > SMALL_N ? -2 : len;
}
// The shared-log batch: merge m is (shared, own_m) or, with shared_is_b, (own_m, shared); its
// class is that of n_shared + len_m.
__device__ __forceinline__ i64 batch_check(const smx_batch_shared& b, i64 m) {
  const i64 o0 = b.off[m], o1 = b.off[m + 1], c0 = b.conf_off[m], c1 = b.conf_off[m + 1];
  if (o0 < b.n_shared || o1 < o0 || o1 > b.n_total || c0 < 0 || c1 < c0) return -1;
  if (o1 - o0 > SMALL_N - b.n_shared) return -2;  // (o1 - o0 <= n_total: no overflow)
  return b.n_shared + (o1 - o0);
}

// The pairs form: the logs' and the result offsets' verdicts of k_pairs_offsets (linfo by log,
// rinfo by pair: -1 for an offset below 0 or below an earlier one, an end before its start or
// past n_total / n_out), then what only the pair knows.
__device__ __forceinline__ i64 batch_check(const smx_pairs& b, i64 p, const i32* linfo, const i32* rinfo) {
  const i64 la = b.pair_a[p], lb = b.pair_b[p], c0 = b.conf_off[p], c1 = b.conf_off[p + 1];
  if (la < 0 || la >= b.n_logs || lb < 0 || lb >= b.n_logs || c0 < 0 || c1 < c0) return -1;
  if (linfo[la] < 0 || linfo[lb] < 0 || rinfo[p] < 0) return -1;
  // (valid logs and a valid region: every difference is within [0, n_total] or [0, n_out])
  const i64 len = (b.log_off[la + 1] - b.log_off[la]) + (b.log_off[lb + 1] - b.log_off[lb]);
  if (b.res_off[p + 1] - b.res_off[p] < len) return -1;
  return len > SMALL_N ? -2 : len;
}

// LARGE (SMX_BATCH_LARGE): no merge gets -2; one over SMALL_N ops goes on a fourth list,
// large_list, for k_compose_batch_large (smx_batch_large.h), its count in cnt[BATCH_CLASSES].
template <typename B, bool LARGE>
__global__ void __launch_bounds__(256) k_batch_classify(B b, u32* cnt, u32* lists, size_t list_stride,
                                                        u32* large_list) {
  constexpr int NC = BATCH_CLASSES + (LARGE ? 1 : 0);
  __shared__ u32 c[NC];
  const int t = threadIdx.x;
  if (t < NC) c[t] = 0;
  __syncthreads();
  for (i64 m = t; m < b.n_merges; m += 256) {
    const i64 len = batch_check(b, m);
    if (LARGE && len == -2) {
      large_list[atomicAdd(&c[BATCH_CLASSES], 1u)] = (u32)m;
      continue;
    }
    if (len < 0) {
      b.counts[2 * m] = len;
      b.counts[2 * m + 1] = len;
      continue;
    }
    int k = 0;
    while (len > batch_class_cap(k)) ++k;
    lists[(size_t)k * list_stride + atomicAdd(&c[k], 1u)] = (u32)m;
  }
  __syncthreads();
  if (t < NC) cnt[t] = c[t];
}

// Merge m's input and output as compose_small takes them.
__device__ __forceinline__ void batch_merge(const smx_batch& b, i64 m, smx_ops* ops, smx_compose_out* out) {
  const i64 o = b.off[m], len = b.off[m + 1] - o, na = b.n_a[m], co = b.conf_off[m];
  *ops = smx_ops{na, len - na, b.n_sym, b.kind + o, b.ts + o, b.oid_hi + o, b.oid_lo + o, b.sym + o, b.v0 + o,
                 b.v1 + o, 0};
  *out = smx_compose_out{b.order + o, b.addr + o, b.file + o, b.ctx + o, b.conflicts + 2 * co,
                         b.conf_off[m + 1] - co, b.counts + 2 * m};
}
__device__ __forceinline__ void batch_merge(const smx_batch_shared& b, i64 m, smx_ops* ops, smx_compose_out* out) {
  const i64 o = b.off[m], len = b.off[m + 1] - o, co = b.conf_off[m];
  // shared log as A: the columns from their start, B (the merge's own ops) o - n_shared
  // entries after A's end.  Shared log as B: the columns from the merge's own ops, and B op
  // j (j >= len) back at the columns' start, j - len = (o + j) - (o + len).  That gap is
  // negative: internal to this kernel (compose_small adds it to the index in 64 bits and
  // nothing else reads it; the public smx_compose rejects b_gap < 0).
  const i64 base = b.shared_is_b ? o : 0;
  *ops = smx_ops{b.shared_is_b ? len : b.n_shared,
                 b.shared_is_b ? b.n_shared : len,
                 b.n_sym,
                 b.kind + base,
                 b.ts + base,
                 b.oid_hi + base,
                 b.oid_lo + base,
                 b.sym + base,
                 b.v0 + base,
                 b.v1 + base,
                 b.shared_is_b ? -(o + len) : o - b.n_shared};
  const i64 r = o + (m - 1) * b.n_shared;  // n_shared + len result entries per merge, in input order
  *out = smx_compose_out{b.order + r, b.addr + r, b.file + r, b.ctx + r, b.conflicts + 2 * co,
                         b.conf_off[m + 1] - co, b.counts + 2 * m};
}

// Pair p = (log a, log b): the columns from log a's start, B op j (j >= len_a) at
// log_off[b] + (j - len_a) = (log_off[a] + j) + b_gap.  The gap has either sign (log b stored
// before log a, a self pair: -len_a) and is internal to these kernels, as the shared form's.
__device__ __forceinline__ void batch_merge(const smx_pairs& b, i64 p, smx_ops* ops, smx_compose_out* out) {
  const i64 la = b.pair_a[p], lb = b.pair_b[p];
  const i64 oa = b.log_off[la], na = b.log_off[la + 1] - oa, ob = b.log_off[lb], nb = b.log_off[lb + 1] - ob;
  const i64 r = b.res_off[p], co = b.conf_off[p];
  *ops = smx_ops{na, nb, b.n_sym, b.kind + oa, b.ts + oa, b.oid_hi + oa, b.oid_lo + oa, b.sym + oa, b.v0 + oa,
                 b.v1 + oa, ob - (oa + na)};
  *out = smx_compose_out{b.order + r, b.addr + r, b.file + r, b.ctx + r, b.conflicts + 2 * co,
                         b.conf_off[p + 1] - co, b.counts + 2 * p};
}

// The pairs form's pre-pass.  Workspace behind the class counts: linfo [n_logs], rinfo
// [n_pairs], then the class lists as in the other two forms.
// Pairs per workgroup of k_pairs_classify: one per thread.  A pair's check is a chain of dependent
// loads (pair -> log_off -> res_off), so a thread that takes several pairs pays the chain once per
// pair: at 8 per thread the kernel took 10.3 us for 1128 pairs.
#define BATCH_CHUNK 256
static inline size_t pairs_info_bytes(int64_t n_logs, int64_t n_pairs) {
  return batch_list_bytes(n_logs) + batch_list_bytes(n_pairs);
}

__global__ void __launch_bounds__(1024) k_pairs_offsets(smx_pairs b, u32* cnt, i32* linfo, i32* rinfo) {
  __shared__ i64 sc[1024 / WAVE + 1];
  if (threadIdx.x < BATCH_CLASSES + 1) cnt[threadIdx.x] = 0;
  screen_log_bounds(b.log_off, b.n_logs, b.n_total, linfo, sc);
  screen_log_bounds(b.res_off, b.n_pairs, b.n_out, rinfo, sc);  // (the scan ends with a barrier: sc is free)
}

template <bool LARGE>
__global__ void __launch_bounds__(256) k_pairs_classify(smx_pairs b, u32* cnt, const i32* linfo, const i32* rinfo,
                                                        u32* lists, size_t list_stride, u32* large_list) {
  constexpr int PER = BATCH_CHUNK / 256;
  constexpr int NC = BATCH_CLASSES + (LARGE ? 1 : 0);
  __shared__ u32 c[NC], start[NC];
  const int t = threadIdx.x;
  if (t < NC) c[t] = 0;
  __syncthreads();
  const i64 p0 = (i64)blockIdx.x * BATCH_CHUNK;
  int cls[PER];
  u32 rk[PER];
#pragma unroll
  for (int q = 0; q < PER; ++q) {
    const i64 p = p0 + q * 256 + t;
    cls[q] = -1;
    rk[q] = 0;
    if (p >= b.n_pairs) continue;
    const i64 len = batch_check(b, p, linfo, rinfo);
    if (len < 0 && !(LARGE && len == -2)) {
      b.counts[2 * p] = len;
      b.counts[2 * p + 1] = len;
      continue;
    }
    int k = 0;
    if (len < 0) k = BATCH_CLASSES;
    else
      while (len > batch_class_cap(k)) ++k;
    cls[q] = k;
    rk[q] = atomicAdd(&c[k], 1u);
  }
  __syncthreads();
  if (t < NC) start[t] = c[t] ? atomicAdd(&cnt[t], c[t]) : 0u;
  __syncthreads();
#pragma unroll
  for (int q = 0; q < PER; ++q) {
    if (LARGE && cls[q] == BATCH_CLASSES) large_list[start[BATCH_CLASSES] + rk[q]] = (u32)(p0 + q * 256 + t);
    else if (cls[q] >= 0) lists[(size_t)cls[q] * list_stride + start[cls[q]] + rk[q]] = (u32)(p0 + q * 256 + t);
  }
}

template <int N, typename B>
__global__ void __launch_bounds__(N / 2) k_compose_batch(B b, const u32* cnt, const u32* list) {
  const u32 c = *cnt;
  for (u32 i = blockIdx.x; i < c; i += gridDim.x) {
    smx_ops ops;
    smx_compose_out out;
    batch_merge(b, (i64)list[i], &ops, &out);
    compose_small<N, false>(ops, out, nullptr, nullptr, 0);
    __syncthreads();  // the next merge's load overwrites what this one's last phase reads
  }
}
