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
// Both run the same two kernels, templates over the batch struct B; what differs between
// smx_batch and smx_batch_shared is in two overloaded functions: batch_check (a merge's
// bounds and its length) and batch_merge (its smx_ops and smx_compose_out).  The entry
// points are in smx_batch.hip.
#pragma once

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
