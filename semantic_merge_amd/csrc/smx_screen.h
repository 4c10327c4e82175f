// smx_screen.h — screen many pairs of logs for DivergentRename conflicts without composing
// them (smx_screen).
//
// The reference composes two logs and looks at the conflicts first; the composed ops are
// used only when there are none.  A merge queue or a monorepo asks that question for many
// pairs over few logs.  The conflict list of a pair is a function of the two logs' rename
// subsequences alone (smx_small.h step 2: T is ordered by precedence first, the
// DivergentRename test fires only between two renames, so both heads are renames exactly
// while both branches are in their rename blocks): each log's renames in (timestamp, id,
// index) order, merged A first on ties, and the two-head walk over that merged list.  So:
//
//   k_screen_logs      one workgroup checks every log's bounds (a prefix maximum over the
//                      offsets: a valid log starts at or after every earlier offset, so
//                      valid logs never overlap) and clears the class counts
//   k_screen_extract   per log, once however many pairs hold it: one workgroup walks the
//                      kind bytes in tiles, compacts the renames stably (counts, one scan
//                      per tile), loads their keys, sorts them (a bitonic sort in LDS, skipped
//                      when they are ordered already) and writes the sorted rename records
//                      (index in the log, symbol, newName class, keys) to the workspace at
//                      the log's own offset, with the log's rename count (-1: invalid log,
//                      SCREEN_N + 1: more than SCREEN_N renames)
//   k_screen_classify  per pair: checks the pair, fails it (counts -1 / -2), answers it at
//                      once when a side has no renames (counts 0), or appends it to the list
//                      of its size class (the renames of both logs together)
//   k_screen_pairs<N>  a grid capped by the class's residency; workgroup b takes the pairs
//                      b, b + grid, ... of the class list, a barrier between two.  Per pair:
//                      the two sorted lists into LDS, each rename's rank in the other list by
//                      binary search (A: B keys strictly below; B: A keys at or below -- the
//                      reference's `<=`), the position and next-rename arrays, and the wave
//                      walk of smx_small.h step 2 without skip marks, chains and emit.
// Nothing here waits, allocates or reads back: six launches on the caller's stream.
//
// With SMX_SCREEN_LARGE (smx_screen_ex) the limit of SCREEN_N renames is gone, in eight launches:
//   k_screen_extract_large  after k_screen_extract, for the logs it left at SCREEN_N + 1: all
//                      their renames, sorted by tiles in LDS and merge levels in the workspace
//   k_screen_classify<true>  no -2; a pair over SCREEN_N renames goes on a fourth list
//   k_screen_stream    after the three classes: a pair of the fourth list in rounds of
//                      SCREEN_N / 2 records per side, the same body as k_screen_pairs, each
//                      round starting at the heads where the one before ran out of a side
// The entry point (argument checks, residency-capped grids, the launches) is in smx_batch.hip.
#pragma once

#include "smx_common.h"

typedef struct smx_screen ScreenArgs;  // (the function smx_screen hides the struct's name)

#define SCREEN_N 2048     // renames per pair (both logs together) and per log
#define SCREEN_T1 512     // threads of k_screen_extract
#define SCREEN_TILE (4 * SCREEN_T1)  // kind bytes per tile of its walk
#define SCREEN_CLASSES 3
#define SCREEN_HDR 256    // workspace: class counts (u32)
#define SCREEN_CHUNK 2048 // pairs per workgroup of k_screen_classify
#define SCREEN_TL 1024    // threads of k_screen_extract_large
#define SCREEN_MERGE 8    // outputs per thread and step of its merge levels
static_assert(SCREEN_N % SCREEN_MERGE == 0, "a thread's outputs lie in one pair of runs");
__host__ __device__ constexpr int screen_class_cap(int c) { return c == 0 ? 128 : c == 1 ? 512 : SCREEN_N; }
static_assert(screen_class_cap(SCREEN_CLASSES - 1) == SCREEN_N, "the last class holds every pair under the limit");

// The workspace: class counts, per-log rename counts, the class lists, and the rename
// records (log l's at [log_off[l], log_off[l] + its rename count) of arrays of n_total).
struct ScreenWs {
  u32* cnt;      // [SCREEN_CLASSES]
  i32* linfo;    // [n_logs]
  u32* lists;    // [SCREEN_CLASSES][list_stride]
  size_t list_stride;
  u64 *rts, *rhi, *rlo;  // [n_total] keys
  u32 *ridx, *rsym;      // [n_total] index in the log, symbol
  i32* rv0;              // [n_total] newName class
};
static inline size_t screen_al(size_t x) { return (x + 255) & ~(size_t)255; }
static inline size_t screen_ws_bytes(int64_t n_logs, int64_t n_total, int64_t n_pairs) {
  return SCREEN_HDR + screen_al((size_t)n_logs * 4) + SCREEN_CLASSES * screen_al((size_t)n_pairs * 4) +
         3 * screen_al((size_t)n_total * 8) + 3 * screen_al((size_t)n_total * 4);
}
static inline ScreenWs screen_ws(void* workspace, int64_t n_logs, int64_t n_total, int64_t n_pairs) {
  char* p = (char*)workspace;
  ScreenWs w;
  w.cnt = (u32*)p;
  p += SCREEN_HDR;
  w.linfo = (i32*)p;
  p += screen_al((size_t)n_logs * 4);
  w.lists = (u32*)p;
  w.list_stride = screen_al((size_t)n_pairs * 4) / 4;
  p += SCREEN_CLASSES * screen_al((size_t)n_pairs * 4);
  const size_t q8 = screen_al((size_t)n_total * 8), q4 = screen_al((size_t)n_total * 4);
  w.rts = (u64*)p;
  w.rhi = (u64*)(p + q8);
  w.rlo = (u64*)(p + 2 * q8);
  p += 3 * q8;
  w.ridx = (u32*)p;
  w.rsym = (u32*)(p + q4);
  w.rv0 = (i32*)(p + 2 * q4);
  return w;
}

// What SMX_SCREEN_LARGE adds behind that workspace: the list of the fourth class (its count
// is cnt[SCREEN_CLASSES]) and two index arrays for the large logs' sort, log l's part of each
// at [log_off[l], ..) as with the records.
struct ScreenLargeWs {
  u32* list;      // [n_pairs]
  u32 *ia, *ib;   // [n_total]
};
static inline size_t screen_large_bytes(int64_t n_total, int64_t n_pairs) {
  return screen_al((size_t)n_pairs * 4) + 2 * screen_al((size_t)n_total * 4);
}
static inline ScreenLargeWs screen_large_ws(void* workspace, int64_t n_logs, int64_t n_total, int64_t n_pairs) {
  char* p = (char*)workspace + screen_ws_bytes(n_logs, n_total, n_pairs);
  ScreenLargeWs x;
  x.list = (u32*)p;
  p += screen_al((size_t)n_pairs * 4);
  x.ia = (u32*)p;
  x.ib = (u32*)(p + screen_al((size_t)n_total * 4));
  return x;
}

// The bounds of every log, by one workgroup of 1024 threads (smx_screen and
// smx_screen_candidates, smx_cand.h): linfo[l] = -1 for a log that starts below an earlier
// offset (or below 0), ends before it starts or ends past n_total, else 0.
// sc: 1024 / WAVE + 1 words of LDS.
__device__ __forceinline__ void screen_log_bounds(const i64* log_off, i64 n_logs, i64 n_total, i32* linfo, i64* sc) {
  const int t = threadIdx.x;
  i64 carry = 0;  // the largest offset before this chunk (negative offsets fail on their own)
  for (i64 l0 = 0; l0 < n_logs; l0 += 1024) {
    const i64 l = l0 + t;
    const i64 o0 = l < n_logs ? log_off[l] : 0;
    i64 tot;
    const i64 pre = block_excl_scan<OpMax, i64, 1024 / WAVE>(o0, sc, &tot);  // (syncs)
    const i64 pm = pre > carry ? pre : carry;
    if (l < n_logs) {
      const i64 o1 = log_off[l + 1];
      linfo[l] = (o0 < pm || o1 < o0 || o1 > n_total) ? -1 : 0;
    }
    carry = tot > carry ? tot : carry;
  }
}

__global__ void __launch_bounds__(1024) k_screen_logs(ScreenArgs s, ScreenWs w) {
  __shared__ i64 sc[1024 / WAVE + 1];
  if (threadIdx.x < SCREEN_CLASSES) w.cnt[threadIdx.x] = 0;
  screen_log_bounds(s.log_off, s.n_logs, s.n_total, w.linfo, sc);
}

// A stable sort of the n <= SCREEN_N renames whose keys lie in LDS by NT threads: a bitonic sort
// of ord (the positions 0 .. n - 1 on entry, the first n in order on return) on
// (ts, id, position); slots past n sort last.  Ends with a barrier.
template <int NT>
__device__ __forceinline__ void screen_sort_tile(const u64* kts, const u64* khi, const u64* klo, u16* ord, int n) {
  const int t = threadIdx.x;
  auto key_lt = [&](u32 x, u32 y) -> bool {  // (ts, id) of x < that of y
    if (kts[x] != kts[y]) return kts[x] < kts[y];
    if (khi[x] != khi[y]) return khi[x] < khi[y];
    return klo[x] < klo[y];
  };
  auto less = [&](u32 x, u32 y) -> bool {  // x before y (x != y)
    if ((int)x >= n || (int)y >= n) return (int)y >= n && (int)x < n;
    if (key_lt(x, y)) return true;
    if (key_lt(y, x)) return false;
    return x < y;
  };
  int P = 1;
  while (P < n) P <<= 1;
  for (int r = n + t; r < P; r += NT) ord[r] = (u16)r;
  __syncthreads();
  for (int k = 2; k <= P; k <<= 1) {
    for (int jj = k >> 1; jj > 0; jj >>= 1) {
      for (int a = t; a < P; a += NT) {
        const int b = a ^ jj;
        if (b > a) {
          const u32 x = ord[a], y = ord[b];
          const bool up = (a & k) == 0;
          if (up ? less(y, x) : less(x, y)) {
            ord[a] = (u16)y;
            ord[b] = (u16)x;
          }
        }
      }
      __syncthreads();
    }
  }
}

__global__ void __launch_bounds__(SCREEN_T1) k_screen_extract(ScreenArgs s, ScreenWs w) {
  constexpr int NW = SCREEN_T1 / WAVE;
  __shared__ __attribute__((aligned(16))) u64 keys[3][SCREEN_N];
  u64* kts = keys[0];
  u64* khi = keys[1];
  u64* klo = keys[2];
  __shared__ u32 sidx[SCREEN_N];  // the r-th rename of the log: its index in the log
  __shared__ u16 ord[SCREEN_N];   // (ts, id, index) order -> r
  __shared__ u32 sscan[NW + 1];
  const int t = threadIdx.x;
  for (i64 l = blockIdx.x; l < s.n_logs; l += gridDim.x) {
    if (w.linfo[l] >= 0) {  // (uniform: one word for the workgroup)
      const i64 o0 = s.log_off[l], len = s.log_off[l + 1] - o0;
      // the renames, compacted in log order; past SCREEN_N only counted (and only up to
      // SCREEN_N + 1), the walk goes on for the kinds' validity
      u32 cnt = 0, bad = 0;
      for (i64 base = 0; base < len; base += SCREEN_TILE) {
        u32 isr = 0, c = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const i64 j = base + 4 * t + i;
          if (j < len) {
            const u32 k = s.kind[o0 + j];
            bad |= k >= SMX_N_KINDS;
            if (k == SMX_KIND_RENAME) {
              isr |= 1u << i;
              ++c;
            }
          }
        }
        u32 tot;
        u32 pos = cnt + block_excl_scan<OpSum, u32, NW>(c, sscan, &tot);  // (syncs)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          if ((isr >> i) & 1) {
            if (pos < SCREEN_N) sidx[pos] = (u32)(base + 4 * t + i);
            ++pos;
          }
        }
        cnt = cnt + tot > SCREEN_N ? SCREEN_N + 1 : cnt + tot;
      }
      bad = __syncthreads_or(bad);  // (also: sidx is complete)
      if (bad || cnt > SCREEN_N) {
        if (t == 0) w.linfo[l] = bad ? -1 : SCREEN_N + 1;
      } else {
        const int n = (int)cnt;
        for (int r = t; r < n; r += SCREEN_T1) {
          const i64 g = o0 + sidx[r];
          kts[r] = s.ts[g];
          khi[r] = s.oid_hi[g];
          klo[r] = s.oid_lo[g];
          ord[r] = (u16)r;
        }
        __syncthreads();
        auto key_lt = [&](u32 x, u32 y) -> bool {  // (ts, id) of x < that of y
          if (kts[x] != kts[y]) return kts[x] < kts[y];
          if (khi[x] != khi[y]) return khi[x] < khi[y];
          return klo[x] < klo[y];
        };
        bool unordered = false;  // equal keys are in index order already
        for (int r = t + 1; r < n; r += SCREEN_T1) unordered |= key_lt((u32)r, (u32)r - 1);
        if (__syncthreads_or(unordered)) {
          screen_sort_tile<SCREEN_T1>(kts, khi, klo, ord, n);
        }
        // the log's records, in order
        for (int r = t; r < n; r += SCREEN_T1) {
          const u32 e = ord[r];
          const i64 g = o0 + sidx[e];
          w.rts[o0 + r] = kts[e];
          w.rhi[o0 + r] = khi[e];
          w.rlo[o0 + r] = klo[e];
          w.ridx[o0 + r] = sidx[e];
          w.rsym[o0 + r] = s.sym[g];
          w.rv0[o0 + r] = s.v0[g];
        }
        if (t == 0) w.linfo[l] = n;
      }
    }
    __syncthreads();  // the next log's walk overwrites what this one's last phase reads
  }
}

// An op of a log with its sort key, read from the columns: (ts, id, index in the log).
struct ScreenKey {
  u64 ts, hi, lo;
  u32 j;
};
__device__ __forceinline__ ScreenKey screen_key(const ScreenArgs& s, i64 o0, u32 j) {
  const i64 g = o0 + j;
  return ScreenKey{s.ts[g], s.oid_hi[g], s.oid_lo[g], j};
}
__device__ __forceinline__ bool screen_key_lt(const ScreenKey& x, const ScreenKey& y) {
  if (x.ts != y.ts) return x.ts < y.ts;
  if (x.hi != y.hi) return x.hi < y.hi;
  if (x.lo != y.lo) return x.lo < y.lo;
  return x.j < y.j;
}

// The logs of more than SCREEN_N renames (SMX_SCREEN_LARGE), which k_screen_extract left at
// SCREEN_N + 1 after checking every kind byte of theirs; any other log leaves at once.  One
// workgroup per log: the renames' indices compacted stably into ia (the log's slice has room
// for every op); the order test on the keys read through them; if it fails, a stable sort of
// the indices -- tiles of SCREEN_N by the bitonic sort in LDS into ib, then merge levels that
// double the runs (ib -> ia -> ib ..., every thread takes SCREEN_MERGE outputs at a time from
// its merge-path split, keys read from the columns; a run's indices are all below the next
// run's, so the index as the last key component keeps the merge stable); then the records
// gathered once, and the true rename count in linfo[l].
__global__ void __launch_bounds__(SCREEN_TL) k_screen_extract_large(ScreenArgs s, ScreenWs w, ScreenLargeWs x) {
  constexpr int NW = SCREEN_TL / WAVE;
  __shared__ __attribute__((aligned(16))) u64 keys[3][SCREEN_N];
  u64* kts = keys[0];
  u64* khi = keys[1];
  u64* klo = keys[2];
  __shared__ u32 sidx[SCREEN_N];  // the r-th rename of the tile: its index in the log
  __shared__ u16 ord[SCREEN_N];   // (ts, id, index) order -> r
  __shared__ u32 sscan[NW + 1];
  const int t = threadIdx.x;
  // (k_screen_logs clears the three class counts; the fourth is this mode's)
  if (blockIdx.x == 0 && t == 0) w.cnt[SCREEN_CLASSES] = 0;
  for (i64 l = blockIdx.x; l < s.n_logs; l += gridDim.x) {
    if (w.linfo[l] != SCREEN_N + 1) continue;  // (uniform: one word for the workgroup)
    const i64 o0 = s.log_off[l], len = s.log_off[l + 1] - o0;
    u32* ia = x.ia + o0;
    u32* ib = x.ib + o0;
    i64 n = 0;
    for (i64 base = 0; base < len; base += 4 * SCREEN_TL) {
      u32 isr = 0, c = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const i64 j = base + 4 * t + i;
        if (j < len && s.kind[o0 + j] == SMX_KIND_RENAME) {
          isr |= 1u << i;
          ++c;
        }
      }
      u32 tot;
      i64 pos = n + block_excl_scan<OpSum, u32, NW>(c, sscan, &tot);  // (syncs)
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if ((isr >> i) & 1) ia[pos++] = (u32)(base + 4 * t + i);
      n += tot;
    }
    __syncthreads();  // ia is complete
    bool unordered = false;  // equal keys are in index order already
    for (i64 r = t + 1; r < n; r += SCREEN_TL)
      unordered |= screen_key_lt(screen_key(s, o0, ia[r]), screen_key(s, o0, ia[r - 1]));
    const u32* fin = ia;
    if (__syncthreads_or(unordered)) {
      for (i64 b0 = 0; b0 < n; b0 += SCREEN_N) {
        const int m = (int)(n - b0 < SCREEN_N ? n - b0 : SCREEN_N);
        for (int r = t; r < m; r += SCREEN_TL) {
          const u32 j = ia[b0 + r];
          const i64 g = o0 + j;
          sidx[r] = j;
          kts[r] = s.ts[g];
          khi[r] = s.oid_hi[g];
          klo[r] = s.oid_lo[g];
          ord[r] = (u16)r;
        }
        screen_sort_tile<SCREEN_TL>(kts, khi, klo, ord, m);
        for (int r = t; r < m; r += SCREEN_TL) ib[b0 + r] = sidx[ord[r]];
        __syncthreads();  // the next tile's load overwrites what this one's last phase reads
      }
      u32* from = ib;
      u32* to = ia;
      for (i64 run = SCREEN_N; run < n; run *= 2) {
        // outputs [d0, e) of the run pair [a0, a1) [a1, b1): SCREEN_MERGE divides SCREEN_N,
        // so they lie in one pair
        for (i64 d0 = (i64)t * SCREEN_MERGE; d0 < n; d0 += (i64)SCREEN_TL * SCREEN_MERGE) {
          const i64 a0 = d0 / (2 * run) * (2 * run);
          const i64 a1 = a0 + run < n ? a0 + run : n, b1 = a0 + 2 * run < n ? a0 + 2 * run : n;
          const i64 na = a1 - a0, nb = b1 - a1, d = d0 - a0;
          const i64 e = d0 + SCREEN_MERGE < b1 ? d0 + SCREEN_MERGE : b1;
          // the first run's elements among the pair's first d outputs
          i64 lo = d > nb ? d - nb : 0, hi = d < na ? d : na;
          while (lo < hi) {
            const i64 mid = (lo + hi) >> 1;
            if (screen_key_lt(screen_key(s, o0, from[a1 + d - 1 - mid]), screen_key(s, o0, from[a0 + mid]))) hi = mid;
            else lo = mid + 1;
          }
          i64 i = lo, k = d - lo;
          ScreenKey ka = i < na ? screen_key(s, o0, from[a0 + i]) : ScreenKey{0, 0, 0, 0};
          ScreenKey kb = k < nb ? screen_key(s, o0, from[a1 + k]) : ScreenKey{0, 0, 0, 0};
          for (i64 o = d0; o < e; ++o) {
            if (i < na && (k >= nb || !screen_key_lt(kb, ka))) {
              to[o] = ka.j;
              if (++i < na) ka = screen_key(s, o0, from[a0 + i]);
            } else {
              to[o] = kb.j;
              if (++k < nb) kb = screen_key(s, o0, from[a1 + k]);
            }
          }
        }
        __syncthreads();  // the level is complete before the next one reads it
        u32* const sw = from;
        from = to;
        to = sw;
      }
      fin = from;
    }
    // the log's records, in order
    for (i64 r = t; r < n; r += SCREEN_TL) {
      const u32 j = fin[r];
      const i64 g = o0 + j;
      w.rts[o0 + r] = s.ts[g];
      w.rhi[o0 + r] = s.oid_hi[g];
      w.rlo[o0 + r] = s.oid_lo[g];
      w.ridx[o0 + r] = j;
      w.rsym[o0 + r] = s.sym[g];
      w.rv0[o0 + r] = s.v0[g];
    }
    if (t == 0) w.linfo[l] = (i32)n;
    __syncthreads();  // the next log's walk reuses sscan, ia and ib
  }
}

// LARGE (SMX_SCREEN_LARGE; linfo holds every log's true rename count): no pair gets -2; one
// whose renames together exceed SCREEN_N goes on a fourth list, large_list, for k_screen_stream.
template <bool LARGE>
__global__ void __launch_bounds__(256) k_screen_classify(ScreenArgs s, ScreenWs w, u32* large_list) {
  constexpr int PER = SCREEN_CHUNK / 256;
  constexpr int NC = SCREEN_CLASSES + (LARGE ? 1 : 0);
  __shared__ u32 c[NC], start[NC];
  const int t = threadIdx.x;
  if (t < NC) c[t] = 0;
  __syncthreads();
  const i64 p0 = (i64)blockIdx.x * SCREEN_CHUNK;
  int cls[PER];
  u32 rk[PER];
#pragma unroll
  for (int q = 0; q < PER; ++q) {
    const i64 p = p0 + q * 256 + t;
    cls[q] = -1;
    rk[q] = 0;
    if (p >= s.n_pairs) continue;
    const i64 la = s.pair_a[p], lb = s.pair_b[p];
    i64 v = -1;
    bool listed = false;
    if (la >= 0 && la < s.n_logs && lb >= 0 && lb < s.n_logs &&
        (!s.conf_off || (s.conf_off[p] >= 0 && s.conf_off[p + 1] >= s.conf_off[p]))) {
      const i32 na = w.linfo[la], nb = w.linfo[lb];
      if (na < 0 || nb < 0) v = -1;
      else if (!LARGE && (na > SCREEN_N || nb > SCREEN_N || na + nb > SCREEN_N)) v = -2;
      else if (na == 0 || nb == 0) v = 0;  // a side without renames: no conflicts, no walk
      else {
        listed = true;
        int k = 0;
        if (LARGE && (i64)na + nb > SCREEN_N) k = SCREEN_CLASSES;
        else
          while (na + nb > screen_class_cap(k)) ++k;
        cls[q] = k;
        rk[q] = atomicAdd(&c[k], 1u);
      }
    }
    if (!listed) s.counts[p] = v;
  }
  __syncthreads();
  if (t < NC) start[t] = c[t] ? atomicAdd(&w.cnt[t], c[t]) : 0u;
  __syncthreads();
#pragma unroll
  for (int q = 0; q < PER; ++q) {
    if (LARGE && cls[q] == SCREEN_CLASSES) large_list[start[SCREEN_CLASSES] + rk[q]] = (u32)(p0 + q * 256 + t);
    else if (cls[q] >= 0) w.lists[(size_t)cls[q] * w.list_stride + start[cls[q]] + rk[q]] = (u32)(p0 + q * 256 + t);
  }
}

// The body of the pair kernels, by N / 2 threads: nA sorted rename records of A from record oa
// and nB of B from record ob (0 < nA, nB; nA + nB <= N) into LDS, their ranks, and the wave
// walk from the heads (0, 0), which ends when a side is used up.  nc: the pair's conflicts so
// far, in and out (wave 0).  Whole pairs (k_screen_pairs: STREAM false) end there and store
// counts[p].  The streamed kernel (k_screen_stream: STREAM true) gives the records in chunks:
// wave 0 leaves in heads[0 .. 1] how many records of A and of B the walk consumed -- the head
// pair at which a side ran out, from which the next round starts.
template <int N, bool STREAM>
__device__ __forceinline__ void screen_pair_round(const ScreenArgs& s, const ScreenWs& w, i64 p, i64 oa, i64 ob, int nA,
                                                  int nB, i64 len_a, u32& nc, u32* heads) {
  constexpr int NT = N / 2;
  static_assert(N >= 2 * WAVE && N <= SCREEN_N && (N & (N - 1)) == 0 && N < 0x10000, "pair capacity, positions in 16 bits");
  __shared__ __attribute__((aligned(16))) u64 keys[3][N];  // by element: A's renames, then B's
  u64* kts = keys[0];
  u64* khi = keys[1];
  u64* klo = keys[2];
  __shared__ u64 sn[N];              // by T: symbol << 32 | newName class
  __shared__ i32 src[N];             // by T: the op's index in A || B
  __shared__ u16 posA[N], posB[N];   // the i-th rename of a side: its T
  __shared__ u16 iat[N + 1];         // by T: A's renames before T
  __shared__ u32 nxtA[N + 1], nxtB[N + 1];  // next rename of a side at or after T: T << 16 | index
  const int t = threadIdx.x, lane = t & (WAVE - 1), wv = t / WAVE;
  const int n = nA + nB;
  for (int e = t; e < n; e += NT) {
    const i64 g = e < nA ? oa + e : ob + (e - nA);
    kts[e] = w.rts[g];
    khi[e] = w.rhi[g];
    klo[e] = w.rlo[g];
  }
  __syncthreads();
  // T of each rename: its index in its own list + its rank in the other one
  for (int e = t; e < n; e += NT) {
    const bool sa = e < nA;
    const u64 ts = kts[e], hi = khi[e], lo = klo[e];
    int lo_i = sa ? nA : 0, hi_i = sa ? n : nA;
    const int base = lo_i;
    while (lo_i < hi_i) {  // A: B keys strictly below; B: A keys at or below (A first on ties)
      const int mid = (lo_i + hi_i) >> 1;
      const u64 mt = kts[mid], mh = khi[mid], ml = klo[mid];
      // (the tie-break, A first on equal keys, is screen_step_merge's too: smx_screen_train.h)
      const bool below = mt != ts ? mt < ts : mh != hi ? mh < hi : sa ? ml < lo : ml <= lo;
      if (below) lo_i = mid + 1;
      else hi_i = mid;
    }
    const int own = sa ? e : e - nA;
    const int T = own + (lo_i - base);
    const i64 g = sa ? oa + e : ob + own;
    sn[T] = (u64)w.rsym[g] << 32 | (u32)w.rv0[g];
    src[T] = (i32)(sa ? (i64)w.ridx[g] : len_a + (i64)w.ridx[g]);
    if (sa) {
      posA[own] = (u16)T;
      iat[T] = (u16)own;
    } else {
      posB[own] = (u16)T;
      iat[T] = (u16)(T - own);
    }
  }
  if (t == 0) iat[n] = (u16)nA;
  __syncthreads();
  for (int T = t; T <= n; T += NT) {
    const int ia = iat[T], ib = T - ia;
    nxtA[T] = (u32)(ia < nA ? posA[ia] : n) << 16 | (u32)ia;
    nxtB[T] = (u32)(ib < nB ? posB[ib] : n) << 16 | (u32)ib;
  }
  __syncthreads();
  if (wv == 0) {
    // the walk of smx_small.h step 2 (the rename block is [0, n)), without the skip marks.
    // Every loop is bounded: a pass consumes at least one rename, the scalar run-following
    // moves to a strictly later lane.
    i32* conf = s.conflicts ? s.conflicts + 2 * s.conf_off[p] : nullptr;
    const i64 cap = s.conflicts ? s.conf_off[p + 1] - s.conf_off[p] : 0;
    u32 hA = (u32)__builtin_amdgcn_readfirstlane((int)nxtA[0]);
    u32 hB = (u32)__builtin_amdgcn_readfirstlane((int)nxtB[0]);
    for (int pass = 0; pass <= n && (int)(hA & 0xffffu) < nA && (int)(hB & 0xffffu) < nB; ++pass) {
      const int pa = (int)(hA >> 16), pb = (int)(hB >> 16);
      const bool ldA = pa < pb;
      const int il = (int)((ldA ? hA : hB) & 0xffffu) + lane;
      const int cl = il < (ldA ? nA : nB) ? (int)(ldA ? posA[il] : posB[il]) : n;
      const int other = ldA ? pb : pa;
      const int g = (int)__popcll(__ballot(cl < other));
      const int q = other + lane - g;
      const int qc = q < n ? q : n;
      const u32 xA2 = nxtA[qc], xB2 = nxtB[qc];
      const u32 xl = (u32)cl << 16 | (u32)il;
      const u32 xA = lane < g ? (ldA ? xl : hA) : xA2;
      const u32 xB = lane < g ? (ldA ? hB : xl) : xB2;
      const int pA = (int)(xA >> 16), pB = (int)(xB >> 16);
      const bool valid = (int)(xA & 0xffffu) < nA && (int)(xB & 0xffffu) < nB;
      const u64 sa = sn[valid ? pA : 0], sb = sn[valid ? pB : 0];
      const u32 nA1 = nxtA[valid ? pA + 1 : n], nB1 = nxtB[valid ? pB + 1 : n];  // the heads after a conflict here
      const i32 oA = src[valid ? pA : 0], oB = src[valid ? pB : 0];
      const bool cf = valid && (sa >> 32) == (sb >> 32) && (u32)sa != (u32)sb;
      // after a conflict here, are both heads past this pair?  Then the walk goes on at the
      // merged state of position max + 1, which a later lane already holds
      const int pmax = pA > pB ? pA : pB;
      const bool jmp = (nA1 >> 16) > (u32)pmax && (nB1 >> 16) > (u32)pmax;
      const u64 cm = __ballot(cf), im = __ballot(!valid), jm = __ballot(jmp);
      const int knl = g + (pmax + 1 - other);  // the lane of position max + 1
      u64 rec = 0;  // the lanes whose pair conflicts on this pass, in walk order
      int k = 0;
      bool done = false;
      for (int it = 0; it < WAVE; ++it) {
        const u64 ge = ~0ull << k;  // (k < WAVE)
        const int jc = (cm & ge) ? __builtin_ctzll(cm & ge) : WAVE;
        const int ji = (im & ge) ? __builtin_ctzll(im & ge) : WAVE;
        if (jc < ji) {
          rec |= 1ull << jc;
          const int kn = __builtin_amdgcn_readlane(knl, jc);
          if (((jm >> jc) & 1) && kn > jc && kn < WAVE) {
            k = kn;
            continue;
          }
          hA = (u32)__builtin_amdgcn_readlane((int)nA1, jc);
          hB = (u32)__builtin_amdgcn_readlane((int)nB1, jc);
        } else if (ji < WAVE) {
          done = true;
          if constexpr (STREAM) {
            // a side ran out: the walk's state is the head pair of the first invalid lane --
            // of that lane and no other (the lane before it still compares its pair, the one
            // after it has already moved past a record)
            hA = (u32)__builtin_amdgcn_readlane((int)xA, ji);
            hB = (u32)__builtin_amdgcn_readlane((int)xB, ji);
          }
        } else {
          hA = (u32)__builtin_amdgcn_readlane((int)xA, WAVE - 1);
          hB = (u32)__builtin_amdgcn_readlane((int)xB, WAVE - 1);
        }
        break;
      }
      if ((rec >> lane) & 1) {  // the pass's conflicts, each by its own lane
        const u32 ci = nc + (u32)__popcll(rec & lanemask_lt());
        if ((i64)ci < cap) {
          conf[2 * ci] = oA;
          conf[2 * ci + 1] = oB;
        }
      }
      nc += (u32)__popcll(rec);
      if (done) break;
    }
    if constexpr (STREAM) {
      // (the loop also ends with a head past its chunk after a conflict or a lane-63 hand-over)
      if (lane == 0) {
        heads[0] = hA & 0xffffu;
        heads[1] = hB & 0xffffu;
      }
    } else {
      if (lane == 0) s.counts[p] = (i64)nc;
    }
  }
}

// Pairs of at most N renames (a power of two, 128 .. SCREEN_N) by N / 2 threads.
template <int N>
__global__ void __launch_bounds__(N / 2) k_screen_pairs(ScreenArgs s, ScreenWs w, const u32* cnt, const u32* list) {
  const u32 c = *cnt;
  for (u32 i = blockIdx.x; i < c; i += gridDim.x) {
    const i64 p = (i64)list[i];
    const i64 la = s.pair_a[p], lb = s.pair_b[p];
    const i64 oa = s.log_off[la], ob = s.log_off[lb];
    const i64 len_a = s.log_off[la + 1] - oa;
    const int nA = w.linfo[la], nB = w.linfo[lb];  // (classified: 0 < nA, nB; nA + nB <= N)
    u32 nc = 0;
    screen_pair_round<N, false>(s, w, p, oa, ob, nA, nB, len_a, nc, nullptr);
    __syncthreads();  // the next pair's load overwrites what this one's walk reads
  }
}

// Pairs of more than SCREEN_N renames (SMX_SCREEN_LARGE), streamed: one workgroup of
// SCREEN_N / 2 threads per pair keeps the two global heads (iA, iB) and repeats a round of
// screen_pair_round on the next SCREEN_N / 2 records of each side from its head.  While both
// heads lie inside their chunks, the chunks' merged order and the walk's comparisons are those
// of the whole pair; the round stops where a chunk is used up, and the heads there start the
// next round.  Every round consumes a whole chunk of one side or ends the pair, which bounds
// the rounds by ceil(RA / chunk) + ceil(RB / chunk).  The conflict count runs across rounds.
__global__ void __launch_bounds__(SCREEN_N / 2) k_screen_stream(ScreenArgs s, ScreenWs w, const u32* cnt,
                                                                const u32* list) {
  constexpr i64 CH = SCREEN_N / 2;
  __shared__ u32 heads[2];
  const u32 c = *cnt;
  for (u32 i = blockIdx.x; i < c; i += gridDim.x) {
    const i64 p = (i64)list[i];
    const i64 la = s.pair_a[p], lb = s.pair_b[p];
    const i64 oa = s.log_off[la], ob = s.log_off[lb];
    const i64 len_a = s.log_off[la + 1] - oa;
    const i64 RA = w.linfo[la], RB = w.linfo[lb];  // (classified: 0 < RA, RB)
    const i64 rounds = SMX_CEIL_DIV(RA, CH) + SMX_CEIL_DIV(RB, CH);
    i64 iA = 0, iB = 0;
    u32 nc = 0;
    for (i64 r = 0; r < rounds; ++r) {
      const int nA = (int)(RA - iA < CH ? RA - iA : CH), nB = (int)(RB - iB < CH ? RB - iB : CH);
      screen_pair_round<SCREEN_N, true>(s, w, p, oa + iA, ob + iB, nA, nB, len_a, nc, heads);
      __syncthreads();  // the heads; and the next round's load overwrites what this walk reads
      iA += heads[0];
      iB += heads[1];
      if (iA >= RA || iB >= RB) break;  // (uniform) a side is used up for good: the pair is done
    }
    if (threadIdx.x == 0) s.counts[p] = (i64)nc;
    // (the next write of heads[] comes after the barriers of the next round's load)
  }
}
