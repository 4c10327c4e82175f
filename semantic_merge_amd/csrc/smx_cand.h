// smx_cand.h — the candidate pairs of many logs for the conflict screen
// (smx_screen_candidates): which pairs (i, j), i < j, share a symbol that both rename to
// different names.  A DivergentRename needs exactly that (compose.py:60-70, 88-98), so every
// other pair has no conflicts in either orientation and need not be screened.
//
//   k_cand_logs      one workgroup: every log's bounds (screen_log_bounds, smx_screen.h's
//                    prefix-maximum rule: valid logs never overlap), and clears the counts
//   k_cand_records   one workgroup per log, two walks of its kind bytes: the first counts
//                    the renames and looks for kind >= 18 (the verdict), the second, for a
//                    valid log only, writes one record per rename at the op's own slot of
//                    [0, n_total): key sym << b | log (b = ceil(log2 n_logs)), value v0.
//                    Every other slot keeps the sentinel key the call filled the array with,
//                    so an invalid log leaves no record and the sort length is n_total
//   radix_sort_pairs (smx_sort.h) on the 33 + b key bits: the sentinel has bit 32 + b set
//                    and sorts after every record
//   k_cand_heads     flags the first record of every (sym, log) run; a scan (smx_scan.h)
//                    numbers them and counts them on the device
//   k_cand_entries   per run head: the run's smallest and largest v0 (as u32), compacted
//                    with its key.  Entries of one symbol are adjacent, in log order
//   k_cand_pairs     a wave per entry, lanes striding over the later entries of its symbol:
//                    two entries are a candidate unless both runs hold one class and the
//                    classes are equal (i.e. some v0 of one differs from some v0 of the
//                    other); sets bit i * n_logs + j of the bit matrix with atomicOr.  A
//                    symbol renamed in g logs costs g (g - 1) / 2 bit sets
//   k_cand_popc      popcounts of the matrix words; a scan gives every word's first output
//   k_cand_emit      the set bits in index order -- ascending (i, j) -- up to pair_cap, and
//                    counts[0]
// Nothing here waits, allocates or reads back; the number of launches depends on n_logs
// alone (the sort's passes).  The entry point is in smx_batch.hip.
#pragma once

#include "smx_screen.h"
#include "smx_sort.h"

typedef struct smx_candidates CandArgs;

#define CAND_HDR 256            // workspace: n_ent, n_cand (u32)
#define CAND_NONE (~0ull)       // the key of a slot that holds no record
#define CAND_PAIR_BLOCKS 2048   // k_cand_pairs: at most this many workgroups of BLOCK threads

static inline int cand_log_bits(int64_t n_logs) {
  int b = 0;
  while (((int64_t)1 << b) < n_logs) ++b;
  return b;
}
static inline size_t cand_words(int64_t n_logs) { return (size_t)(((u64)n_logs * (u64)n_logs + 31) / 32); }

struct CandWs {
  u32* n_ent;    // entries (runs of one symbol in one log), device-held
  u32* n_cand;   // candidates
  i32* linfo;    // [n_logs] -1 or the log's renames
  u64 *keys, *k2;   // [n_total] the records' keys; after the sort k2 holds the entries' keys
  u32 *vals, *v2;   // [n_total] v0; after the sort v2 holds the entry numbers
  u32* flag;        // [n_total] run heads
  u64* emm;         // [n_total] per entry: largest v0 << 32 | smallest v0
  u32* hist;        // the sort's histograms
  u32* partials;    // [SCAN_NB]
  u32 *mat, *pop, *wpos;  // [cand_words] the bit matrix, its popcounts, their prefix
  size_t n_words;
};
static inline size_t cand_ws_bytes(int64_t n_logs, int64_t n_total) {
  return CAND_HDR + screen_al((size_t)n_logs * 4) + 3 * screen_al((size_t)n_total * 8) +
         3 * screen_al((size_t)n_total * 4) + screen_al(radix_hist_bytes(n_total)) + screen_al(SCAN_NB * 4) +
         3 * screen_al(cand_words(n_logs) * 4);
}
static inline CandWs cand_ws(void* workspace, int64_t n_logs, int64_t n_total) {
  char* p = (char*)workspace;
  CandWs w;
  w.n_ent = (u32*)p;
  w.n_cand = (u32*)p + 1;
  p += CAND_HDR;
  w.linfo = (i32*)p;
  p += screen_al((size_t)n_logs * 4);
  const size_t q8 = screen_al((size_t)n_total * 8), q4 = screen_al((size_t)n_total * 4);
  w.keys = (u64*)p;
  w.k2 = (u64*)(p + q8);
  w.emm = (u64*)(p + 2 * q8);
  p += 3 * q8;
  w.vals = (u32*)p;
  w.v2 = (u32*)(p + q4);
  w.flag = (u32*)(p + 2 * q4);
  p += 3 * q4;
  w.hist = (u32*)p;
  p += screen_al(radix_hist_bytes(n_total));
  w.partials = (u32*)p;
  p += screen_al(SCAN_NB * 4);
  w.n_words = cand_words(n_logs);
  const size_t qm = screen_al(w.n_words * 4);
  w.mat = (u32*)p;
  w.pop = (u32*)(p + qm);
  w.wpos = (u32*)(p + 2 * qm);
  return w;
}

__global__ void __launch_bounds__(1024) k_cand_logs(CandArgs c, CandWs w) {
  __shared__ i64 sc[1024 / WAVE + 1];
  if (threadIdx.x == 0) {
    c.counts[0] = 0;
    c.counts[1] = 0;
    *w.n_ent = 0;
    *w.n_cand = 0;
  }
  screen_log_bounds(c.log_off, c.n_logs, c.n_total, w.linfo, sc);
}

__global__ void __launch_bounds__(BLOCK) k_cand_records(CandArgs c, CandWs w, int bits) {
  __shared__ u32 s_cnt;
  const int t = threadIdx.x;
  for (i64 l = blockIdx.x; l < c.n_logs; l += gridDim.x) {
    if (t == 0) s_cnt = 0;
    __syncthreads();
    bool ok = w.linfo[l] >= 0;  // (uniform: one word for the workgroup)
    i64 o0 = 0, len = 0;
    if (ok) {
      o0 = c.log_off[l];
      len = c.log_off[l + 1] - o0;  // (valid bounds: 0 <= o0, o0 + len <= n_total)
      u32 cnt = 0, bad = 0;
      for (i64 j = t; j < len; j += BLOCK) {
        const u32 k = c.kind[o0 + j];
        bad |= k >= SMX_N_KINDS;
        cnt += k == SMX_KIND_RENAME;
      }
      if (cnt) atomicAdd(&s_cnt, cnt);
      ok = !__syncthreads_or(bad);  // (also: s_cnt is complete)
    }
    if (ok) {  // the verdict is in: the log's records, each at its op's own slot
      for (i64 j = t; j < len; j += BLOCK) {
        if (c.kind[o0 + j] == SMX_KIND_RENAME) {
          w.keys[o0 + j] = (u64)c.sym[o0 + j] << bits | (u64)l;
          w.vals[o0 + j] = (u32)c.v0[o0 + j];
        }
      }
    }
    if (t == 0) {
      const i32 info = ok ? (i32)s_cnt : -1;  // (len <= n_total < 2^31)
      w.linfo[l] = info;
      if (c.log_info) c.log_info[l] = info;
      if (!ok) atomicAdd((unsigned long long*)&c.counts[1], 1ull);
    }
    __syncthreads();  // the next log clears s_cnt
  }
}

__global__ void __launch_bounds__(BLOCK) k_cand_heads(CandWs w, i64 n) {
  for (i64 p = (i64)blockIdx.x * BLOCK + threadIdx.x; p < n; p += (i64)gridDim.x * BLOCK) {
    const u64 k = w.keys[p];
    w.flag[p] = k != CAND_NONE && (p == 0 || w.keys[p - 1] != k);
  }
}

// (after the scan: v2[p] = run heads before p, *n_ent = all of them)
__global__ void __launch_bounds__(BLOCK) k_cand_entries(CandWs w, i64 n) {
  for (i64 p = (i64)blockIdx.x * BLOCK + threadIdx.x; p < n; p += (i64)gridDim.x * BLOCK) {
    if (!w.flag[p]) continue;
    const u64 k = w.keys[p];
    u32 lo = w.vals[p], hi = lo;
    for (i64 q = p + 1; q < n && w.keys[q] == k; ++q) {  // the run: this symbol's renames in this log
      const u32 v = w.vals[q];
      lo = v < lo ? v : lo;
      hi = v > hi ? v : hi;
    }
    const u32 e = w.v2[p];  // (e < n_ent <= n)
    w.k2[e] = k;
    w.emm[e] = (u64)hi << 32 | lo;
  }
}

__global__ void __launch_bounds__(BLOCK) k_cand_pairs(CandArgs c, CandWs w, int bits) {
  const int lane = threadIdx.x & (WAVE - 1);
  const u32 n_ent = *w.n_ent;
  const u64 lmask = ((u64)1 << bits) - 1;
  const u32 nw = gridDim.x * NWAVES;
  for (u32 e = blockIdx.x * NWAVES + threadIdx.x / WAVE; e < n_ent; e += nw) {  // (wave-uniform)
    const u64 ke = w.k2[e], me = w.emm[e];
    const u64 sym = ke >> bits, i = ke & lmask;
    const bool single = (u32)(me >> 32) == (u32)me;
    // the later entries of this symbol, which follow it in log order (j > i); bounded by n_ent
    for (u32 f0 = e + 1; f0 < n_ent; f0 += WAVE) {
      const u32 f = f0 + lane;
      bool in = f < n_ent;
      if (in) {
        const u64 kf = w.k2[f];
        in = (kf >> bits) == sym;
        if (in) {
          const u64 mf = w.emm[f];
          if (!(single && mf == me)) {  // not: one class on each side, and the same one
            const u64 idx = i * (u64)c.n_logs + (kf & lmask);  // (i, j < n_logs)
            atomicOr(&w.mat[idx >> 5], 1u << (idx & 31));
          }
        }
      }
      if (__ballot(in) != ~0ull) break;  // the symbol's group ends in this stride
    }
  }
}

__global__ void __launch_bounds__(BLOCK) k_cand_popc(CandWs w) {
  for (size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; i < w.n_words; i += (size_t)gridDim.x * BLOCK)
    w.pop[i] = (u32)__popc(w.mat[i]);
}

__global__ void __launch_bounds__(BLOCK) k_cand_emit(CandArgs c, CandWs w) {
  if (blockIdx.x == 0 && threadIdx.x == 0) c.counts[0] = (i64)*w.n_cand;
  for (size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; i < w.n_words; i += (size_t)gridDim.x * BLOCK) {
    u32 m = w.mat[i];
    i64 k = (i64)w.wpos[i];
    while (m && k < c.pair_cap) {  // the word's pairs in bit order: ascending (i, j)
      const u64 idx = (u64)i * 32 + (u32)__builtin_ctz(m);
      c.pair_a[k] = (i32)(idx / (u64)c.n_logs);
      c.pair_b[k] = (i32)(idx % (u64)c.n_logs);
      m &= m - 1;
      ++k;
    }
  }
}
