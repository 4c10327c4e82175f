// smx_batch_large.h — merges of more than SMALL_N ops inside a batch (SMX_BATCH_LARGE of
// smx_compose_batch_ex / smx_compose_batch_shared_ex).
//
// compose_small holds a whole merge in LDS, which is where the batch's limit of SMALL_N ops
// came from; nothing in the reference's loop needs it.  Here one 1024-thread workgroup runs
// the four steps of smx_small.h's header comment on a merge of any length through global
// memory, in the merge's own slice of the workspace (LARGE_OP_BYTES per op of the batch, at
// the offset of the merge's results: no per-workgroup slots, no length cap):
//   1. T: tiles of LARGE_TILE op indices sorted in LDS by a bitonic sort on the full key
//      (kind, ts, oid_hi, oid_lo, index in A||B -- A's indices lie below B's, so the index
//      stands for (side, index)), then merge levels that double the runs between the two
//      index arrays ia / ib, every thread LARGE_MERGE outputs at a time from its merge-path
//      split, the keys read from the columns through the index (smx_screen.h's
//      k_screen_extract_large is the model).  The key is a total order (the index is unique),
//      so T does not depend on how the merge is cut into tiles;
//   2. the walk over the rename block of T in rounds of up to LARGE_CH renames per side from
//      the two global heads (smx_screen.h's screen_pair_round<.., true>: a round ends where a
//      side's chunk is used up and the next starts at those heads).  T is global, so a round
//      merges its two chunks by comparing T, not keys.  Every conflict marks both T positions
//      as skipped, whatever the conflict capacity is;
//   3. the chains in an exact open-addressing table on the full 32-bit symbol, 2 slots per
//      move or rename of the merge, in the slice: the last non-None move address and file
//      writer and the last kept rename (atomic max of T + 1); a move with a None value gets
//      its symbol's inclusive prefix from one wave that walks the move block in T order, 64
//      moves a step, only when some move has a None value (smx_small.h phase 3);
//   4. emit: every op of T that is not skipped, at T minus the skips before it.
// Invalid input (kind >= 18, sym >= n_sym anywhere in the merge) is found by a first pass over
// the merge's columns, before the first output store: counts -1 and nothing else.
//
// Workspace arrays of the slice (entries of the merge at [wb, wb + n), tables at [2 wb, ..)):
//   ia, ib   the sort's two index arrays; the one that does not end up as T holds each
//            move's and rename's table slot afterwards
//   xy       by T: x = a rename the walk skipped, or T' + 1 of a move's prefix address writer;
//            y = T' + 1 of a move's prefix file writer
//   tab      the table, by slot: symbol, last address / file writer, last kept rename
//   run      the i-th rename of A and of B: its T (until the walk ends); then, by slot, the
//            running writers of the None-valued moves' walk
#pragma once

#include "smx_batch.h"

#define LARGE_NT 1024
#define LARGE_TILE 2048  // op indices per tile of the sort
#define LARGE_CH 1024    // renames per side and round of the walk
#define LARGE_MERGE 8    // outputs per thread and step of the merge levels
#define LARGE_OP_BYTES 64  // workspace per op of the batch: ia, ib 4 each, xy 8, tab 2 x 16, run 2 x 8
static_assert(LARGE_TILE % LARGE_MERGE == 0, "a thread's outputs lie in one pair of runs");
static_assert(LARGE_TILE == 2 * LARGE_NT && LARGE_CH == LARGE_NT && LARGE_TILE < 0x10000, "two elements per thread, positions in 16 bits");

struct LargeXY {  // by T
  u32 x, y;
};
struct LargeSlot {  // a symbol's table entry: T + 1 of its last address / file writer and kept rename (0: none)
  u32 key, wa, wf, wr;
};
struct LargeRun {  // by slot: the running address / file writers of the None-valued moves' walk
  u32 a, f;
};
struct BatchLargeWs {
  u32* list;  // [n_merges] the merges over SMALL_N ops (their number: cnt[BATCH_CLASSES])
  u32 *ia, *ib;    // [n_ops]
  LargeXY* xy;     // [n_ops]
  LargeSlot* tab;  // [2 * n_ops]
  LargeRun* run;   // [2 * n_ops]
};
static inline size_t batch_al(size_t x) { return (x + 255) & ~(size_t)255; }
// What SMX_BATCH_LARGE adds behind the unflagged workspace, for result arrays of n_ops entries.
static inline size_t batch_large_bytes(int64_t n_merges, int64_t n_ops) {
  return batch_list_bytes(n_merges) + 2 * batch_al((size_t)n_ops * 4) + batch_al((size_t)n_ops * 8) +
         batch_al((size_t)n_ops * 32) + batch_al((size_t)n_ops * 16);
}
static inline BatchLargeWs batch_large_ws(void* at, int64_t n_merges, int64_t n_ops) {
  char* p = (char*)at;
  const size_t q4 = batch_al((size_t)n_ops * 4);
  BatchLargeWs w;
  w.list = (u32*)p;
  p += batch_list_bytes(n_merges);
  w.ia = (u32*)p;
  w.ib = (u32*)(p + q4);
  p += 2 * q4;
  w.xy = (LargeXY*)p;
  p += batch_al((size_t)n_ops * 8);
  w.tab = (LargeSlot*)p;
  p += batch_al((size_t)n_ops * 32);
  w.run = (LargeRun*)p;
  return w;
}

// Where merge m's slice of the workspace starts: where its results do.
__device__ __forceinline__ i64 batch_slice(const smx_batch& b, i64 m) { return b.off[m]; }
__device__ __forceinline__ i64 batch_slice(const smx_batch_shared& b, i64 m) { return b.off[m] + (m - 1) * b.n_shared; }
__device__ __forceinline__ i64 batch_slice(const smx_pairs& b, i64 m) { return b.res_off[m]; }

// The LDS of the sort's tiles and of the walk's rounds, one after the other.
struct LargeSortLds {
  u64 kts[LARGE_TILE], khi[LARGE_TILE], klo[LARGE_TILE];
  u16 ord[LARGE_TILE];
  u8 skd[LARGE_TILE];
};
struct LargeWalkLds {
  u64 sn[LARGE_TILE];                             // by round position: symbol << 32 | newName class
  u32 src[LARGE_TILE];                            // by round position: the op's index in A || B
  u32 gT[LARGE_TILE];                             // by round position: its T
  u32 nxtA[LARGE_TILE + 1], nxtB[LARGE_TILE + 1];  // next rename of a side at or after a position: position << 16 | index
  u32 cT[2][LARGE_CH];                            // the chunks: T of A's and of B's renames from the heads
  u16 posA[LARGE_TILE], posB[LARGE_TILE];         // the i-th rename of a side's chunk: its round position
  u16 iat[LARGE_TILE + 2];                        // by round position: A's renames before it
};
union LargeLds {
  LargeSortLds s;
  LargeWalkLds w;
};

// An op of A||B with its sort key, read from the columns (B op e at e + b_gap, in 64 bits).
struct LargeKey {
  u64 ts, hi, lo;
  u32 k, e;
};
__device__ __forceinline__ i64 large_col(const smx_ops& o, i64 e) { return e < o.n_a ? e : e + o.b_gap; }
__device__ __forceinline__ LargeKey large_key(const smx_ops& o, u32 e) {
  const i64 j = large_col(o, (i64)e);
  return LargeKey{o.ts[j], o.oid_hi[j], o.oid_lo[j], (u32)o.kind[j], e};
}
__device__ __forceinline__ bool large_key_lt(const LargeKey& x, const LargeKey& y) {
  if (x.k != y.k) return x.k < y.k;
  if (x.ts != y.ts) return x.ts < y.ts;
  if (x.hi != y.hi) return x.hi < y.hi;
  if (x.lo != y.lo) return x.lo < y.lo;
  return x.e < y.e;  // (side, index): A's indices lie below B's
}

// screen_sort_tile with the kind in front: a bitonic sort of S.ord (the positions 0 .. n - 1
// of the tile on entry, which are in (side, index) order) on (kind, ts, id, position); slots
// past n sort last.  Ends with a barrier.
__device__ __forceinline__ void large_sort_tile(LargeSortLds& S, int n) {
  const int t = threadIdx.x;
  auto less = [&](u32 x, u32 y) -> bool {  // x before y (x != y)
    if ((int)x >= n || (int)y >= n) return (int)y >= n && (int)x < n;
    if (S.skd[x] != S.skd[y]) return S.skd[x] < S.skd[y];
    if (S.kts[x] != S.kts[y]) return S.kts[x] < S.kts[y];
    if (S.khi[x] != S.khi[y]) return S.khi[x] < S.khi[y];
    if (S.klo[x] != S.klo[y]) return S.klo[x] < S.klo[y];
    return x < y;
  };
  int P = 1;
  while (P < n) P <<= 1;
  for (int r = n + t; r < P; r += LARGE_NT) S.ord[r] = (u16)r;
  __syncthreads();
  for (int k = 2; k <= P; k <<= 1) {
    for (int jj = k >> 1; jj > 0; jj >>= 1) {
      for (int a = t; a < P; a += LARGE_NT) {
        const int b = a ^ jj;
        if (b > a) {
          const u32 x = S.ord[a], y = S.ord[b];
          const bool up = (a & k) == 0;
          if (up ? less(y, x) : less(x, y)) {
            S.ord[a] = (u16)y;
            S.ord[b] = (u16)x;
          }
        }
      }
      __syncthreads();
    }
  }
}

// One round of the walk (screen_pair_round<.., true> on T instead of keys): cA renames of A
// from posA and cB of B from posB (0 < cA, cB <= LARGE_CH; their T, ascending), merged by T
// into round positions, and the wave walk from the chunks' heads, which ends when a side's
// chunk is used up.  A conflict is recorded while the capacity lasts and always marks both T
// as skipped in xy.  nc: the merge's conflicts so far, in and out (wave 0); heads[0 .. 1]:
// how many renames of A and of B the round consumed.
__device__ __forceinline__ void large_walk_round(const smx_ops& ops, const smx_compose_out& out, const u32* ord,
                                                 const u32* posA, const u32* posB, int cA, int cB, LargeXY* xy,
                                                 LargeWalkLds& W, u32& nc, u32* heads) {
  const int t = threadIdx.x, lane = t & (WAVE - 1), wv = t / WAVE;
  const int n = cA + cB;
  if (t < cA) W.cT[0][t] = posA[t];
  if (t < cB) W.cT[1][t] = posB[t];
  __syncthreads();
  for (int e = t; e < n; e += LARGE_NT) {
    const bool sa = e < cA;
    const int own = sa ? e : e - cA;
    const u32 myT = W.cT[sa ? 0 : 1][own];
    const u32* oth = W.cT[sa ? 1 : 0];
    int lo = 0, hi = sa ? cB : cA;
    while (lo < hi) {  // the other chunk's renames before this one (every T is another)
      const int mid = (lo + hi) >> 1;
      if (oth[mid] < myT) lo = mid + 1;
      else hi = mid;
    }
    const int T = own + lo;
    const u32 el = ord[myT];
    const i64 j = large_col(ops, (i64)el);
    W.sn[T] = (u64)ops.sym[j] << 32 | (u32)ops.v0[j];
    W.src[T] = el;
    W.gT[T] = myT;
    if (sa) {
      W.posA[own] = (u16)T;
      W.iat[T] = (u16)own;
    } else {
      W.posB[own] = (u16)T;
      W.iat[T] = (u16)(T - own);
    }
  }
  if (t == 0) W.iat[n] = (u16)cA;
  __syncthreads();
  for (int T = t; T <= n; T += LARGE_NT) {
    const int ia = W.iat[T], ib = T - ia;
    W.nxtA[T] = (u32)(ia < cA ? W.posA[ia] : n) << 16 | (u32)ia;
    W.nxtB[T] = (u32)(ib < cB ? W.posB[ib] : n) << 16 | (u32)ib;
  }
  __syncthreads();
  if (wv == 0) {
    // the walk of smx_small.h step 2 (the rename block is [0, n)).  Every loop is bounded: a
    // pass consumes at least one rename, the scalar run-following moves to a strictly later lane.
    u32 hA = (u32)__builtin_amdgcn_readfirstlane((int)W.nxtA[0]);
    u32 hB = (u32)__builtin_amdgcn_readfirstlane((int)W.nxtB[0]);
    for (int pass = 0; pass <= n && (int)(hA & 0xffffu) < cA && (int)(hB & 0xffffu) < cB; ++pass) {
      const int pa = (int)(hA >> 16), pb = (int)(hB >> 16);
      const bool ldA = pa < pb;
      const int il = (int)((ldA ? hA : hB) & 0xffffu) + lane;
      const int cl = il < (ldA ? cA : cB) ? (int)(ldA ? W.posA[il] : W.posB[il]) : n;
      const int other = ldA ? pb : pa;
      const int g = (int)__popcll(__ballot(cl < other));
      const int q = other + lane - g;
      const int qc = q < n ? q : n;
      const u32 xA2 = W.nxtA[qc], xB2 = W.nxtB[qc];
      const u32 xl = (u32)cl << 16 | (u32)il;
      const u32 xA = lane < g ? (ldA ? xl : hA) : xA2;
      const u32 xB = lane < g ? (ldA ? hB : xl) : xB2;
      const int pA = (int)(xA >> 16), pB = (int)(xB >> 16);
      const bool valid = (int)(xA & 0xffffu) < cA && (int)(xB & 0xffffu) < cB;
      const u64 sa = W.sn[valid ? pA : 0], sb = W.sn[valid ? pB : 0];
      const u32 nA1 = W.nxtA[valid ? pA + 1 : n], nB1 = W.nxtB[valid ? pB + 1 : n];  // the heads after a conflict here
      const u32 oA = W.src[valid ? pA : 0], oB = W.src[valid ? pB : 0];
      const u32 tA = W.gT[valid ? pA : 0], tB = W.gT[valid ? pB : 0];
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
          // a side's chunk ran out: the walk's state is the head pair of the first invalid lane
          done = true;
          hA = (u32)__builtin_amdgcn_readlane((int)xA, ji);
          hB = (u32)__builtin_amdgcn_readlane((int)xB, ji);
        } else {
          hA = (u32)__builtin_amdgcn_readlane((int)xA, WAVE - 1);
          hB = (u32)__builtin_amdgcn_readlane((int)xB, WAVE - 1);
        }
        break;
      }
      if ((rec >> lane) & 1) {  // the pass's conflicts, each by its own lane
        const u32 ci = nc + (u32)__popcll(rec & lanemask_lt());
        if ((i64)ci < out.conflict_cap) {
          out.conflicts[2 * (i64)ci] = (i32)oA;
          out.conflicts[2 * (i64)ci + 1] = (i32)oB;
        }
        xy[tA].x = 1u;
        xy[tB].x = 1u;
      }
      nc += (u32)__popcll(rec);
      if (done) break;
    }
    if (lane == 0) {
      heads[0] = hA & 0xffffu;
      heads[1] = hB & 0xffffu;
    }
  }
}

// One merge of more than SMALL_N ops (any length up to 2^31 - 1) by the LARGE_NT threads of
// the calling workgroup, in the workspace slice that starts at entry wb.  The kernel puts a
// barrier between two merges: every piece of LDS and workspace state is set up inside the call.
__device__ __forceinline__ void compose_large(const smx_ops& ops, const smx_compose_out& out, const BatchLargeWs& w,
                                              i64 wb) {
  constexpr int NT = LARGE_NT, NW = NT / WAVE;
  __shared__ __attribute__((aligned(16))) LargeLds L;
  __shared__ u32 sscan[NW + 1];
  __shared__ u32 sinfo[4];  // [0] moves, [1] moves and renames
  __shared__ u32 heads[2];
  const int t = threadIdx.x, lane = t & (WAVE - 1), wv = t / WAVE;
  const u32 na = (u32)ops.n_a, n = (u32)(ops.n_a + ops.n_b);  // (n <= 2^31 - 1: positions and indices in 32 bits)
  u32* ia = w.ia + wb;
  u32* ib = w.ib + wb;
  LargeXY* xy = w.xy + wb;
  LargeSlot* tab = w.tab + 2 * wb;
  LargeRun* run = w.run + 2 * wb;
  if (t < 4) sinfo[t] = 0;
  __syncthreads();
  // 0. every kind and symbol of the merge, before anything is written for it; the blocks' sizes
  {
    u32 bad = 0, cm = 0, cr = 0;
    for (u32 e = t; e < n; e += NT) {
      const i64 j = large_col(ops, (i64)e);
      const u32 k = ops.kind[j], s = ops.sym[j];
      bad |= (k >= SMX_N_KINDS) | (s >= (u64)ops.n_sym);
      cm += k <= SMX_KIND_MOVE;
      cr += k <= SMX_KIND_RENAME;
    }
    if (cm) atomicAdd(&sinfo[0], cm);
    if (cr) atomicAdd(&sinfo[1], cr);
    if (__syncthreads_or(bad)) {
      if (t == 0) {
        out.counts[0] = -1;
        out.counts[1] = -1;
      }
      return;
    }
  }
  const u32 nmv = sinfo[0], rend = sinfo[1];  // the move block [0, nmv), the rename block [nmv, rend)
  // 1. T: tiles in LDS into ib ...
  for (u32 b0 = 0; b0 < n; b0 += LARGE_TILE) {
    const int m = (int)(n - b0 < LARGE_TILE ? n - b0 : LARGE_TILE);
    for (int r = t; r < m; r += NT) {
      const i64 j = large_col(ops, (i64)(b0 + r));
      L.s.kts[r] = ops.ts[j];
      L.s.khi[r] = ops.oid_hi[j];
      L.s.klo[r] = ops.oid_lo[j];
      L.s.skd[r] = ops.kind[j];
      L.s.ord[r] = (u16)r;
    }
    large_sort_tile(L.s, m);
    for (int r = t; r < m; r += NT) ib[b0 + r] = (u32)(b0 + L.s.ord[r]);
    __syncthreads();  // the next tile's load overwrites what this one's last phase reads
  }
  // ... then merge levels that double the runs, ib -> ia -> ib ...
  u32* from = ib;
  u32* to = ia;
  for (u32 rl = LARGE_TILE; rl < n; rl *= 2) {  // (a0 + 2 rl < 2^31 + 2^31: no overflow)
    // outputs [d0, e) of the run pair [a0, a1) [a1, b1): LARGE_MERGE divides LARGE_TILE, so
    // they lie in one pair
    for (u32 d0 = (u32)t * LARGE_MERGE; d0 < n; d0 += NT * LARGE_MERGE) {
      const u32 a0 = d0 & ~(2 * rl - 1);  // (rl is a power of two)
      const u32 a1 = a0 + rl < n ? a0 + rl : n, b1 = a0 + 2 * rl < n ? a0 + 2 * rl : n;
      const u32 ra = a1 - a0, rb = b1 - a1, d = d0 - a0;
      const u32 e = d0 + LARGE_MERGE < b1 ? d0 + LARGE_MERGE : b1;
      // the first run's elements among the pair's first d outputs
      u32 lo = d > rb ? d - rb : 0, hi = d < ra ? d : ra;
      while (lo < hi) {
        const u32 mid = (lo + hi) >> 1;
        if (large_key_lt(large_key(ops, from[a1 + d - 1 - mid]), large_key(ops, from[a0 + mid]))) hi = mid;
        else lo = mid + 1;
      }
      u32 i = lo, k = d - lo;
      LargeKey ka = i < ra ? large_key(ops, from[a0 + i]) : LargeKey{0, 0, 0, 0, 0};
      LargeKey kb = k < rb ? large_key(ops, from[a1 + k]) : LargeKey{0, 0, 0, 0, 0};
      for (u32 o = d0; o < e; ++o) {
        if (i < ra && (k >= rb || !large_key_lt(kb, ka))) {
          to[o] = ka.e;
          if (++i < ra) ka = large_key(ops, from[a0 + i]);
        } else {
          to[o] = kb.e;
          if (++k < rb) kb = large_key(ops, from[a1 + k]);
        }
      }
    }
    __syncthreads();  // the level is complete before the next one reads it
    u32* const sw = from;
    from = to;
    to = sw;
  }
  const u32* ord = from;  // T -> the op's index in A || B
  u32* slot = to;         // by T < rend: the op's table slot (step 3)
  // 2. the rename lists of the two sides, in T order; x and y start clear
  u32* posA = reinterpret_cast<u32*>(run);  // (4 n words: dead before the running writers)
  u32* posB = posA + n;
  u32 n_ren_a = 0;
  for (u32 base = nmv; base < rend; base += NT) {
    const u32 T = base + t;
    const u32 isa = T < rend && ord[T] < na;
    u32 tot;
    const u32 ra = n_ren_a + block_excl_scan<OpSum, u32, NW>(isa, sscan, &tot);  // (syncs)
    if (T < rend) {
      if (isa) posA[ra] = T;
      else posB[T - nmv - ra] = T;
    }
    n_ren_a += tot;
  }
  for (u32 T = t; T < n; T += NT) xy[T] = LargeXY{0u, 0u};
  __syncthreads();
  const u32 nA = n_ren_a, nB = rend - nmv - nA;
  u32 nc = 0;
  if (nA > 0 && nB > 0) {
    // every round uses up a whole chunk of one side or ends the walk
    const u32 rounds = SMX_CEIL_DIV(nA, (u32)LARGE_CH) + SMX_CEIL_DIV(nB, (u32)LARGE_CH);
    u32 iA = 0, iB = 0;
    for (u32 r = 0; r < rounds; ++r) {
      const int cA = (int)(nA - iA < LARGE_CH ? nA - iA : LARGE_CH), cB = (int)(nB - iB < LARGE_CH ? nB - iB : LARGE_CH);
      large_walk_round(ops, out, ord, posA + iA, posB + iB, cA, cB, xy, L.w, nc, heads);
      __syncthreads();  // the heads and the skip marks; the next round's load overwrites what this walk reads
      iA += heads[0];
      iB += heads[1];
      if (iA >= nA || iB >= nB) break;  // (uniform) a side is used up for good
    }
  }
  if (t == 0) {
    out.counts[0] = (i64)n - 2 * (i64)nc;
    out.counts[1] = (i64)nc;
  }
  // 3. the chains: an open-addressing table of 2 slots per move or rename (posA / posB are dead)
  const u32 HT = 2 * rend;  // (rend <= 2^31 - 1)
  auto home = [&](u32 s) -> u32 { return (u32)(((u64)(s * 2654435761u) * (u64)HT) >> 32); };
  bool none_here = false;
  if (rend > 0) {
    for (u32 i = t; i < HT; i += NT) {  // (HT + NT < 2^32)
      tab[i] = LargeSlot{SMALL_EMPTY, 0u, 0u, 0u};  // (no symbol: sym < n_sym <= 2^32 - 1)
    }
    __syncthreads();
    for (u32 T = t; T < rend; T += NT) {
      const u32 s = ops.sym[large_col(ops, (i64)ord[T])];
      u32 h = home(s);
      for (u32 probe = 0; probe < HT; ++probe) {  // (at most rend symbols in 2 rend slots: a slot is found)
        const u32 cur = __hip_atomic_load(&tab[h].key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (cur == s) break;
        if (cur == SMALL_EMPTY) {
          const u32 old = atomicCAS(&tab[h].key, SMALL_EMPTY, s);
          if (old == SMALL_EMPTY || old == s) break;
        }
        h = h + 1 == HT ? 0u : h + 1;
      }
      slot[T] = h;
    }
    __syncthreads();
    // last writers: T + 1 (0: none)
    for (u32 T = t; T < rend; T += NT) {
      const u32 h = slot[T];
      if (T < nmv) {
        const i64 j = large_col(ops, (i64)ord[T]);
        const i32 a = ops.v0[j], f = ops.v1[j];
        if (a >= 0) atomicMax(&tab[h].wa, T + 1u);
        if (f >= 0) atomicMax(&tab[h].wf, T + 1u);
        none_here |= (a < 0) | (f < 0);
      } else if (!xy[T].x) {  // a kept rename (compose.py:71-72)
        atomicMax(&tab[h].wr, T + 1u);
      }
    }
  }
  const bool any_none = __syncthreads_or(none_here);  // (also orders the last-writer maxes)
  if (any_none) {
    // the moves' inclusive prefixes (compose.py:73-82), as smx_small.h phase 3: one wave walks
    // the move block in T order, 64 moves a step
    for (u32 i = t; i < HT; i += NT) run[i] = LargeRun{0u, 0u};
    __syncthreads();
    if (wv == 0) {
      const u64 lt = lanemask_lt();
      for (u32 c0 = 0; c0 < nmv; c0 += WAVE) {
        const u32 T = c0 + lane;
        const bool v = T < nmv;
        const u32 h = v ? slot[T] : 0u;
        const i64 j = large_col(ops, v ? (i64)ord[T] : 0);
        const bool ha = v && ops.v0[j] >= 0, hf = v && ops.v1[j] >= 0;
        const u64 peers = wave_peers<32>(h, v);
        const u64 pa = __ballot(ha) & peers, pf = __ballot(hf) & peers;
        const u32 ra = v ? run[h].a : 0u, rf = v ? run[h].f : 0u;  // (read before the step's updates)
        if (v) {
          xy[T].x = (pa & lt) ? c0 + (u32)(63 - __clzll(pa & lt)) + 1u : ra;
          xy[T].y = (pf & lt) ? c0 + (u32)(63 - __clzll(pf & lt)) + 1u : rf;
        }
        __builtin_amdgcn_wave_barrier();
        if (ha && (pa >> lane) == 1ull) run[h].a = T + 1u;
        if (hf && (pf >> lane) == 1ull) run[h].f = T + 1u;
        // the step's stores before the next step's loads, across the lanes of the wave
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
      }
    }
    __syncthreads();
  }
  // 4. emit: T -> T - skips before it (renames only are skipped)
  u32 skipped = 0;
  for (u32 base = 0; base < n; base += NT) {
    const u32 T = base + t;
    const u32 sk = T >= nmv && T < rend ? xy[T].x : 0u;
    u32 tot;
    const u32 before = skipped + block_excl_scan<OpSum, u32, NW>(sk, sscan, &tot);  // (syncs)
    skipped += tot;
    if (T >= n || sk) continue;
    const u32 e = ord[T];
    const i64 j = large_col(ops, (i64)e);
    i32 a = SMX_NONE, f = SMX_NONE, c = SMX_NONE;
    if (T < nmv) {
      // the inclusive prefix of the symbol's moves: its own value, else the last earlier
      // non-None one (compose.py:73-82 then 37-41)
      a = ops.v0[j];
      f = ops.v1[j];
      const LargeXY p = xy[T];  // (only a walk over None values sets them)
      if (a < 0 && p.x) a = ops.v0[large_col(ops, (i64)ord[p.x - 1])];
      if (f < 0 && p.y) f = ops.v1[large_col(ops, (i64)ord[p.y - 1])];
    } else if (rend > 0) {
      const u32 k = ops.kind[j];
      bool found = T < rend;
      u32 h = found ? slot[T] : 0u;
      if (!found) {
        const u32 s = ops.sym[j];
        h = home(s);
        for (u32 probe = 0; probe < HT; ++probe) {
          const u32 cur = tab[h].key;
          if (cur == s) {
            found = true;
            break;
          }
          if (cur == SMALL_EMPTY) break;
          h = h + 1 == HT ? 0u : h + 1;
        }
      }
      if (found) {
        const LargeSlot sl = tab[h];
        const u32 wa = sl.wa, wf = sl.wf, wr = sl.wr;
        if (wa) a = ops.v0[large_col(ops, (i64)ord[wa - 1])];
        if (wf) f = ops.v1[large_col(ops, (i64)ord[wf - 1])];
        if (k != SMX_KIND_RENAME && wr) c = ops.v1[large_col(ops, (i64)ord[wr - 1])];  // renameContext: non-renames only
      }
    }
    const u32 o = T - before;
    out.order[o] = (i32)e;
    out.addr[o] = a;
    out.file[o] = f;
    out.ctx[o] = c;
  }
}

// The merges of the fourth list: one workgroup per merge, b, b + grid, ... one after another.
template <typename B>
__global__ void __launch_bounds__(LARGE_NT) k_compose_batch_large(B b, const u32* cnt, BatchLargeWs w) {
  const u32 c = *cnt;
  for (u32 i = blockIdx.x; i < c; i += gridDim.x) {
    const i64 m = (i64)w.list[i];
    smx_ops ops;
    smx_compose_out out;
    batch_merge(b, m, &ops, &out);
    compose_large(ops, out, w, batch_slice(b, m));
    __syncthreads();  // the next merge's first phase overwrites what this one's last phase reads
  }
}
