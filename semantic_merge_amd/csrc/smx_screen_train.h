// smx_screen_train.h — screen merge trains for DivergentRename conflicts from the logs' renames
// alone (smx_screen_train).
//
// smx_screen.h: a pair's conflict list is a function of the two logs' rename subsequences.
// smx_train.h: a step that lands leaves a rename's timestamp, id, symbol and newName as they
// were.  So the accumulator of a train, as far as conflicts go, is a sorted list of rename
// records; a step is the screen's two-head walk of that list against one log's sorted renames,
// and a step that lands is a stable merge of the two lists, A first on equal keys.  No limit on
// ops or renames comes in anywhere.
//
// The kernels of smx_screen.h do the work, unchanged.  The six record arrays have
// n_total + 2 * n_acc entries: the logs' records at [0, n_total), as k_screen_extract and
// k_screen_extract_large write them, and behind them two buffers per train, at
// n_total + acc_off[r] and n_total + n_acc + acc_off[r], that hold the accumulator in turn.  An
// accumulator record keeps its op's column index in ridx, so screen_pair_round takes the
// accumulator as its A side through `oa`, and with len_a = log_off[l] its src[] is the column
// index for both sides.
//
//   k_screen_train_offsets   one workgroup checks log_off, train_off and acc_off with a running
//                            maximum each (screen_log_bounds) and clears the class counts
//   k_screen_extract, k_screen_extract_large   every log's renames, once (smx_screen.h)
//   k_screen_train_classify  a thread per train: fails it (counts -1, -1: bad offsets, or a
//                            region below the rename counts of its valid logs) or appends it to
//                            the list of its class, by min(that sum, SCREEN_N)
//   k_screen_train<N>        a residency-capped grid; workgroup b runs trains b, b + grid, ... of
//                            the class list, a train's steps one after another
// Seven launches, nothing waited for, allocated or read back.  The entry point is in smx_batch.hip.
//
// The step is stated here once, as screen_step_walk and screen_step_merge: k_screen_tree
// (smx_screen_tree.h) runs the same two on a node, and screen_step_logs serves both entry points
// (DESIGN.md §27).
#pragma once

#include "smx_screen.h"
#include "smx_train.h"  // train_uniform

typedef struct smx_screen_train ScreenTrainArgs;

// The workspace: smx_screen's for n_total + 2 * n_acc records and n_trains list entries (its
// class counts and lists are the trains'), then the trains' verdicts and the large logs' two
// index arrays.
struct ScreenTrainWs {
  i32 *tinfo, *ainfo;  // [n_trains]: screen_log_bounds' verdicts on train_off / acc_off
  ScreenLargeWs x;     // (list: not used)
};
static inline int64_t screen_train_records(int64_t n_total, int64_t n_acc) { return n_total + 2 * n_acc; }
static inline size_t screen_train_ws_bytes(int64_t n_logs, int64_t n_total, int64_t n_trains, int64_t n_acc) {
  return screen_ws_bytes(n_logs, screen_train_records(n_total, n_acc), n_trains) + 2 * screen_al((size_t)n_trains * 4) +
         2 * screen_al((size_t)n_total * 4);
}
static inline ScreenTrainWs screen_train_ws(void* workspace, int64_t n_logs, int64_t n_total, int64_t n_trains,
                                            int64_t n_acc) {
  char* p = (char*)workspace + screen_ws_bytes(n_logs, screen_train_records(n_total, n_acc), n_trains);
  ScreenTrainWs y;
  y.tinfo = (i32*)p;
  y.ainfo = (i32*)(p + screen_al((size_t)n_trains * 4));
  p += 2 * screen_al((size_t)n_trains * 4);
  y.x.list = nullptr;
  y.x.ia = (u32*)p;
  y.x.ib = (u32*)(p + screen_al((size_t)n_total * 4));
  return y;
}

// What the extraction kernels read of a screen over trains or over a tree (B: ScreenTrainArgs,
// ScreenTreeArgs): the logs and their columns.
template <typename B>
static inline ScreenArgs screen_step_logs(const B& b) {
  ScreenArgs s = {};
  s.n_logs = b.n_logs, s.n_total = b.n_total, s.log_off = b.log_off;
  s.kind = b.kind, s.ts = b.ts, s.oid_hi = b.oid_hi, s.oid_lo = b.oid_lo, s.sym = b.sym, s.v0 = b.v0;
  s.grid_cap = b.grid_cap;
  return s;
}

__global__ void __launch_bounds__(1024) k_screen_train_offsets(ScreenTrainArgs b, ScreenWs w, ScreenTrainWs y) {
  __shared__ i64 sc[1024 / WAVE + 1];
  if (threadIdx.x < SCREEN_CLASSES) w.cnt[threadIdx.x] = 0;
  screen_log_bounds(b.log_off, b.n_logs, b.n_total, w.linfo, sc);
  screen_log_bounds(b.train_off, b.n_trains, b.n_steps, y.tinfo, sc);  // (each scan ends with a barrier: sc is free)
  screen_log_bounds(b.acc_off, b.n_trains, b.n_acc, y.ainfo, sc);
}

// After the extraction (linfo: -1 or the log's renames): train r's class, by the most renames
// its accumulator can hold, or counts -1, -1.
__global__ void __launch_bounds__(256) k_screen_train_classify(ScreenTrainArgs b, ScreenWs w, ScreenTrainWs y) {
  __shared__ u32 c[SCREEN_CLASSES], start[SCREEN_CLASSES];
  const int t = threadIdx.x;
  if (t < SCREEN_CLASSES) c[t] = 0;
  __syncthreads();
  const i64 r = (i64)blockIdx.x * 256 + t;
  int cls = -1;
  u32 rk = 0;
  if (r < b.n_trains) {
    i64 sum = -1;
    if (y.tinfo[r] >= 0 && y.ainfo[r] >= 0) {
      sum = 0;  // (at most 2^31 - 1 steps of at most 2^31 - 1 renames each: no overflow)
      for (i64 g = b.train_off[r]; g < b.train_off[r + 1]; ++g) {
        const i64 l = b.train_log[g];
        if (l >= 0 && l < b.n_logs && w.linfo[l] > 0) sum += w.linfo[l];
      }
      if (b.acc_off[r + 1] - b.acc_off[r] < sum) sum = -1;
    }
    if (sum < 0) {
      b.counts[2 * r] = -1;
      b.counts[2 * r + 1] = -1;
    } else {
      cls = 0;
      while (cls < SCREEN_CLASSES - 1 && sum > screen_class_cap(cls)) ++cls;
      rk = atomicAdd(&c[cls], 1u);
    }
  }
  __syncthreads();
  if (t < SCREEN_CLASSES) start[t] = c[t] ? atomicAdd(&w.cnt[t], c[t]) : 0u;
  __syncthreads();
  if (cls >= 0) w.lists[(size_t)cls * w.list_stride + start[cls] + rk] = (u32)r;
}

// ---- the step, for k_screen_train<N> and k_screen_tree<N> (smx_screen_tree.h) alike: N / 2
// threads, B the call's struct ----

// The walk of the accumulator's records [at, at + acc) against the log's [ob, ob + RB), both
// non-empty: the step as a pair of the screen, its conflict region conf_off[slot]'s (one that
// conf_off does not describe holds nothing).  At most N renames together are one round of
// screen_pair_round; any more run k_screen_stream's rounds of N / 2 records per side from the two
// heads.  Returns the conflicts, uniform, through heads[2].
template <int N, typename B>
__device__ __forceinline__ u32 screen_step_walk(const B& b, const ScreenWs& w, i64 slot, i64 at, i64 acc, i64 ob,
                                                i64 RB, u32* heads) {
  constexpr i64 CH = N / 2;
  u32 nc = 0;  // (wave 0's count, as screen_pair_round leaves it)
  ScreenArgs s = {};
  if (b.conflicts) {
    const i64 c0 = train_uniform(b.conf_off[slot]), c1 = train_uniform(b.conf_off[slot + 1]);
    if (c0 >= 0 && c1 >= c0) s.conflicts = b.conflicts, s.conf_off = b.conf_off;
  }
  const i64 rounds = SMX_CEIL_DIV(acc, CH) + SMX_CEIL_DIV(RB, CH);
  i64 iA = 0, iB = 0;
  for (i64 k = 0; k < rounds; ++k) {
    const bool whole = (acc - iA) + (RB - iB) <= (i64)N;
    const int nA = (int)(whole || acc - iA < CH ? acc - iA : CH);
    const int nB = (int)(whole || RB - iB < CH ? RB - iB : CH);
    screen_pair_round<N, true>(s, w, slot, at + iA, ob + iB, nA, nB, ob, nc, heads);
    __syncthreads();  // the heads; and the next round's load overwrites what this walk reads
    iA += (i64)__builtin_amdgcn_readfirstlane((int)heads[0]);
    iB += (i64)__builtin_amdgcn_readfirstlane((int)heads[1]);
    if (iA >= acc || iB >= RB) break;  // (uniform) a side is used up for good: the step is done
  }
  if (threadIdx.x == 0) heads[2] = nc;  // (wave 0 counted)
  __syncthreads();
  return (u32)__builtin_amdgcn_readfirstlane((int)heads[2]);
}

// The stable merge of the accumulator's records [at, at + acc) and the log's [ob, ob + RB) into
// [dst, dst + acc + RB): a record's place is its index in its own list and its rank in the other
// one, by the round's comparison (A: B keys strictly below; B: A keys at or below).  With an
// empty accumulator it is the copy of the log's sorted records, ridx turned into column indices.
template <int N>
__device__ __forceinline__ void screen_step_merge(const ScreenWs& w, i64 at, i64 acc, i64 ob, i64 RB, i64 dst) {
  const i64 n = acc + RB;
  for (i64 e = threadIdx.x; e < n; e += N / 2) {
    const bool sa = e < acc;
    const i64 own = sa ? e : e - acc;
    const i64 q = (sa ? at : ob) + own, base = sa ? ob : at;
    const u64 ts = w.rts[q], hi = w.rhi[q], lo = w.rlo[q];
    i64 lo_i = 0, hi_i = sa ? RB : acc;
    while (lo_i < hi_i) {
      const i64 mid = (lo_i + hi_i) >> 1;
      const u64 mt = w.rts[base + mid];
      bool below = mt < ts;
      if (mt == ts) {
        const u64 mh = w.rhi[base + mid];
        below = mh < hi;
        if (mh == hi) {
          const u64 ml = w.rlo[base + mid];
          // (A first on equal keys: the tie-break of smx_screen.h's merge of a pair's two lists too)
          below = sa ? ml < lo : ml <= lo;
        }
      }
      if (below) lo_i = mid + 1;
      else hi_i = mid;
    }
    const i64 d = dst + own + lo_i;
    w.rts[d] = ts;
    w.rhi[d] = hi;
    w.rlo[d] = lo;
    w.ridx[d] = sa ? w.ridx[q] : (u32)(ob + (i64)w.ridx[q]);  // the op's column index
    w.rsym[d] = w.rsym[q];
    w.rv0[d] = w.rv0[q];
  }
}

// Trains by N / 2 threads, a train's steps one after another; the accumulator goes to and fro
// between the train's two buffers.  (A train of class N < SCREEN_N never holds more than N.)
template <int N>
__global__ void __launch_bounds__(N / 2) k_screen_train(ScreenTrainArgs b, ScreenWs w, const u32* cnt, const u32* list) {
  __shared__ u32 heads[3];  // a round's two heads; a step's conflicts
  const int t = threadIdx.x;
  const u32 c = *cnt;
  for (u32 i = blockIdx.x; i < c; i += gridDim.x) {
    const i64 r = train_uniform((i64)list[i]);
    const i64 g1 = train_uniform(b.train_off[r + 1]);
    const i64 buf = b.n_total + train_uniform(b.acc_off[r]);
    i64 acc = 0, landed = 0;  // the accumulator: records [at, at + acc) of the record arrays
    i64 at = buf, other = buf + b.n_acc;
    for (i64 g = train_uniform(b.train_off[r]); g < g1; ++g) {
      const i64 l = train_uniform((i64)b.train_log[g]);
      const i64 RB = l >= 0 && l < b.n_logs ? train_uniform((i64)w.linfo[l]) : -1;
      i64 outcome = -1;
      if (RB >= 0) {  // (uniform)
        const i64 ob = train_uniform(b.log_off[l]);
        u32 nc = 0;
        if (acc > 0 && RB > 0) nc = screen_step_walk<N>(b, w, g, at, acc, ob, RB, heads);
        outcome = (i64)nc;
        if (nc == 0) {
          ++landed;
          if (RB > 0) {  // the merge into the other buffer
            const i64 n = acc + RB;
            screen_step_merge<N>(w, at, acc, ob, RB, other);
            const i64 sw = at;
            at = other;
            other = sw;
            acc = n;
          }
        }
      }
      if (t == 0) {
        b.step_counts[2 * g] = acc;
        b.step_counts[2 * g + 1] = outcome;
      }
      // the next step reads the merged records through global memory, and its rounds write the
      // LDS that this one's walk read
      __threadfence_block();
      __syncthreads();
    }
    if (t == 0) {
      b.counts[2 * r] = acc;
      b.counts[2 * r + 1] = landed;
    }
  }
}
