// smx_train.h — merge trains: each log composed against what landed before (smx_compose_train,
// DESIGN.md §21).
//
// A train takes logs P1..Pk in order: compose(acc, P1), and if that has no conflict the composed
// log becomes acc; a log that conflicts is put off the train and the next one goes on against
// what landed.  On the host that is a loop of compose, materialise, marshal again and copy in
// again per step.  Here a train is one workgroup's loop over compose_small (smx_small.h), and
// what leads from one step to the next is a gather.
//
// The accumulator is not a set of columns: it is, per entry, the op's column index (src: logs
// are stored once, so the index names log and op) and the addr / file / ctx it has gathered,
// per field the last value a step gave that was not SMX_NONE.  Its columns are the source op's
// own, except a move's v0 / v1: those are the accumulated addr / file where there is one --
// what marshalling the materialised op again would give (an accumulated file that is the
// empty string gives the op's own `file` instead, v1_alt: `newFile or file`).  So each step
//   stages   the accumulator's columns (gathered through src, moves rewritten) and the log's
//            behind them in the train's slice of the workspace: A and B with b_gap = 0
//   composes them with compose_small<N, false> into a scratch result in the same slice
//   lands    on zero conflicts: entry k of the new accumulator is the old entry order[k] (or a
//            fresh one of the log) with the step's addr / file / ctx folded in, written to the
//            other of two state buffers
//   or not   conflicts: their element indices translated to column indices, with the addr and
//            file the A op carried; an invalid log (-1) or one that does not fit (-2): the
//            accumulator stays and the train goes on with its next log
// The slices lie at the train's res_off in arrays of n_out entries, as the large batch's do:
// no per-workgroup slots, and a train whose region is too small never runs.
//
//   k_train_offsets    one workgroup checks log_off, train_off and res_off with a running
//                      maximum each (screen_log_bounds) and clears the class counts
//   k_train_classify   a thread per train: fails it (counts -1, -1) or appends it to the list
//                      of its class, by min(sum of its valid logs' lengths, SMALL_N)
//   k_compose_train<N> a residency-capped grid; workgroup b runs trains b, b + grid, ... of
//                      the class list one after another
// Five launches, nothing waited for, allocated or read back.  The entry point is in smx_batch.hip.
//
// The step's rules per entry (train_staged, train_landed, train_conflict_record) and its three
// loops in a workgroup (train_stage_loop, train_record_loop, train_land_loop) are stated here
// once: k_compose_tree (smx_tree.h) runs the same loops, k_train_stage and k_train_land
// (smx_train_step.h) the same rules.
#pragma once

#include "smx_batch.h"

// The workspace: the pre-pass's verdicts and lists, then arrays of n_out entries that hold
// every train's slice at its res_off.
struct TrainWs {
  u32* cnt;                 // [BATCH_CLASSES] class counts
  i32 *linfo, *tinfo, *rinfo;  // by log / by train: screen_log_bounds' verdicts
  u32* lists;               // [BATCH_CLASSES][stride]
  size_t stride;
  i64* rcounts;             // [2 * n_trains]: the last step's counts of each train
  u8* kind;                 // the staged columns
  u64 *ts, *hi, *lo;
  u32* sym;
  i32 *v0, *v1;
  // arrays of `arr` words each, one after another (one pointer and a stride: fewer registers
  // than a pointer per array)
  i32* st;                  // [2][4]: the accumulator's src / addr / file / ctx, two buffers
  i32* res;                 // [5]: a step's order / addr / file / ctx, then its conflict pairs
                            // (element indices)
  size_t arr;
};

static inline size_t train_arr_bytes(int64_t n_out, size_t width) {
  return ((size_t)n_out * width + 255) & ~(size_t)255;
}
static inline size_t train_ws_bytes(int64_t n_logs, int64_t n_trains, int64_t n_out) {
  return BATCH_HDR + batch_list_bytes(n_logs) + (2 + BATCH_CLASSES) * batch_list_bytes(n_trains) +
         train_arr_bytes(n_trains, 16) + train_arr_bytes(n_out, 1) + 3 * train_arr_bytes(n_out, 8) +
         (3 + 8 + 4 + 1) * train_arr_bytes(n_out, 4);
}
static inline TrainWs train_ws(void* workspace, int64_t n_logs, int64_t n_trains, int64_t n_out) {
  TrainWs w;
  char* p = (char*)workspace;
  auto take = [&](size_t bytes) {
    char* q = p;
    p += bytes;
    return q;
  };
  w.cnt = (u32*)take(BATCH_HDR);
  w.linfo = (i32*)take(batch_list_bytes(n_logs));
  w.tinfo = (i32*)take(batch_list_bytes(n_trains));
  w.rinfo = (i32*)take(batch_list_bytes(n_trains));
  w.stride = batch_list_bytes(n_trains) / 4;
  w.lists = (u32*)take(BATCH_CLASSES * batch_list_bytes(n_trains));
  w.rcounts = (i64*)take(train_arr_bytes(n_trains, 16));
  w.ts = (u64*)take(train_arr_bytes(n_out, 8));
  w.hi = (u64*)take(train_arr_bytes(n_out, 8));
  w.lo = (u64*)take(train_arr_bytes(n_out, 8));
  w.sym = (u32*)take(train_arr_bytes(n_out, 4));
  w.v0 = (i32*)take(train_arr_bytes(n_out, 4));
  w.v1 = (i32*)take(train_arr_bytes(n_out, 4));
  w.arr = train_arr_bytes(n_out, 4) / 4;
  w.st = (i32*)take(8 * train_arr_bytes(n_out, 4));
  w.res = (i32*)take(5 * train_arr_bytes(n_out, 4));
  w.kind = (u8*)take(train_arr_bytes(n_out, 1));
  return w;
}

__global__ void __launch_bounds__(1024) k_train_offsets(smx_train b, TrainWs w) {
  __shared__ i64 sc[1024 / WAVE + 1];
  if (threadIdx.x < BATCH_CLASSES) w.cnt[threadIdx.x] = 0;
  screen_log_bounds(b.log_off, b.n_logs, b.n_total, w.linfo, sc);
  screen_log_bounds(b.train_off, b.n_trains, b.n_steps, w.tinfo, sc);  // (each scan ends with a barrier: sc is free)
  screen_log_bounds(b.res_off, b.n_trains, b.n_out, w.rinfo, sc);
}

// Log l of a step: valid under smx_screen's log_off rules.
__device__ __forceinline__ bool train_log_ok(const smx_train& b, const TrainWs& w, i64 l) {
  return l >= 0 && l < b.n_logs && w.linfo[l] >= 0;
}

// Train r before any column is touched: -1 for bad offsets or a region below the sum of its
// valid logs' lengths (the most its accumulator can hold), else min(that sum, SMALL_N).
__device__ __forceinline__ i64 train_check(const smx_train& b, const TrainWs& w, i64 r) {
  if (w.tinfo[r] < 0 || w.rinfo[r] < 0) return -1;
  i64 sum = 0;  // (at most 2^31 - 1 steps of at most n_total ops each: no overflow)
  for (i64 g = b.train_off[r]; g < b.train_off[r + 1]; ++g) {
    const i64 l = b.train_log[g];
    if (train_log_ok(b, w, l)) sum += b.log_off[l + 1] - b.log_off[l];
  }
  if (b.res_off[r + 1] - b.res_off[r] < sum) return -1;
  return sum > SMALL_N ? SMALL_N : sum;
}

__global__ void __launch_bounds__(256) k_train_classify(smx_train b, TrainWs w) {
  __shared__ u32 c[BATCH_CLASSES], start[BATCH_CLASSES];
  const int t = threadIdx.x;
  if (t < BATCH_CLASSES) c[t] = 0;
  __syncthreads();
  const i64 r = (i64)blockIdx.x * 256 + t;
  int cls = -1;
  u32 rk = 0;
  if (r < b.n_trains) {
    const i64 len = train_check(b, w, r);
    if (len < 0) {
      b.counts[2 * r] = -1;
      b.counts[2 * r + 1] = -1;
    } else {
      cls = 0;
      while (len > batch_class_cap(cls)) ++cls;
      rk = atomicAdd(&c[cls], 1u);
    }
  }
  __syncthreads();
  if (t < BATCH_CLASSES) start[t] = c[t] ? atomicAdd(&w.cnt[t], c[t]) : 0u;
  __syncthreads();
  if (cls >= 0) w.lists[(size_t)cls * w.stride + start[cls] + rk] = (u32)r;
}

// A value every thread of the workgroup loads from the same address, in scalar registers: the
// loads below follow the kernel's own stores, so the compiler issues them per lane and would
// keep every length, offset and pointer derived from them in vector registers.
__device__ __forceinline__ i64 train_uniform(i64 v) {
  const u32 lo = (u32)__builtin_amdgcn_readfirstlane((int)(u32)v);
  const u32 hi = (u32)__builtin_amdgcn_readfirstlane((int)(u32)((u64)v >> 32));
  return (i64)((u64)hi << 32 | lo);
}

// ---- the step's rules, per entry: stated here once, for k_compose_train, k_compose_tree
// (smx_tree.h) and k_train_stage / k_train_land (smx_train_step.h) ----

// The staged v0 / v1 of an entry: the op's own, except a move's -- those are what marshalling
// the materialised move would give, the accumulated addr `a` / file `f` where there is one.
// (v1_alt is read only where f is empty_str: it may be null while empty_str is SMX_NONE.)
__device__ __forceinline__ void train_staged(u8 kind, i32 v0, i32 v1, i32 a, i32 f, i32 empty_str, const i32* v1_alt,
                                             i64 j, i32& x0, i32& x1) {
  x0 = v0, x1 = v1;
  if (kind == SMX_KIND_MOVE) {
    if (a != SMX_NONE) x0 = a;
    // (an empty newFile: marshalling falls through to the op's own `file`)
    if (f != SMX_NONE) x1 = f == empty_str ? v1_alt[j] : f;
  }
}

// Per field, the last value a step gave that was not SMX_NONE.
__device__ __forceinline__ i32 train_fold(i32 ra, i32 a) { return ra != SMX_NONE ? ra : a; }

// Entry q of the accumulator a landing leaves: element e of the step (an entry of the
// accumulator in below n_acc, else op e - n_acc of the log that starts at column lo) with the
// step's addr / file / ctx folded in.
__device__ __forceinline__ void train_landed(i64 e, i64 n_acc, i64 lo, const i32* ssrc, const i32* saddr,
                                             const i32* sfile, const i32* sctx, i32 ra, i32 rf, i32 rx, i32* nsrc,
                                             i32* naddr, i32* nfile, i32* nctx, i64 q) {
  i32 s = (i32)(lo + (e - n_acc)), a = SMX_NONE, f = SMX_NONE, x = SMX_NONE;
  if (e < n_acc) {
    s = ssrc[e];
    a = saddr[e];
    f = sfile[e];
    x = sctx[e];
  }
  nsrc[q] = s;
  naddr[q] = train_fold(ra, a);
  nfile[q] = train_fold(rf, f);
  nctx[q] = train_fold(rx, x);
}

// A conflict pair of element indices (ea in the accumulator, eb in the log) as a record: the
// two ops' column indices, and the addr and file the A op carried.
__device__ __forceinline__ void train_conflict_record(i32* rec, i64 ea, i64 eb, i64 n_acc, i64 lo, const i32* ssrc,
                                                      const i32* saddr, const i32* sfile) {
  rec[0] = ssrc[ea];
  rec[1] = (i32)(lo + (eb - n_acc));
  rec[2] = saddr[ea];
  rec[3] = sfile[ea];
}

// ---- the step's three loops in a workgroup of NT threads, for k_compose_train and k_compose_tree
// (B: smx_train / smx_tree, W: TrainWs / TreeWs).  Each makes the thread index opaque: else each
// array's per-thread address is computed once for the whole train and lives in registers across
// compose_small ----

// Stages the accumulator in (acc entries, gathered through ssrc with the moves rewritten) and
// the log [lo, lo + n - acc) behind it at the slice R.
template <int NT, typename B, typename W>
__device__ __forceinline__ void train_stage_loop(const B& b, const W& w, i64 R, const i32* ssrc, const i32* saddr,
                                                 const i32* sfile, int acc, int n, i64 lo) {
  int tt = threadIdx.x;
  asm volatile("" : "+v"(tt));
#pragma unroll 1
  for (int e = tt; e < n; e += NT) {
    i64 j = lo + (e - acc);
    i32 a = SMX_NONE, f = SMX_NONE;
    if (e < acc) {
      j = ssrc[e];
      a = saddr[e];
      f = sfile[e];
    }
    const u8 k = b.kind[j];
    i32 x0, x1;
    train_staged(k, b.v0[j], b.v1[j], a, f, b.empty_str, b.v1_alt, j, x0, x1);
    w.kind[R + e] = k;
    w.ts[R + e] = b.ts[j];
    w.hi[R + e] = b.oid_hi[j];
    w.lo[R + e] = b.oid_lo[j];
    w.sym[R + e] = b.sym[j];
    w.v0[R + e] = x0;
    w.v1[R + e] = x1;
  }
}

// The step's nc conflict pairs (element indices) as records in the region of conf_off[slot]: as
// many as it holds, and one that conf_off does not describe holds none.
template <int NT, typename B>
__device__ __forceinline__ void train_record_loop(const B& b, i64 slot, i64 nc, const i32* pairs, const i32* ssrc,
                                                  const i32* saddr, const i32* sfile, int acc, i64 lo) {
  const i64 c0 = train_uniform(b.conf_off[slot]), c1 = train_uniform(b.conf_off[slot + 1]);
  i64 cap = c0 < 0 || c1 < c0 ? 0 : c1 - c0;
  if (cap > nc) cap = nc;
  int tt = threadIdx.x;
  asm volatile("" : "+v"(tt));
#pragma unroll 1
  for (i64 q = tt; q < cap; q += NT)
    train_conflict_record(b.conflicts + 4 * (c0 + q), pairs[2 * q], pairs[2 * q + 1], acc, lo, ssrc, saddr, sfile);
}

// The k entries of the accumulator out from the step's result (res: order / addr / file / ctx,
// arrays of arr words).
template <int NT>
__device__ __forceinline__ void train_land_loop(const i32* res, size_t arr, int k, const i32* ssrc, const i32* saddr,
                                                const i32* sfile, const i32* sctx, int acc, i64 lo, i32* nsrc,
                                                i32* naddr, i32* nfile, i32* nctx) {
  int tt = threadIdx.x;
  asm volatile("" : "+v"(tt));
#pragma unroll 1
  for (int q = tt; q < k; q += NT)
    train_landed(res[q], acc, lo, ssrc, saddr, sfile, sctx, res[arr + q], res[2 * arr + q], res[3 * arr + q], nsrc,
                 naddr, nfile, nctx, q);
}

template <int N>
__global__ void __launch_bounds__(N / 2) k_compose_train(smx_train b, TrainWs w, const u32* cnt, const u32* list) {
  constexpr int NT = N / 2;
  const int t = threadIdx.x;
  const u32 c = *cnt;
  for (u32 i = blockIdx.x; i < c; i += gridDim.x) {
    const i64 r = train_uniform((i64)list[i]);
    const i64 R0 = train_uniform(b.res_off[r]), g1 = train_uniform(b.train_off[r + 1]);
    int acc = 0;  // the accumulator: entries [0, acc) of ssrc / saddr / sfile / sctx
    i64 landed = 0;
    int cur = 0;  // which of the two state buffers holds the accumulator
    const size_t arr = w.arr;
    for (i64 g = train_uniform(b.train_off[r]); g < g1; ++g) {
      const i64 l = train_uniform((i64)b.train_log[g]);
      // (the slice's offset made opaque per step: else every per-thread address that compose_small
      // derives from it is computed once for the whole train and kept in registers)
      i64 R = R0;
      asm volatile("" : "+s"(R));
      i32* const res = w.res + R;
      i64 outcome = -1;
      i64 lo = 0, nb = 0;
      const bool ok = train_uniform((i64)train_log_ok(b, w, l)) != 0;
      if (ok) {
        lo = train_uniform(b.log_off[l]);
        nb = train_uniform(b.log_off[l + 1]) - lo;
      }
      const bool fits = (i64)acc + nb <= (i64)SMALL_N;
      if (ok && !fits) outcome = -2;
      if (ok && fits) {
        // (acc + nb is at most the class's N: the train's sum is, or N is SMALL_N)
        const int n = acc + (int)nb;
        const i32* const ssrc = w.st + (size_t)cur * 4 * arr + R;
        const i32 *saddr = ssrc + arr, *sfile = ssrc + 2 * arr, *sctx = ssrc + 3 * arr;
        train_stage_loop<NT>(b, w, R, ssrc, saddr, sfile, acc, n, lo);
        __syncthreads();
        const smx_ops ops = {(i64)acc, nb,       b.n_sym,   w.kind + R, w.ts + R, w.hi + R,
                             w.lo + R, w.sym + R, w.v0 + R, w.v1 + R,   0};
        const smx_compose_out out = {res,           res + arr,    res + 2 * arr,    res + 3 * arr,
                                     res + 4 * arr, (i64)(n / 2), w.rcounts + 2 * r};
        compose_small<N, false>(ops, out, nullptr, nullptr, 0);
        __syncthreads();
        const i64 k = train_uniform(w.rcounts[2 * r]), nc = train_uniform(w.rcounts[2 * r + 1]);
        // (the log's start read again: one scalar pair fewer to keep across compose_small)
        const i64 lo2 = train_uniform(b.log_off[train_uniform((i64)b.train_log[g])]);
        if (k < 0) {
          outcome = -1;  // an op with kind >= 18 or sym >= n_sym in the log
        } else if (nc > 0) {
          outcome = nc;
          train_record_loop<NT>(b, g, nc, res + 4 * arr, ssrc, saddr, sfile, acc, lo2);
        } else {
          outcome = 0;
          i32* const nsrc = w.st + (size_t)(cur ^ 1) * 4 * arr + R;
          train_land_loop<NT>(res, arr, (int)k, ssrc, saddr, sfile, sctx, acc, lo2, nsrc, nsrc + arr, nsrc + 2 * arr,
                              nsrc + 3 * arr);
          cur ^= 1;
          acc = (int)k;
          ++landed;
        }
      }
      if (t == 0) {
        b.step_counts[2 * g] = acc;
        b.step_counts[2 * g + 1] = outcome;
      }
      __syncthreads();  // the next step stages over what this one read, and reads what it wrote
    }
    const i64 R = R0;
    const i32* const fin = w.st + (size_t)cur * 4 * arr + R;
#pragma unroll 1
    for (int q = t; q < acc; q += NT) {
      b.src[R + q] = fin[q];
      b.addr[R + q] = fin[arr + q];
      b.file[R + q] = fin[2 * arr + q];
      b.ctx[R + q] = fin[3 * arr + q];
    }
    if (t == 0) {
      b.counts[2 * r] = acc;
      b.counts[2 * r + 1] = landed;
    }
  }
}
