// smx_tree.h — merge trains that share prefixes, composed once (smx_compose_tree).
//
// A root-to-node path of the tree is a train of smx_compose_train (smx_train.h): node n composes
// (its parent's accumulator as A, log node_log[n] as B) by that kernel's step -- stage,
// compose_small, land -- and a level-0 node starts from the empty accumulator.  What the tree adds
// is where the accumulator lives: a node that lands writes its accumulator into its own result
// region, and its children read it from there.  So a prefix that many trains share is composed
// once, every node's accumulator is a result, and the two state buffers of TrainWs are gone: the
// parent's region is the state in, the node's own the state out.  A node that does not land
// (conflicts, -1, -2) writes no accumulator; node_acc[n] names the nearest ancestor-or-self that
// landed, and its children go on from that node's region.
//
// Nodes are stored level by level, and a level depends on the level before only through stream
// order: no workgroup waits for another one.
//
//   k_tree_prepass      one workgroup: log_off, res_off and level_off checked with a running
//                       maximum each (screen_log_bounds); then the levels one after another, a
//                       thread per node: the node fails structurally (counts -1, -1, node_acc
//                       SMX_NONE) or gets min(sum of the valid logs' lengths on its root path,
//                       SMALL_N), which needs its parent's, and goes on the list of that class
//                       inside its level's segment of the lists.  All of it is the input's shape,
//                       none of it a compose result, so it runs ahead of every level.
//   k_compose_tree<N>   per level and class, a residency-capped grid; workgroup b runs nodes b,
//                       b + grid, ... of the level's class list
// 1 + 3 * n_levels launches, nothing waited for, allocated or read back.  The classes are the
// trains' (256 / 1024 / 2048 ops by the path sum): a step of the 2048 class costs several of the
// 256 class, which outweighs the two launches a level spends on classes it may not have.  The
// entry point is in smx_batch.hip.
#pragma once

#include "smx_train.h"

#define TREE_MAX_LEVELS 4096
static_assert(TREE_MAX_LEVELS == SMX_TREE_MAX_LEVELS, "the header's limit");

// The workspace: the pre-pass's verdicts and lists, then arrays of n_out entries that hold every
// node's slice (staged columns, the step's scratch result) at its res_off.
struct TreeWs {
  u32* lcnt;                // [n_levels][4]: the level's three class counts, then its first node
  i32 *linfo, *rinfo, *vinfo;  // by log / node / level: screen_log_bounds' verdicts
  i32* ninfo;               // by node: -1 failed structurally, else min(path sum, SMALL_N)
  u32* lists;               // [BATCH_CLASSES][stride]; level d's lists start at its first node
  size_t stride;
  u8* kind;                 // the staged columns
  u64 *ts, *hi, *lo;
  u32* sym;
  i32 *v0, *v1;
  i32* res;                 // [5] arrays of `arr` words: a step's order / addr / file / ctx, then its
  size_t arr;               // conflict pairs (element indices)
};

static inline size_t tree_ws_bytes(int64_t n_logs, int64_t n_nodes, int64_t n_levels, int64_t n_out) {
  return train_arr_bytes(n_levels, 16) + batch_list_bytes(n_logs) + batch_list_bytes(n_levels) +
         (2 + BATCH_CLASSES) * batch_list_bytes(n_nodes) + train_arr_bytes(n_out, 1) +
         3 * train_arr_bytes(n_out, 8) + (3 + 5) * train_arr_bytes(n_out, 4);
}
static inline TreeWs tree_ws(void* workspace, int64_t n_logs, int64_t n_nodes, int64_t n_levels, int64_t n_out) {
  TreeWs w;
  char* p = (char*)workspace;
  auto take = [&](size_t bytes) {
    char* q = p;
    p += bytes;
    return q;
  };
  w.lcnt = (u32*)take(train_arr_bytes(n_levels, 16));
  w.linfo = (i32*)take(batch_list_bytes(n_logs));
  w.vinfo = (i32*)take(batch_list_bytes(n_levels));
  w.rinfo = (i32*)take(batch_list_bytes(n_nodes));
  w.ninfo = (i32*)take(batch_list_bytes(n_nodes));
  w.stride = batch_list_bytes(n_nodes) / 4;
  w.lists = (u32*)take(BATCH_CLASSES * batch_list_bytes(n_nodes));
  w.ts = (u64*)take(train_arr_bytes(n_out, 8));
  w.hi = (u64*)take(train_arr_bytes(n_out, 8));
  w.lo = (u64*)take(train_arr_bytes(n_out, 8));
  w.sym = (u32*)take(train_arr_bytes(n_out, 4));
  w.v0 = (i32*)take(train_arr_bytes(n_out, 4));
  w.v1 = (i32*)take(train_arr_bytes(n_out, 4));
  w.arr = train_arr_bytes(n_out, 4) / 4;
  w.res = (i32*)take(5 * train_arr_bytes(n_out, 4));
  w.kind = (u8*)take(train_arr_bytes(n_out, 1));
  return w;
}

// Log l of a node: valid under smx_screen's log_off rules.
__device__ __forceinline__ bool tree_log_ok(const smx_tree& b, const TreeWs& w, i64 l) {
  return l >= 0 && l < b.n_logs && w.linfo[l] >= 0;
}

// ---- the two structural rules of a tree, for k_tree_prepass and k_screen_tree_prepass
// (smx_screen_tree.h) ----

// The level rule: level d's nodes [lo, hi), none where the level is not valid.  A level is valid
// when its level_off entries are (vinfo, screen_log_bounds' verdict: not negative, not below an
// earlier entry, not decreasing, not past n_nodes), level 0 starts at node 0 and the last level
// ends at n_nodes; valid levels never overlap.
__device__ __forceinline__ void tree_level(const i64* level_off, const i32* vinfo, i64 d, i64 n_levels, i64 n_nodes,
                                           i64& lo, i64& hi) {
  lo = hi = 0;
  if (vinfo[d] >= 0) {
    lo = level_off[d];
    hi = level_off[d + 1];
    if ((d == 0 && lo != 0) || (d == n_levels - 1 && hi != n_nodes)) lo = hi = 0;
  }
}

// The parent rule, for a node of level d with parent p: a level-0 node has none; any other's
// lies in the level before, [plo, phi) (that level invalid: no node does), and did not fail
// (info[p] >= 0).  ps: the parent's info, 0 without a parent.
template <typename T>
__device__ __forceinline__ bool tree_parent_ok(i64 d, i64 p, i64 plo, i64 phi, const T* info, i64& ps) {
  ps = 0;
  if (d == 0) return p == SMX_NONE;
  if (p < plo || p >= phi) return false;
  ps = info[p];
  return ps >= 0;
}

// Every structural check, before any column of a node is read through an unchecked index.  A
// node outside every valid level fails (tree_level), and so does a node whose parent breaks the
// parent rule (tree_parent_ok), whose res_off entries are bad or whose region is below
// min(path sum, SMALL_N).
__global__ void __launch_bounds__(1024) k_tree_prepass(smx_tree b, TreeWs w) {
  __shared__ i64 sc[1024 / WAVE + 1];
  __shared__ u32 c[BATCH_CLASSES];
  const int t = threadIdx.x;
  screen_log_bounds(b.log_off, b.n_logs, b.n_total, w.linfo, sc);
  screen_log_bounds(b.res_off, b.n_nodes, b.n_out, w.rinfo, sc);  // (each scan ends with a barrier: sc is free)
  screen_log_bounds(b.level_off, b.n_levels, b.n_nodes, w.vinfo, sc);
  for (i64 n = t; n < b.n_nodes; n += 1024) w.ninfo[n] = -1;
  __syncthreads();
  i64 plo = 0, phi = 0;  // the level before: its nodes (none: it is invalid, or this is level 0)
  for (i64 d = 0; d < b.n_levels; ++d) {
    if (t < BATCH_CLASSES) c[t] = 0;
    __syncthreads();
    i64 lo, hi;
    tree_level(b.level_off, w.vinfo, d, b.n_levels, b.n_nodes, lo, hi);
    for (i64 n = lo + t; n < hi; n += 1024) {
      i64 ps;
      bool good = w.rinfo[n] >= 0 && tree_parent_ok(d, b.node_parent[n], plo, phi, w.ninfo, ps);
      if (good) {
        const i64 l = b.node_log[n];
        if (tree_log_ok(b, w, l)) ps += b.log_off[l + 1] - b.log_off[l];
        if (ps > SMALL_N) ps = SMALL_N;
        good = b.res_off[n + 1] - b.res_off[n] >= ps;
      }
      if (good) {
        w.ninfo[n] = (i32)ps;
        int cls = 0;
        while (ps > batch_class_cap(cls)) ++cls;
        w.lists[(size_t)cls * w.stride + lo + atomicAdd(&c[cls], 1u)] = (u32)n;
      }
    }
    __syncthreads();  // the level's ninfo and counts are complete
    if (t < BATCH_CLASSES) w.lcnt[4 * d + t] = c[t];
    if (t == BATCH_CLASSES) w.lcnt[4 * d + BATCH_CLASSES] = (u32)lo;
    plo = lo;
    phi = hi;
  }
  for (i64 n = t; n < b.n_nodes; n += 1024)
    if (w.ninfo[n] < 0) {
      b.node_counts[2 * n] = -1;
      b.node_counts[2 * n + 1] = -1;
      b.node_acc[n] = SMX_NONE;
    }
}

// One level's nodes of one class.  k_compose_train's step, by its three loops (train_stage_loop,
// train_record_loop, train_land_loop in smx_train.h) in a skeleton of this kernel's own: the
// accumulator in is the region of node_acc[parent], node_counts[2 * parent] entries long, and
// the accumulator out the node's own region.
template <int N>
__global__ void __launch_bounds__(N / 2) k_compose_tree(smx_tree b, TreeWs w, i32 level, const u32* cnt,
                                                        const u32* list) {
  constexpr int NT = N / 2;
  const int t = threadIdx.x;
  const u32 c = *cnt;
  list += w.lcnt[4 * level + BATCH_CLASSES];
  const size_t arr = w.arr;
  for (u32 i = blockIdx.x; i < c; i += gridDim.x) {
    const i64 n = train_uniform((i64)list[i]);
    const i64 R = train_uniform(b.res_off[n]);
    // (the pre-pass checked the parent: a node of the level before that did not fail, so its
    // counts and node_acc are what that level's launches wrote)
    int acc = 0;
    i64 from = SMX_NONE;  // the node whose region holds the accumulator in
    if (level > 0) {
      const i64 p = train_uniform((i64)b.node_parent[n]);
      acc = (int)train_uniform(b.node_counts[2 * p]);
      from = train_uniform((i64)b.node_acc[p]);
    }
    // (an empty accumulator may have no region: nothing is read through A then)
    const i64 A = from >= 0 ? train_uniform(b.res_off[from]) : 0;
    const i64 l = train_uniform((i64)b.node_log[n]);
    i32* const res = w.res + R;
    i64 outcome = -1;
    i64 lo = 0, nb = 0;
    const bool ok = train_uniform((i64)tree_log_ok(b, w, l)) != 0;
    if (ok) {
      lo = train_uniform(b.log_off[l]);
      nb = train_uniform(b.log_off[l + 1]) - lo;
    }
    const bool fits = (i64)acc + nb <= (i64)SMALL_N;
    if (ok && !fits) outcome = -2;
    bool landed = false;
    if (ok && fits) {
      // (acc + nb is at most min(path sum, SMALL_N): the class's N at most, and the region's size)
      const int m = acc + (int)nb;
      const i32 *ssrc = b.src + A, *saddr = b.addr + A, *sfile = b.file + A, *sctx = b.ctx + A;
      train_stage_loop<NT>(b, w, R, ssrc, saddr, sfile, acc, m, lo);
      __syncthreads();
      const smx_ops ops = {(i64)acc, nb,       b.n_sym,   w.kind + R, w.ts + R, w.hi + R,
                           w.lo + R, w.sym + R, w.v0 + R, w.v1 + R,   0};
      // (the node's own counts take compose_small's pair; thread 0 overwrites them below)
      const smx_compose_out out = {res,           res + arr,    res + 2 * arr,     res + 3 * arr,
                                   res + 4 * arr, (i64)(m / 2), b.node_counts + 2 * n};
      compose_small<N, false>(ops, out, nullptr, nullptr, 0);
      __syncthreads();
      const i64 k = train_uniform(b.node_counts[2 * n]), nc = train_uniform(b.node_counts[2 * n + 1]);
      __syncthreads();  // every thread has read the pair before thread 0 replaces it
      if (k < 0) {
        outcome = -1;  // an op with kind >= 18 or sym >= n_sym in the log
      } else if (nc > 0) {
        outcome = nc;
        train_record_loop<NT>(b, n, nc, res + 4 * arr, ssrc, saddr, sfile, acc, lo);
      } else {
        outcome = 0;
        landed = true;
        train_land_loop<NT>(res, arr, (int)k, ssrc, saddr, sfile, sctx, acc, lo, b.src + R, b.addr + R, b.file + R,
                            b.ctx + R);
        acc = (int)k;
      }
    }
    if (t == 0) {
      b.node_counts[2 * n] = acc;
      b.node_counts[2 * n + 1] = outcome;
      b.node_acc[n] = landed ? (i32)n : (i32)from;
    }
    __syncthreads();  // the next node's compose_small sets its LDS up over what this one read
  }
}
