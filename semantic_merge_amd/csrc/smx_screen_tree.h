// smx_screen_tree.h — screen merge trains that share prefixes for DivergentRename conflicts from
// the logs' renames alone (smx_screen_tree).
//
// smx_screen_train.h: as far as conflicts go, an accumulator is a sorted list of rename records, a
// step is the screen's two-head walk and a landing is a stable merge, A first on equal keys.
// smx_tree.h: nodes are stored level by level, a node's accumulator lives in its own region and
// is where all its children start, and a level depends on the level before through stream order
// alone.  Together: every log's renames extracted and sorted once, every node walked once against
// its parent's accumulator, and no size refused.
//
// The six record arrays have n_total + n_acc entries: the logs' records at [0, n_total), as
// k_screen_extract and k_screen_extract_large write them, and node n's region at
// n_total + acc_off[n].  One buffer per node: the parent's region is the state in, the node's own
// the state out.  acc_node[n] names the node whose region holds n's accumulator: n itself only
// when it landed and its log has renames; else acc_node[parent] (a conflict, a -1, a landed log
// without renames: nothing is copied), SMX_NONE while nothing on the root path put a rename down.
// An accumulator record keeps its op's column index in ridx (screen_pair_round's A side, as in
// k_screen_train).
//
//   k_screen_tree_offsets  one workgroup checks log_off, acc_off and level_off with a running
//                          maximum each (screen_log_bounds) and clears the class counts
//   k_screen_extract, k_screen_extract_large   every log's renames, once (smx_screen.h)
//   k_screen_tree_prepass  one workgroup, the levels one after another, a thread per node: the node
//                          fails structurally (counts -1, -1) or gets P(n), the rename counts of
//                          the valid logs on its root path, which needs its parent's, and goes on
//                          the list of its class inside its level's segment of the lists: by
//                          min(P(n), SCREEN_N), and the smallest class for a node whose own log is
//                          invalid or has no renames (it only hands its parent's state on)
//   k_screen_tree<N>       per level and class, a residency-capped grid; workgroup b runs nodes b,
//                          b + grid, ... of the level's class list
// 4 + 3 * n_levels launches, nothing waited for, allocated or read back.  The entry point is in
// smx_batch.hip.
#pragma once

#include "smx_screen_train.h"
#include "smx_tree.h"  // TREE_MAX_LEVELS

typedef struct smx_screen_tree ScreenTreeArgs;

// The workspace: smx_screen's for n_total + n_acc records and n_nodes list entries, then the
// nodes' verdicts and acc_node, the levels' verdicts and class counts, and the large logs' two
// index arrays.
struct ScreenTreeWs {
  i32* ainfo;     // [n_nodes]: screen_log_bounds' verdict on acc_off
  i64* pinfo;     // [n_nodes]: -1 failed structurally, else P(n)
  i32* acc_node;  // [n_nodes]
  i32* vinfo;     // [n_levels]: screen_log_bounds' verdict on level_off
  u32* lcnt;      // [n_levels][4]: the level's three class counts, then its first node
  ScreenLargeWs x;  // (list: not used)
};
static inline size_t screen_tree_ws_bytes(int64_t n_logs, int64_t n_total, int64_t n_nodes, int64_t n_levels,
                                          int64_t n_acc) {
  return screen_ws_bytes(n_logs, n_total + n_acc, n_nodes) + 2 * screen_al((size_t)n_nodes * 4) +
         screen_al((size_t)n_nodes * 8) + screen_al((size_t)n_levels * 4) + screen_al((size_t)n_levels * 16) +
         2 * screen_al((size_t)n_total * 4);
}
static inline ScreenTreeWs screen_tree_ws(void* workspace, int64_t n_logs, int64_t n_total, int64_t n_nodes,
                                          int64_t n_levels, int64_t n_acc) {
  char* p = (char*)workspace + screen_ws_bytes(n_logs, n_total + n_acc, n_nodes);
  auto take = [&](size_t bytes) {
    char* q = p;
    p += screen_al(bytes);
    return q;
  };
  ScreenTreeWs y;
  y.pinfo = (i64*)take((size_t)n_nodes * 8);
  y.ainfo = (i32*)take((size_t)n_nodes * 4);
  y.acc_node = (i32*)take((size_t)n_nodes * 4);
  y.vinfo = (i32*)take((size_t)n_levels * 4);
  y.lcnt = (u32*)take((size_t)n_levels * 16);
  y.x.list = nullptr;
  y.x.ia = (u32*)take((size_t)n_total * 4);
  y.x.ib = (u32*)take((size_t)n_total * 4);
  return y;
}

__global__ void __launch_bounds__(1024) k_screen_tree_offsets(ScreenTreeArgs b, ScreenWs w, ScreenTreeWs y) {
  __shared__ i64 sc[1024 / WAVE + 1];
  if (threadIdx.x < SCREEN_CLASSES) w.cnt[threadIdx.x] = 0;
  screen_log_bounds(b.log_off, b.n_logs, b.n_total, w.linfo, sc);
  screen_log_bounds(b.acc_off, b.n_nodes, b.n_acc, y.ainfo, sc);  // (each scan ends with a barrier: sc is free)
  screen_log_bounds(b.level_off, b.n_levels, b.n_nodes, y.vinfo, sc);
}

// After the extraction (linfo: -1 or the log's renames): every structural check, before any
// record of a node is read through an unchecked index.  The level rule and the parent rule are
// k_tree_prepass's (tree_level, tree_parent_ok in smx_tree.h).  A node outside every valid level
// fails, and so does a node whose parent breaks the parent rule, whose acc_off entries are bad,
// or whose own log is valid and has renames while its region is below P(n).
__global__ void __launch_bounds__(1024) k_screen_tree_prepass(ScreenTreeArgs b, ScreenWs w, ScreenTreeWs y) {
  __shared__ u32 c[SCREEN_CLASSES];
  const int t = threadIdx.x;
  for (i64 n = t; n < b.n_nodes; n += 1024) y.pinfo[n] = -1;
  __syncthreads();
  i64 plo = 0, phi = 0;  // the level before: its nodes (none: it is invalid, or this is level 0)
  for (i64 d = 0; d < b.n_levels; ++d) {
    if (t < SCREEN_CLASSES) c[t] = 0;
    __syncthreads();
    i64 lo, hi;
    tree_level(b.level_off, y.vinfo, d, b.n_levels, b.n_nodes, lo, hi);
    for (i64 n = lo + t; n < hi; n += 1024) {
      i64 ps;  // (at most 4096 levels of at most 2^31 - 1 renames each: no overflow)
      bool good = y.ainfo[n] >= 0 && tree_parent_ok(d, b.node_parent[n], plo, phi, y.pinfo, ps);
      i64 rb = -1;  // the node's own log: -1 invalid, else its renames
      if (good) {
        const i64 l = b.node_log[n];
        if (l >= 0 && l < b.n_logs) rb = w.linfo[l];
        if (rb > 0) {
          ps += rb;
          good = b.acc_off[n + 1] - b.acc_off[n] >= ps;
        }
      }
      if (good) {
        y.pinfo[n] = ps;
        int cls = 0;
        if (rb > 0)
          while (cls < SCREEN_CLASSES - 1 && ps > screen_class_cap(cls)) ++cls;
        w.lists[(size_t)cls * w.list_stride + lo + atomicAdd(&c[cls], 1u)] = (u32)n;
      }
    }
    __syncthreads();  // the level's pinfo and counts are complete
    if (t < SCREEN_CLASSES) y.lcnt[4 * d + t] = c[t];
    if (t == SCREEN_CLASSES) y.lcnt[4 * d + SCREEN_CLASSES] = (u32)lo;
    plo = lo;
    phi = hi;
  }
  for (i64 n = t; n < b.n_nodes; n += 1024)
    if (y.pinfo[n] < 0) {
      b.node_counts[2 * n] = -1;
      b.node_counts[2 * n + 1] = -1;
      y.acc_node[n] = SMX_NONE;
    }
}

// One level's nodes of one class by N / 2 threads: k_screen_train's step (screen_step_walk,
// screen_step_merge), with the accumulator in the region of acc_node[parent],
// node_counts[2 * parent] records long, and the accumulator out the node's own region.  (A node of
// class N < SCREEN_N never holds more than N.)
template <int N>
__global__ void __launch_bounds__(N / 2) k_screen_tree(ScreenTreeArgs b, ScreenWs w, ScreenTreeWs y, i32 level,
                                                       const u32* cnt, const u32* list) {
  __shared__ u32 heads[3];  // a round's two heads; the node's conflicts
  const int t = threadIdx.x;
  const u32 c = *cnt;
  list += y.lcnt[4 * level + SCREEN_CLASSES];
  for (u32 i = blockIdx.x; i < c; i += gridDim.x) {
    const i64 n = train_uniform((i64)list[i]);
    // (the pre-pass checked the parent: a node of the level before that did not fail, so its
    // count and acc_node are what that level's launches wrote)
    i64 acc = 0;
    i64 from = SMX_NONE;  // the node whose region holds the accumulator in
    if (level > 0) {
      const i64 p = train_uniform((i64)b.node_parent[n]);
      acc = train_uniform(b.node_counts[2 * p]);
      from = train_uniform((i64)y.acc_node[p]);
    }
    // (an empty accumulator may have no region: nothing is read through `at` then)
    const i64 at = from >= 0 ? b.n_total + train_uniform(b.acc_off[from]) : 0;
    const i64 l = train_uniform((i64)b.node_log[n]);
    const i64 RB = l >= 0 && l < b.n_logs ? train_uniform((i64)w.linfo[l]) : -1;
    i64 outcome = -1;
    bool own = false;  // the node landed and its log has renames: its region holds the accumulator
    if (RB >= 0) {  // (uniform)
      const i64 ob = train_uniform(b.log_off[l]);
      u32 nc = 0;
      if (acc > 0 && RB > 0) nc = screen_step_walk<N>(b, w, n, at, acc, ob, RB, heads);
      outcome = (i64)nc;
      if (nc == 0 && RB > 0) {  // the merge into the node's own region
        screen_step_merge<N>(w, at, acc, ob, RB, b.n_total + train_uniform(b.acc_off[n]));
        acc += RB;
        own = true;
      }
    }
    if (t == 0) {
      b.node_counts[2 * n] = acc;
      b.node_counts[2 * n + 1] = outcome;
      y.acc_node[n] = own ? (i32)n : (i32)from;
    }
    __syncthreads();  // the next node's rounds write the LDS that this one's walk read
  }
}
