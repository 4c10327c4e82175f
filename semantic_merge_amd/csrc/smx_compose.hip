// smx_compose.hip — MI355X (gfx950) implementation of semmerge's compose_oplogs
// (semmerge/compose.py:11-114) behind the C ABI of include/smx.h.
//
// Exact data-parallel restatement of the reference's sequential loop:
//   T      = stable order of A||B by (precedence, timestamp, id, side, index)
//            (per-branch sorted() + merge with A on ties, compose.py:16-21,51-56)
//   moves  precede renames precede everything else in T, so
//            moveDecl k sees the inclusive per-symbol prefix of last non-None
//            newAddress/newFile; every later op sees the final move state;
//            non-renames see the final non-skipped rename (compose.py:27-49,71-82)
//   DivergentRename skips (compose.py:60-70,88-98) are found by replaying a
//            two-state transducer (ahead side, depth d) over the rename block
//            from every "natural-head" candidate, and resolving overlapping
//            regions cluster by cluster.
//
// Pipeline (one merge):
//   k_fpart     presorted windows: merge-path on timestamps, cut at ts boundaries
//   k_wcount    per-window kind counts + presorted-layout checks
//   k_wscan     window offsets and kind totals  k_bases   T segment starts
//   [generic]   radix-sort each branch by (ts, oid) and cut fixed windows
//   k_window    per window, in LDS: the T order (presorted, k_window_f: ops grouped by
//               (kind, timestamp run), each group ordered by id, no merge; generic,
//               k_window_g: merge A/B parts, multisplit by kind); the moves' final
//               records, the other ops' (source, symbol) in T order, natural-head
//               DivergentRename flags
//   walk        k_boundary -> candidate scan/compact -> k_replay_q -> max-scan ->
//               k_cluster -> scan -> k_replay_write (conflict pairs, skip bits,
//               sorted skip list)
//   tables      per-symbol last writers: bucket by symbol range, LDS max-reduce
//   k_emit      compacted output of every op after the move block: order, addr,
//               file, ctx
// A merge of at most SMALL_N ops skips all of that: k_compose_small, one workgroup
// (smx_small.h).  The entry points that take many merges or log pairs at once are a unit of
// their own, smx_batch.hip.
//
// This file: the workspace layout, Ctx, the launchers, the plans with their fallback chain
// and one merge's entry points.  Headers included once each, here, hold the rest: smx_prof.h
// (last error, stage timers), smx_plan.h, smx_window.h, smx_walk.h, smx_tables.h, smx_emit.h,
// smx_segsort.h, smx_small.h, smx_sort.h, and smx_shard.h (the sharded merge) at the end.
#include <algorithm>
#include <atomic>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "smx_sort.h"
#include "smx_window.h"
#include "smx_small.h"
#include "smx_tables.h"


#include "smx_prof.h"

#include "smx_plan.h"
#include "smx_walk.h"

#include "smx_emit.h"

// ---------------------------------------------------------------------------
// workspace layout

struct Layout {
  size_t off[64];
  size_t total;
};

enum Buf {
  B_META, B_BND, B_WCNT, B_WOFF, B_STS, B_SHI, B_SLO, B_PERM, B_RKEY, B_RVAL, B_RK2, B_RV2,
  B_RHIST, B_PART, B_MSYM, B_TSRC, B_TSYM, B_RSTR, B_WREN, B_WBND, B_CSLOT, B_WCAND, B_WCANDB,
  B_WCOFF, B_CAND, B_Q, B_PM, B_NCONF, B_NREAL, B_COFF, B_SKIPBITS, B_SKIPLIST,
  B_TABA, B_TABF, B_TABR, B_FIN, B_REC, B_TBHIST, B_CCNT, B_TSUM, B_SMP, B_N
};

static i64 max_windows(i64 nn) { return SMX_CEIL_DIV(nn, (i64)WIN_TGT_MIN) + 2; }

static Layout layout(i64 na, i64 nb, i64 n_sym) {
  const i64 n = na + nb;
  const i64 nn = n > 0 ? n : 1;
  const i64 W = max_windows(nn);
  size_t sz[B_N];
  sz[B_META] = sizeof(ComposeMeta);
  sz[B_BND] = (size_t)(W + 1) * 2 * 8;
  sz[B_WCNT] = (size_t)NCNT * W * 4;
  sz[B_WOFF] = (size_t)NCNT * W * 4;
  sz[B_STS] = sz[B_SHI] = sz[B_SLO] = (size_t)nn * 8;
  sz[B_PERM] = (size_t)nn * 4;
  sz[B_RKEY] = (size_t)nn * 8;
  sz[B_RVAL] = (size_t)nn * 4;
  sz[B_RK2] = (size_t)nn * 8;
  sz[B_RV2] = (size_t)nn * 4;
  sz[B_RHIST] = radix_hist_bytes(nn);
  sz[B_PART] = (size_t)SCAN_NB * 8;
  sz[B_MSYM] = sz[B_TSRC] = sz[B_TSYM] = sz[B_RSTR] = (size_t)nn * 4;
  sz[B_WREN] = (size_t)W * 2 * 4;
  sz[B_WBND] = sz[B_WCAND] = sz[B_WCANDB] = sz[B_WCOFF] = (size_t)W * 4;
  sz[B_CSLOT] = sz[B_CAND] = sz[B_Q] = sz[B_PM] = sz[B_NCONF] = sz[B_NREAL] = sz[B_COFF] = (size_t)nn * 4;
  sz[B_SKIPBITS] = (size_t)(SMX_CEIL_DIV(nn, (i64)64) + 1) * 8;
  sz[B_SKIPLIST] = (size_t)nn * 4;
  const i64 ns = n_sym > 0 ? n_sym : 1;
  sz[B_TABA] = sz[B_TABF] = sz[B_TABR] = (size_t)ns * 4;
  sz[B_FIN] = (size_t)ns * 16;
  sz[B_REC] = (size_t)nn * 4;
  sz[B_TBHIST] = (size_t)(TB_MAXBK + 1) * SMX_CEIL_DIV(nn, (i64)TB_TILE) * 4;  // k_tb_scatter's lst
  sz[B_CCNT] = (size_t)2 * SMX_N_KINDS * (SMX_CEIL_DIV(nn, (i64)256) + 2) * 4;
  sz[B_SMP] = (size_t)(SMX_CEIL_DIV(nn, (i64)CH) + 4) * 8;
  sz[B_TSUM] = (size_t)2 * SMX_N_KINDS * (SMX_CEIL_DIV(nn, (i64)CH * CS_TILE) + 2) * 4;
  Layout L{};
  size_t acc = 0;
  for (int i = 0; i < B_N; ++i) {
    L.off[i] = acc;
    acc += (sz[i] + 255) & ~(size_t)255;
  }
  L.total = acc;
  return L;
}

// ---------------------------------------------------------------------------
// C ABI

static int grid_for(i64 n, int per_block_items = BLOCK) {
  i64 g = SMX_CEIL_DIV(n > 0 ? n : 1, (i64)per_block_items);
  if (g > 4096) g = 4096;
  return (int)g;
}

extern "C" int smx_compose_workspace_bytes(int64_t n_a, int64_t n_b, int64_t n_sym, size_t* bytes) {
  if (!bytes || n_a < 0 || n_b < 0 || n_sym < 0) return set_err(SMX_E_ARG, "bad argument");
  *bytes = layout(n_a, n_b, n_sym).total;
  return SMX_OK;
}

struct Ctx {
  const smx_ops* ops;
  const smx_compose_out* out;
  hipStream_t st;
  Layout L{};
  char* base;
  i64 na, nb, n, n_sym;
  i64 src_a, src_b;  // global source index of local op j (see WinArgs)
  StageTimer* tm;
  const i32* src_map = nullptr;
  u64* hrec = nullptr;  // the synchronous call's verdict word (k_emit stores it), or null
  u64 hseq = 0;
  template <typename T>
  T* ws(int b) const { return (T*)(base + L.off[b]); }
};
// (a single merge: src_a = 0, src_b = n_a, so local and global source indices agree)
static Ctx make_ctx(const smx_ops* ops, const smx_compose_out* out, void* ws, const Layout& L, hipStream_t st,
                    StageTimer* tm, i64 src_a, i64 src_b) {
  return Ctx{ops, out, st, L, (char*)ws, ops->n_a, ops->n_b, ops->n_a + ops->n_b, ops->n_sym, src_a, src_b, tm};
}

// Diagnostic builds only (tools/window_phases.py): a device buffer for k_window_f's
// step stamps (its DBG instances: the shipped order with stamps).
#if SMX_DIAG
static void* g_phase_dbg = nullptr;
static size_t g_phase_dbg_bytes = 0;
extern "C" int smx_debug_phase_buffer(void* p, size_t bytes) {
  g_phase_dbg = p;
  g_phase_dbg_bytes = bytes;
  return SMX_OK;
}
#else
static constexpr void* g_phase_dbg = nullptr;
static constexpr size_t g_phase_dbg_bytes = 0;
#endif

static WinArgs win_args(const Ctx& C) {
  WinArgs P{};
  P.kind = C.ops->kind;
  P.sym = C.ops->sym;
  P.v0 = C.ops->v0;
  P.v1 = C.ops->v1;
  P.na = C.na;
  P.nb = C.nb;
  P.bgap = C.ops->b_gap;
  P.n_sym = C.n_sym;
  P.src_a = C.src_a;
  P.src_b = C.src_b;
  P.src_map = C.src_map;
  P.bnd = C.ws<i64>(B_BND);
  P.woff = C.ws<u32>(B_WOFF);
  P.meta = C.ws<ComposeMeta>(B_META);
  P.out_order = C.out->order;
  P.out_addr = C.out->addr;
  P.out_file = C.out->file;
  P.out_ctx = C.out->ctx;
  P.msym = C.ws<u32>(B_MSYM);
  P.tsrc = C.ws<i32>(B_TSRC);
  P.tsym = C.ws<u32>(B_TSYM);
  P.Rstr = C.ws<i32>(B_RSTR);
  P.wren = C.ws<u32>(B_WREN);
  P.wbnd = C.ws<u32>(B_WBND);
  P.cslot = C.ws<u32>(B_CSLOT);
  P.wcand = C.ws<u32>(B_WCAND);
  return P;
}

static WalkArgs walk_args(const Ctx& C, const smx_shard* sh) {
  WalkArgs Wk{};
  Wk.tsrc = C.ws<i32>(B_TSRC);
  Wk.tsym = C.ws<u32>(B_TSYM);
  Wk.v0 = C.ops->v0;
  Wk.wren = C.ws<u32>(B_WREN);
  Wk.wbnd = C.ws<u32>(B_WBND);
  Wk.meta = C.ws<ComposeMeta>(B_META);
  Wk.na_cap = (u64)C.na;
  Wk.nb_cap = (u64)C.nb;
  Wk.bgap = C.ops->b_gap;
  Wk.src_a = C.src_a;
  Wk.src_b = C.src_b;
  Wk.src_map = C.src_map;
  Wk.halo_dev = sh ? sh->halo_dev : nullptr;
  for (int b = 0; b < 2; ++b) {
    Wk.halo_sym[b] = sh ? sh->halo_sym[b] : nullptr;
    Wk.halo_cls[b] = sh ? sh->halo_cls[b] : nullptr;
    Wk.halo_src[b] = sh ? sh->halo_src[b] : nullptr;
    Wk.halo_n[b] = sh && sh->halo_sym[b] ? (u64)sh->halo_n[b] : 0;
    Wk.halo_more[b] = sh ? sh->halo_more[b] : 0;
  }
  // staging for k_replay_q's short regions: buffers of the sorting plans and of the
  // None-value move prefix, free while the walk runs
  Wk.stage = C.ws<u32>(B_RK2);
  Wk.sok = C.ws<u32>(B_RV2);
  Wk.stage_cap = RS_CONF ? (u64)(C.n > 0 ? C.n : 1) * 2 / (RS_CONF ? RS_W : 1) : 0;  // B_RK2: 8 bytes per op
  return Wk;
}

// DivergentRename walk (smx_walk.h): conflicts, skip bits, sorted skip list.
// Every size is read on the device from meta: no host sync.
static int launch_walk(const Ctx& C, const smx_shard* sh) {
  hipStream_t st = C.st;
  ComposeMeta* meta = C.ws<ComposeMeta>(B_META);
  const i64 n = C.n;
  u64* skipbits = C.ws<u64>(B_SKIPBITS);
  u32* skiplist = C.ws<u32>(B_SKIPLIST);
  u32* part = C.ws<u32>(B_PART);
  const u64 nskipw = (u64)SMX_CEIL_DIV(n, (i64)64) + 1;  // (cleared by k_boundary)
  const WalkArgs Wk = walk_args(C, sh);
  u32* cslot = C.ws<u32>(B_CSLOT);
  u32* wcand = C.ws<u32>(B_WCAND);
  u32* wtot = C.ws<u32>(B_WCANDB);
  u32* wcoff = C.ws<u32>(B_WCOFF);
  u32* cand = C.ws<u32>(B_CAND);
  u32* q = C.ws<u32>(B_Q);
  u32* pm = C.ws<u32>(B_PM);
  u32* nconf = C.ws<u32>(B_NCONF);
  u32* nreal = C.ws<u32>(B_NREAL);
  u32* coff = C.ws<u32>(B_COFF);
  // u64 counters of meta: the scans write their u32 totals into the low word
  // (little endian) of the zeroed fields
  u32* nconf32 = (u32*)&meta->n_conf_loc;
  u32* ncand32 = (u32*)&meta->n_cand;
  const u64* ncand_dev = &meta->n_cand;
  const i64 Wmax = max_windows(n);
#ifndef WALK_GSMALL
#define WALK_GSMALL 256  // (64 and 1024 measured the same on configs 2 and 3: profiles/r06/ab_c3_walk_grid.txt)
#endif
  const int gsmall = WALK_GSMALL;  // grid for loops over the (few) candidates
  hipLaunchKernelGGL(k_boundary, dim3(grid_for(Wmax)), dim3(BLOCK), 0, st, Wk, meta, cslot, wcand, wtot, skipbits,
                     nskipw);
  if (sh && (sh->in_d > 0 || sh->in_state_dev))
    hipLaunchKernelGGL(k_replay_in, dim3(1), dim3(1), 0, st, Wk, (int)sh->in_ahead, (u32)sh->in_d,
                       (const i64*)sh->in_state_dev, meta, C.out->conflicts, (u64)C.out->conflict_cap, skiplist,
                       skipbits);
  // (one k_scan1 block over the window counts measured slower on config 3: walk 0.165 ->
  // 0.185 ms, round 3; small merges are launch-bound: one block)
  if (Wmax <= WALK_CC_FUSED_MAXW) {
    hipLaunchKernelGGL(k_cand_scan_compact, dim3(1), dim3(S1_NT), 0, st, Wk, wtot, wcoff, (u64)Wmax, ncand32, cslot,
                       cand);
  } else {
    if (Wmax <= WALK_SCAN1_MAXW)
      hipLaunchKernelGGL(k_scan1<OpSum>, dim3(1), dim3(S1_NT), 0, st, wtot, wcoff, (const u64*)&meta->n_win,
                         (u64)Wmax, ncand32);
    else
      HIP_TRY((scan_excl<OpSum, u32, u32>(wtot, wcoff, Wmax, &meta->n_win, part, ncand32, st)));
    hipLaunchKernelGGL(k_cand_compact, dim3(grid_for(Wmax)), dim3(BLOCK), 0, st, Wk, cslot, wcoff, ncand_dev, cand);
  }
  if (n <= WALK_FUSED_MAXN) {  // small merges: max scan, clusters and sum scan in one block
    hipLaunchKernelGGL(k_replay_q, dim3(gsmall), dim3(BLOCK), 0, st, Wk, cand, meta, q, nconf);
    hipLaunchKernelGGL(k_cluster_fused, dim3(1), dim3(S1_NT), 0, st, Wk, cand, q, pm, nconf, meta, nreal, coff,
                       (u64)n, nconf32);
  } else {
    hipLaunchKernelGGL(k_replay_q, dim3(gsmall), dim3(BLOCK), 0, st, Wk, cand, meta, q, nconf);
    hipLaunchKernelGGL(k_scan1<OpMax>, dim3(1), dim3(S1_NT), 0, st, q, pm, ncand_dev, (u64)n, (u32*)nullptr);
    hipLaunchKernelGGL(k_cluster, dim3(gsmall), dim3(BLOCK), 0, st, Wk, cand, q, pm, nconf, meta, nreal);
    hipLaunchKernelGGL(k_scan1<OpSum>, dim3(1), dim3(S1_NT), 0, st, nreal, coff, ncand_dev, (u64)n, nconf32);
  }
  hipLaunchKernelGGL(k_replay_write, dim3(gsmall), dim3(BLOCK), 0, st, Wk, cand, nreal, coff, meta,
                     C.out->conflicts, (u64)C.out->conflict_cap, skiplist, skipbits);
  HIP_TRY(hipGetLastError());
  return SMX_OK;
}

static TbArgs tb_args(const Ctx& C) {
  TbArgs A{};
  A.msym = C.ws<u32>(B_MSYM);
  A.tsym = C.ws<u32>(B_TSYM);
  A.skipbits = C.ws<u64>(B_SKIPBITS);
  A.mv_addr = C.out->addr;
  A.mv_file = C.out->file;
  A.Rstr = C.ws<i32>(B_RSTR);
  A.meta = C.ws<ComposeMeta>(B_META);
  A.ncap = (u64)C.n;
  A.width = 1u;
  A.nbk = 1u;
  A.smax = (u32)(C.n_sym - 1);
  return A;
}

// Bucket geometry of the per-symbol tables: the bucketed path when it returns true.
static bool tb_geometry(const Ctx& C, u64* width_o, u64* nbk_o) {
  u64 width = SMX_CEIL_DIV((u64)C.n_sym, (u64)TB_NBK_TGT);
  if (width < 1) width = 1;
  if (width > TB_WIDTH) width = TB_WIDTH;
  *width_o = width;
  *nbk_o = SMX_CEIL_DIV((u64)C.n_sym, width);
  return *nbk_o <= TB_MAXBK;
}

// The table records bucketed with every rename kept (k_tb_scatter keep_skip): it needs
// only the window outputs, so it can run before or beside the walk; k_tb_unskip then
// applies the walk's skips.  No-op off the bucketed path.
static int launch_tb_prescatter(const Ctx& C) {
  u64 width, nbk;
  if (!tb_geometry(C, &width, &nbk)) return SMX_OK;
  TbArgs A = tb_args(C);
  A.width = (u32)width;
  A.nbk = (u32)nbk;
  A.keep_skip = 1u;
  hipLaunchKernelGGL(k_tb_scatter, dim3((int)SMX_CEIL_DIV((u64)C.n, (u64)TB_TILE)), dim3(TB_NT), 0, C.st, A,
                     C.ws<u32>(B_TBHIST), C.ws<u32>(B_REC));
  HIP_TRY(hipGetLastError());
  return SMX_OK;
}

// Per-symbol last writers.  part == nullptr: the final-state table fin (packed
// when the value widths allow); otherwise this shard's partial tables.  prescattered:
// launch_tb_prescatter already bucketed the records (then only the skips and the
// reduce run here).
static int launch_tables(const Ctx& C, void* part_tab, u32 tag, int tagbits, bool* bucketed,
                         bool prescattered = false) {
  hipStream_t st = C.st;
  const i64 n = C.n;
  int4* fin = C.ws<int4>(B_FIN);
  *bucketed = false;
  const i64 n_sym = C.n_sym;
  TbArgs A = tb_args(C);
  u64 width, nbk;
  if (tb_geometry(C, &width, &nbk)) {
    *bucketed = true;
    A.width = (u32)width;
    A.nbk = (u32)nbk;
    const int nblk = (int)SMX_CEIL_DIV((u64)n, (u64)TB_TILE);
    u32* lst = C.ws<u32>(B_TBHIST);
    u32* rec = C.ws<u32>(B_REC);
    if (prescattered) {
      A.keep_skip = 1u;
      hipLaunchKernelGGL(k_tb_unskip, dim3(1024), dim3(BLOCK), 0, st, A, lst, rec, C.ws<u32>(B_SKIPLIST));
    } else {
      hipLaunchKernelGGL(k_tb_scatter, dim3(nblk), dim3(TB_NT), 0, st, A, lst, rec);
    }
    hipLaunchKernelGGL(k_tb_reduce, dim3(nbk), dim3(TBR_NT), 0, st, A, lst, rec, n_sym, fin,
                       PartTab{part_tab, tag, tagbits, C.ws<ComposeMeta>(B_META)});
  } else {
    // very large symbol spaces: device-scope atomics on the packed keys
    u32* tabA = C.ws<u32>(B_TABA);
    u32* tabF = C.ws<u32>(B_TABF);
    u32* tabR = C.ws<u32>(B_TABR);
    int rc;
    if ((rc = zero_async(tabA, (size_t)n_sym * 4, st)) || (rc = zero_async(tabF, (size_t)n_sym * 4, st)) ||
        (rc = zero_async(tabR, (size_t)n_sym * 4, st)))
      return rc;
    hipLaunchKernelGGL(k_tab_atomic, dim3(grid_for(n)), dim3(BLOCK), 0, st, A, tabA, tabF, tabR);
    hipLaunchKernelGGL(k_finalize, dim3(grid_for(n_sym)), dim3(BLOCK), 0, st, A, tabA, tabF, tabR, n_sym, fin,
                       PartTab{part_tab, tag, tagbits, C.ws<ComposeMeta>(B_META)});
  }
  HIP_TRY(hipGetLastError());
  return SMX_OK;
}

static int launch_emit(const Ctx& C, bool packable, const smx_shard* sh) {
  hipStream_t st = C.st;
  ComposeMeta* meta = C.ws<ComposeMeta>(B_META);
  const i64 n = C.n;
  EmitArgs E{C.ws<i32>(B_TSRC), C.ws<u32>(B_TSYM), C.ws<u64>(B_SKIPBITS), C.ws<u32>(B_SKIPLIST),
             C.ws<int4>(B_FIN), meta, (u64)n, (u32)(C.n_sym - 1), packable ? 1 : 0, (u64)C.na, C.src_a,
             C.src_b, C.src_map, C.out->order, C.out->addr, C.out->file, C.out->ctx, C.out->counts, sh ? 0 : 1,
             sh ? nullptr : C.hrec, C.hseq};
  const i64 ewaves = SMX_CEIL_DIV(n, (i64)EMIT_WT);
  const bool al16 = ((uintptr_t)C.out->order | (uintptr_t)C.out->addr | (uintptr_t)C.out->file |
                     (uintptr_t)C.out->ctx) % 16 == 0;
  if (al16)
    hipLaunchKernelGGL(k_emit4, dim3(SMX_CEIL_DIV(ewaves, (i64)NWAVES)), dim3(BLOCK), 0, st, E);
  else
    hipLaunchKernelGGL(k_emit, dim3(SMX_CEIL_DIV(ewaves, (i64)NWAVES)), dim3(BLOCK), 0, st, E);
  HIP_TRY(hipGetLastError());
  return SMX_OK;
}

// Diagnostic knobs (SMX_ABLATE, SMX_WIN_TGT, SMX_TB_SERIAL, SMX_SIDE_CUS) are read
// from the environment only in a diagnostic build (-DSMX_DIAG=1, tools/build_variants.sh);
// the release library always takes the compiled defaults, so no environment variable
// can change what smx_compose computes.
#if SMX_DIAG
static int knob(const char* name, int dflt) {
  const char* v = getenv(name);
  return v && *v ? atoi(v) : dflt;
}
#else
static constexpr int knob(const char*, int dflt) { return dflt; }
#endif

// A second stream (and its fork/join events) for the table scatter, which runs beside
// the walk: the walk is a chain of small, latency-bound launches that leaves most of
// the chip idle.  One per (device, caller stream), created on first use, so that calls
// on distinct streams never share one (and a graph capture of one caller's stream
// pulls in only that caller's side stream).  `mu` is held from the fork record to the
// join wait: two threads that share a caller stream cannot interleave their records.
// The fork/join is by events, so it also works inside a HIP graph capture.
struct SideStream {
  std::mutex mu;
  int dev = -1;
  hipStream_t caller = nullptr;
  hipStream_t s = nullptr;
  hipEvent_t fork = nullptr, join = nullptr;
};
#define SIDE_MAX 256  // distinct caller streams with a side stream; beyond: no overlap
static std::mutex g_side_mu;
static SideStream* g_side[SIDE_MAX];
static int g_nside = 0;

// *out = the side stream of (current device, caller), or nullptr when the table is
// full (the caller then runs the tables on its own stream).
static int side_stream(hipStream_t caller, SideStream** out) {
  *out = nullptr;
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  std::lock_guard<std::mutex> g(g_side_mu);
  for (int i = 0; i < g_nside; ++i)
    if (g_side[i]->dev == dev && g_side[i]->caller == caller) {
      *out = g_side[i];
      return SMX_OK;
    }
  if (g_nside == SIDE_MAX) return SMX_OK;
  SideStream* S = new SideStream;
  S->dev = dev;
  S->caller = caller;
  // (the lowest stream priority for it measured the same, profiles/r02_k/side_prio_ab.txt)
  // SMX_SIDE_CUS = k > 0 (diagnostic builds): the side stream runs on the first k CUs
  // only (measured slower, profiles/r02_k/side_cumask_ab.txt)
  int ncu = 0;
  HIP_TRY(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev));
  const int k = knob("SMX_SIDE_CUS", 0);
  if (k > 0 && k < ncu) {
    std::vector<uint32_t> mask((size_t)(ncu + 31) / 32, 0u);
    for (int i = 0; i < k; ++i) mask[(size_t)i / 32] |= 1u << (i % 32);
    HIP_TRY(hipExtStreamCreateWithCUMask(&S->s, (uint32_t)mask.size(), mask.data()));
  } else {
    HIP_TRY(hipStreamCreateWithFlags(&S->s, hipStreamNonBlocking));
  }
  // (device-scope events: both streams are on this device.  A default event's record
  // also fences at system scope -- an L2 write-back the next kernel on the recording
  // stream waits behind: ~11 us before k_boundary and ~6 us before the reduce on config 3,
  // profiles/r06/c3_timeline_start.txt)
  const unsigned evf = hipEventDisableTiming | hipEventDisableSystemFence;
  HIP_TRY(hipEventCreateWithFlags(&S->fork, evf));
  HIP_TRY(hipEventCreateWithFlags(&S->join, evf));
  g_side[g_nside++] = S;
  *out = S;
  return SMX_OK;
}

#ifndef SMX_TB_UNSKIP_MAXN
#define SMX_TB_UNSKIP_MAXN (1 << 22)  // up to: k_tb_reduce reads the skip bits; above: k_tb_unskip
#endif
#ifndef SMX_TB_OVERLAP_MIN
#define SMX_TB_OVERLAP_MIN (1 << 18)  // ops (config 2: 0.1746 -> 0.1724 ms with the overlap, profiles/r05_x/c2_overlap_ab.txt; graph replay makes the fork/join cheap)
#endif

// Walk, tables, emit of a single merge.  The bucketed tables' scatter keeps every
// rename and runs on the side stream while the walk runs; k_tb_unskip then kills
// the records of the renames the walk skipped (compose.py:60-70: a skipped rename
// never enters rename_chain) before the reduce.
static int launch_tail(const Ctx& C) {
  u64 width, nbk;
  const bool geo = tb_geometry(C, &width, &nbk);
  // the smallest merges are launch-bound: below SMX_TB_OVERLAP_MIN the fork/join costs more than the overlap saves
  SideStream* S = nullptr;
  if (geo && C.n >= SMX_TB_OVERLAP_MIN && !knob("SMX_TB_SERIAL", 0)) {
    int rc = side_stream(C.st, &S);
    if (rc) return rc;
  }
  std::unique_lock<std::mutex> own;  // fork record .. join wait
  int rc;
  hipStream_t st = C.st;
  TbArgs A{};
  u32* lst = C.ws<u32>(B_TBHIST);
  u32* rec = C.ws<u32>(B_REC);
  if (S) {  // fork: the scatter on the side stream
    own = std::unique_lock<std::mutex>(S->mu);
    A = tb_args(C);
    A.width = (u32)width;
    A.nbk = (u32)nbk;
    // small merges: no k_tb_unskip launch, k_tb_reduce tests the skip bits of the renames
    A.keep_skip = C.n <= SMX_TB_UNSKIP_MAXN ? 2u : 1u;
    const int nblk = (int)SMX_CEIL_DIV((u64)C.n, (u64)TB_TILE);
    HIP_TRY(hipEventRecord(S->fork, st));
    HIP_TRY(hipStreamWaitEvent(S->s, S->fork, 0));
    hipLaunchKernelGGL(k_tb_scatter, dim3(nblk), dim3(TB_NT), 0, S->s, A, lst, rec);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(S->join, S->s));
  }
  C.tm->begin(ST_WALK);
  if ((rc = launch_walk(C, nullptr))) {
    if (S) (void)hipStreamWaitEvent(st, S->join, 0);  // never leave the side stream unjoined
    return rc;
  }
  C.tm->end(ST_WALK);
  if (S) HIP_TRY(hipStreamWaitEvent(st, S->join, 0));
  C.tm->begin(ST_TABLES);
  bool bucketed = true;
  if (S) {  // the scattered records: the walk's skips, then the reduce
    if (A.keep_skip == 1u)
      hipLaunchKernelGGL(k_tb_unskip, dim3(1024), dim3(BLOCK), 0, st, A, lst, rec, C.ws<u32>(B_SKIPLIST));
    hipLaunchKernelGGL(k_tb_reduce, dim3(nbk), dim3(TBR_NT), 0, st, A, lst, rec, C.n_sym, C.ws<int4>(B_FIN),
                       PartTab{nullptr, 0u, 0, nullptr});
    HIP_TRY(hipGetLastError());
  } else if ((rc = launch_tables(C, nullptr, 0, 0, &bucketed))) {
    return rc;
  }
  C.tm->end(ST_TABLES);
  C.tm->begin(ST_EMIT);
  if ((rc = launch_emit(C, bucketed, nullptr))) return rc;
  C.tm->end(ST_EMIT);
  return SMX_OK;
}

// Presorted plan: branch logs with non-decreasing timestamps (what lift.ts
// emits).  Speculative: k_window_f verifies the layout and flags f_fail.

// early (optional, not inside a graph capture): k_khist raises early->flag[0] when a
// timestamp group is longer than a window (the normal windows cannot hold the log) and
// flag[1] on an invalid kind; early->ev is recorded right behind k_khist, so the host
// knows while k_fpart and the column scans run, and launches the windows that hold the
// groups (run_presorted's Deferred).  (Off the normal level, k_fpart raises flag[0] and
// the event follows it.)
struct EarlyFail {
  u32* flag_host = nullptr;
  u32* flag_dev = nullptr;
  hipEvent_t ev = nullptr;
};
// Presorted window sizes: normal, wide (timestamp groups no normal window holds).
// (A small level, 512-op windows for merges up to some size, measured slower: config 2's
// window stage 0.048 -> 0.218 ms, profiles/r04_h/ab_c2.txt; removed.)
enum WinLevel { WL_NORMAL, WL_WIDE };
static i64 level_cap(int lv) { return lv == WL_WIDE ? WF_WIDE_CAP : WF_CAP; }
// (SMX_FIRST_WIDE, diagnostic builds: start at the wide windows, so that SMX_ABLATE's
// phase exits reach the wide instance)
static int first_level(const Ctx& C) { return knob("SMX_FIRST_WIDE", 0) ? WL_WIDE : WL_NORMAL; }
static i64 first_tgt(const Ctx& C) {
  return knob("SMX_WIN_TGT", first_level(C) == WL_WIDE ? WF_WIDE_CAP : WIN_TGT);
}

// One k_window_f instance over P.W windows; the release instances of one capacity.
template <int CAP, int NT, bool DBG, bool MAP>
static void launch_window_f(const WinArgs& P, hipStream_t st) {
  hipLaunchKernelGGL((k_window_f<CAP, NT, DBG, MAP>), dim3(P.W), dim3(NT), 0, st, P);
}
template <int CAP, int NT>
static void launch_window_level(const WinArgs& P, hipStream_t st) {
  if (P.src_map) launch_window_f<CAP, NT, false, true>(P, st);
  else launch_window_f<CAP, NT, false, false>(P, st);
}

// The presorted windows over the boundaries k_fpart left (W windows).
static int launch_presorted_windows(const Ctx& C, i64 W, i64 CM, int level) {
  const bool wide = level == WL_WIDE;
  hipStream_t st = C.st;
  WinArgs P = win_args(C);
  P.cpre = C.ws<u32>(B_CCNT);
  P.CM = CM;
  P.kts = C.ops->ts;
  P.khi = C.ops->oid_hi;
  P.klo = C.ops->oid_lo;
  P.perm = nullptr;
  P.W = W;
  P.ablate = knob("SMX_ABLATE", 0);
  const int stage = wide ? ST_WINDOW_WIDE : ST_WINDOW;
  C.tm->begin(stage);
#if SMX_DIAG
  if (g_phase_dbg && !P.src_map && (size_t)W * WF_NSTAMP * 8 <= g_phase_dbg_bytes) {
    P.dbg = (u64*)g_phase_dbg;
    if (wide) launch_window_f<WF_WIDE_CAP, WF_WIDE_NT, true, false>(P, st);
    else launch_window_f<WF_CAP, WF_NT, true, false>(P, st);
  } else
#endif
  if (wide) launch_window_level<WF_WIDE_CAP, WF_WIDE_NT>(P, st);
  else launch_window_level<WF_CAP, WF_NT>(P, st);
  HIP_TRY(hipGetLastError());
  C.tm->end(stage);
  return SMX_OK;
}

// wide: WF_WIDE_CAP-op windows on WF_WIDE_NT threads (one per CU) for logs whose
// equal-timestamp groups no WF_CAP window holds (config 5: 8192-op groups).
// With `early` at the normal level (the synchronous merge): k_khist makes the long-group
// test and early->ev is recorded behind it; k_fpart and the column scans are enqueued
// for either outcome (normal boundaries, or the wide plan's after F_LONG: LongW), and the
// windows are left to the caller (*defer), which launches the normal or the wide ones
// once the host has read the verdict.
struct Deferred {
  bool on = false;
  i64 W = 0, W_w = 0, CM = 0;
};

// Geometry of a presorted attempt at `level`: tgt clamped to [WIN_TGT_MIN, the level's
// capacity] and chunk-aligned (k_fpart's sampled first level searches diagonals that are
// multiples of CH), W windows of at most D chunks, CM count columns per kind, and the
// branches' chunk samples in B_SMP.
struct PreGeo {
  i64 tgt, W, D, CM;
  u64 *sA, *sB;
};
static PreGeo presorted_geometry(const Ctx& C, i64 tgt, int level) {
  const i64 cap = level_cap(level);
  tgt = std::min(std::max(tgt, (i64)WIN_TGT_MIN), cap);
  tgt -= tgt % CH;
  u64* sA = C.ws<u64>(B_SMP);
  return PreGeo{tgt, SMX_CEIL_DIV(C.n, tgt), cap / CH, SMX_CEIL_DIV(std::max(C.na, C.nb), (i64)CH) + 1, sA,
                sA + SMX_CEIL_DIV(C.na, (i64)CH) + 1};
}

static int run_presorted(const Ctx& C, i64 tgt, const EarlyFail* early = nullptr, int level = WL_NORMAL,
                         Deferred* defer = nullptr) {
  hipStream_t st = C.st;
  ComposeMeta* meta = C.ws<ComposeMeta>(B_META);
  i64* bnd = C.ws<i64>(B_BND);
  C.tm->begin(ST_PLAN);
  static_assert(sizeof(ComposeMeta) % 4 == 0, "meta is zeroed by words");
  const PreGeo G = presorted_geometry(C, tgt, level);
  const i64 W = G.W, CM = G.CM;
  // (a single-pass look-back column scan fused with k_fpart measured slower on config 3:
  // plan 0.133 -> 0.157 ms -- the blocks' tickets and status round trips, profiles/r06)
  const bool cs_small = CM <= CS_SMALL_CM;
  {
    const int rc = zero_async(meta, sizeof(ComposeMeta), st);
    if (rc) return rc;
  }
  const i64 nchunk = SMX_CEIL_DIV(C.na, (i64)CH) + SMX_CEIL_DIV(C.nb, (i64)CH);
  u32* ccnt = C.ws<u32>(B_CCNT);
  const bool lmode = early && defer && level == WL_NORMAL;
  LongW lw{};
  if (lmode) {  // (the first wide attempt of order_fallbacks)
    const PreGeo Gw = presorted_geometry(C, level_cap(WL_WIDE), WL_WIDE);
    lw.tgt_w = Gw.tgt;
    lw.W_w = Gw.W;
    lw.D_w = Gw.D;
  }
  hipLaunchKernelGGL(k_khist, dim3(SMX_CEIL_DIV(nchunk, (i64)CH_PER_BLOCK * KH_R)), dim3(KH_NT), 0, st,
                     C.ops->kind, C.ops->ts, C.na, C.nb, C.ops->b_gap, CM, ccnt, G.sA, G.sB, meta,
                     early ? early->flag_dev : nullptr, lmode ? G.D : (i64)0);
  if (lmode) HIP_TRY(hipEventRecord(early->ev, st));  // (k_khist's verdict)
  const i64 nfp = SMX_CEIL_DIV(W + 1, (i64)BLOCK);   // (>= the wide plan's W_w + 1 boundaries)
  const bool fused = cs_small && !early;  // small merges: k_fpart and k_cscan_small in one launch
  if (fused)
    hipLaunchKernelGGL(k_fpart_cscan, dim3(nfp + 2 * SMX_N_KINDS), dim3(BLOCK), 0, st, C.ops->ts,
                       C.ops->ts + C.na + C.ops->b_gap, G.sA, G.sB, C.na, C.nb, W, G.tgt, G.D, bnd, meta,
                       (u32*)nullptr, ccnt, CM, nfp);
  else
    hipLaunchKernelGGL(k_fpart, dim3(nfp), dim3(BLOCK), 0, st, C.ops->ts, C.ops->ts + C.na + C.ops->b_gap, G.sA,
                       G.sB, C.na, C.nb, W, G.tgt, G.D, bnd, meta, (early && !lmode) ? early->flag_dev : nullptr, lw);
  if (early && !lmode) HIP_TRY(hipEventRecord(early->ev, st));
  const u64 nwin_long = lmode ? (u64)lw.W_w : 0ull;
  if (fused) {
    // (k_fpart_cscan scanned the columns)
  } else if (cs_small) {
    hipLaunchKernelGGL(k_cscan_small, dim3(2 * SMX_N_KINDS), dim3(BLOCK), 0, st, ccnt, C.na, C.nb, CM, meta, (u64)W,
                       nwin_long);
  } else {
    const i64 NT = SMX_CEIL_DIV(CM, (i64)CS_TILE);
    u32* tsum = C.ws<u32>(B_TSUM);
    hipLaunchKernelGGL(k_cscan_up, dim3(NT, 2 * SMX_N_KINDS), dim3(BLOCK), 0, st, ccnt, C.na, C.nb, CM, NT, tsum,
                       meta);
    hipLaunchKernelGGL(k_cscan_mid, dim3(2 * SMX_N_KINDS), dim3(BLOCK), 0, st, tsum, C.na, C.nb, CM, NT, ccnt,
                       meta, (u64)W, nwin_long);
    hipLaunchKernelGGL(k_cscan_down, dim3(NT, 2 * SMX_N_KINDS), dim3(BLOCK), 0, st, ccnt, C.na, C.nb, CM, NT,
                       tsum, meta);
  }
  HIP_TRY(hipGetLastError());
  C.tm->end(ST_PLAN);
  if (lmode) {
    *defer = Deferred{true, W, lw.W_w, CM};
    return SMX_OK;
  }
  return launch_presorted_windows(C, W, CM, level);
}

// k_fpart's long-group verdict (f_fail == F_LONG) is given before any window runs, so
// the plan's chunk counts, prefixes and bases stand: only the boundaries and the windows
// are redone, at the wide capacity.
__global__ void k_plan_rearm(ComposeMeta* meta, u64 nwin) {
  if (meta->f_fail == F_LONG) meta->f_fail = 0;
  meta->n_win = nwin;
}
// (which is why the chunk scans never leave on a failed plan: they write base[] and the
// prefixes even when k_fpart flagged F_LONG, or the wide windows would read stale prefixes)
static int run_presorted_rewide(const Ctx& C, i64 tgt, int level = WL_WIDE) {
  hipStream_t st = C.st;
  ComposeMeta* meta = C.ws<ComposeMeta>(B_META);
  const PreGeo G = presorted_geometry(C, tgt, level);
  C.tm->begin(ST_PLAN);
  hipLaunchKernelGGL(k_plan_rearm, dim3(1), dim3(1), 0, st, meta, (u64)G.W);
  hipLaunchKernelGGL(k_fpart, dim3(SMX_CEIL_DIV(G.W + 1, (i64)BLOCK)), dim3(BLOCK), 0, st, C.ops->ts,
                     C.ops->ts + C.na + C.ops->b_gap, G.sA, G.sB, C.na, C.nb, G.W, G.tgt, G.D, C.ws<i64>(B_BND), meta,
                     (u32*)nullptr, LongW{});
  HIP_TRY(hipGetLastError());
  C.tm->end(ST_PLAN);
  return launch_presorted_windows(C, G.W, G.CM, level);
}

#include "smx_segsort.h"

// Host wait for a stream: the blocking sync.  No spin on hipStreamQuery before it for the
// merges: spinning measured slower there (config 2 0.161 -> 0.166 ms,
// profiles/r05_x/spin_ab.txt), while the RGA call gains from it (smx_rga.hip RGA_SPIN_US).
static hipError_t stream_wait(hipStream_t st) { return hipStreamSynchronize(st); }

// GEN_SEG: when the segmented sort cannot order this log it flags seg_over and f_fail
// bit 3; every kernel after it leaves at once, and the caller reads seg_over from the
// meta after the tail.
static int run_generic(const Ctx& C, int mode) {
  hipStream_t st = C.st;
  ComposeMeta* meta = C.ws<ComposeMeta>(B_META);
  i64* bnd = C.ws<i64>(B_BND);
  u32* wcnt = C.ws<u32>(B_WCNT);
  u32* woff = C.ws<u32>(B_WOFF);
  const i64 na = C.na, nb = C.nb, n = C.n;
  u64* sts = C.ws<u64>(B_STS);
  u64* shi = C.ws<u64>(B_SHI);
  u64* slo = C.ws<u64>(B_SLO);
  u32* perm = C.ws<u32>(B_PERM);
  C.tm->begin(ST_GSORT);
  HIP_TRY(hipMemsetAsync(meta, 0, sizeof(ComposeMeta), st));
  if (mode == GEN_SEG) {
    C.tm->begin(ST_SEGSORT);
    for (int side = 0; side < 2; ++side) {
      const i64 off = side ? na : 0, cnt = side ? nb : na;
      if (cnt == 0) continue;
      hipLaunchKernelGGL(k_segsort, dim3(SMX_CEIL_DIV(cnt, (i64)SEG_H)), dim3(SEG_NT), 0, st, C.ops->ts + off,
                         C.ops->oid_hi + off, C.ops->oid_lo + off, cnt, (u32)off, sts + off, shi + off, slo + off,
                         perm + off, meta);
    }
    C.tm->end(ST_SEGSORT);
  } else {
    const bool with_lo = mode == GEN_RADIX_LO;
    hipLaunchKernelGGL(k_meta_init, dim3(1), dim3(1), 0, st, meta);
    hipLaunchKernelGGL(k_keymask, dim3(grid_for(n, BLOCK * 8)), dim3(BLOCK), 0, st, C.ops->ts, C.ops->oid_hi,
                       C.ops->oid_lo, na, n, meta);
    ComposeMeta hm;
    HIP_TRY(hipMemcpyAsync(&hm, meta, sizeof(ComposeMeta), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    RadixTemp rt{C.ws<u64>(B_RK2), C.ws<u32>(B_RV2), C.ws<u32>(B_RHIST), C.ws<u32>(B_PART)};
    const u64* words[3] = {C.ops->oid_lo, C.ops->oid_hi, C.ops->ts};
    const int w0 = with_lo ? 0 : 1;
    for (int side = 0; side < 2; ++side) {
      const i64 off = side ? na : 0, cnt = side ? nb : na;
      if (cnt == 0) continue;
      u64* key = C.ws<u64>(B_RKEY) + off;
      u32* val = perm + off;
      for (int wi = w0; wi < 3; ++wi) {
        const int q = 2 - wi;  // meta order: 0 = ts, 1 = hi, 2 = lo
        const u64 varying = hm.key_or[side][q] ^ hm.key_and[side][q];
        int shifts[8], ns = 0;
        for (int dgt = 0; dgt < 8; ++dgt)
          if ((varying >> (8 * dgt)) & 0xffull) shifts[ns++] = 8 * dgt;
        if (wi == w0) {
          hipLaunchKernelGGL(k_gather_init, dim3(grid_for(cnt)), dim3(BLOCK), 0, st, words[wi] + off, key, val,
                             cnt);
          if (off)  // values are op indices of A||B
            hipLaunchKernelGGL(k_offset, dim3(grid_for(cnt)), dim3(BLOCK), 0, st, val, cnt, (u32)off);
        } else {
          hipLaunchKernelGGL(k_gather, dim3(grid_for(cnt)), dim3(BLOCK), 0, st, words[wi], val, key, cnt);
        }
        if (ns) HIP_TRY(radix_sort_pairs(key, val, cnt, shifts, ns, rt, st));
      }
      // the last key word is ts, so the sorted keys are ts in sorted order already
      HIP_TRY(hipMemcpyAsync(sts + off, key, (size_t)cnt * 8, hipMemcpyDeviceToDevice, st));
      hipLaunchKernelGGL(k_gather2, dim3(grid_for(cnt)), dim3(BLOCK), 0, st, C.ops->oid_hi, C.ops->oid_lo, val,
                         shi + off, slo + off, cnt);
    }
    if (!with_lo) hipLaunchKernelGGL(k_dupcheck, dim3(grid_for(n)), dim3(BLOCK), 0, st, sts, shi, na, n, meta);
  }
  const i64 W = SMX_CEIL_DIV(n, (i64)WG_CAP);
  hipLaunchKernelGGL(k_gpart, dim3(SMX_CEIL_DIV(W + 1, (i64)BLOCK)), dim3(BLOCK), 0, st, sts, shi, slo, na, nb,
                     W, bnd, meta);
  hipLaunchKernelGGL(k_wcount, dim3(W), dim3(WC_NT), 0, st, C.ops->kind, C.ops->v0, C.ops->v1, perm, bnd, na, W,
                     wcnt, meta);
  hipLaunchKernelGGL(k_wscan, dim3(NCNT), dim3(BLOCK), 0, st, wcnt, woff, W, meta);
  hipLaunchKernelGGL(k_bases, dim3(1), dim3(1), 0, st, meta, (u64)W);
  HIP_TRY(hipGetLastError());
  C.tm->end(ST_GSORT);
  WinArgs P = win_args(C);
  P.kts = sts;
  P.khi = shi;
  P.klo = slo;
  P.perm = perm;
  P.W = W;
  P.ablate = 0;
  C.tm->begin(ST_WINDOW_G);
  hipLaunchKernelGGL(k_window_g, dim3(W), dim3(WG_NT), 0, st, P);
  HIP_TRY(hipGetLastError());
  C.tm->end(ST_WINDOW_G);
  return SMX_OK;
}

// The meta block comes back through a pinned staging buffer (one per host thread): a
// DMA, not the runtime's staged copy into pageable memory.
struct PinnedMeta {  // freed when its host thread exits (thread-pool callers)
  ComposeMeta* p = nullptr;
  ~PinnedMeta() {
    if (p) (void)hipHostFree(p);
  }
};
static int read_meta(const Ctx& C, ComposeMeta* hm) {
  static thread_local PinnedMeta holder;
  ComposeMeta*& pinned = holder.p;
  if (!pinned) HIP_TRY(hipHostMalloc((void**)&pinned, sizeof(ComposeMeta), hipHostMallocDefault));
  HIP_TRY(hipMemcpyAsync(pinned, C.ws<ComposeMeta>(B_META), sizeof(ComposeMeta), hipMemcpyDeviceToHost, C.st));
  HIP_TRY(stream_wait(C.st));
  std::memcpy(hm, pinned, sizeof(ComposeMeta));
  return SMX_OK;
}

static int check_args(const smx_ops* ops, const smx_compose_out* out, void* ws, size_t ws_bytes, Layout* L) {
  const i64 na = ops->n_a, nb = ops->n_b, n = na + nb, n_sym = ops->n_sym;
  if (na < 0 || nb < 0 || n_sym < 0) return set_err(SMX_E_ARG, "negative size");
  if (n >= (i64)0x7fffffff) return set_err(SMX_E_ARG, "n_a + n_b must be < 2^31");
  if (n_sym > (i64)SYM_MASK + 1) return set_err(SMX_E_ARG, "n_sym must be <= 2^30");
  if (!out || !out->counts) return set_err(SMX_E_ARG, "null output");
  if (n == 0) return SMX_OK;
  if (!ops->kind || !ops->ts || !ops->oid_hi || !ops->oid_lo || !ops->sym || !ops->v0 || !ops->v1 ||
      !out->order || !out->addr || !out->file || !out->ctx || (!out->conflicts && out->conflict_cap > 0))
    return set_err(SMX_E_ARG, "null input/output pointer");
  if (n_sym < 1) return set_err(SMX_E_ARG, "n_sym must be >= 1");
  if (ops->b_gap < 0) return set_err(SMX_E_ARG, "b_gap must be >= 0");
  if (out->conflict_cap < 0) return set_err(SMX_E_ARG, "conflict_cap must be >= 0");
  *L = layout(na, nb, n_sym);
  if (!ws || ws_bytes < L->total)
    return set_err(SMX_E_WORKSPACE, "workspace too small: need " + std::to_string(L->total));
  return SMX_OK;
}

// The plan the last compose on this thread used (smx_last_plan).
static thread_local int g_plan = SMX_PLAN_PRESORTED;

// One attempt at the T order: the plan, the tail (walk, tables, emit) behind it when
// `tail` -- every tail kernel is a no-op if the plan flagged itself as failed -- and
// the meta it left (hm): one host wait.
template <typename Plan>
static int attempt(const Ctx& C, bool tail, ComposeMeta* hm, Plan&& plan) {
  int rc;
  if ((rc = plan())) return rc;
  if (tail && (rc = launch_tail(C))) return rc;
  return read_meta(C, hm);
}

// After a presorted attempt with target window size tgt (hm: the meta it left):
// a window that overflows LDS (dense timestamp ties) retries with smaller windows;
// a log that is not timestamp-ordered goes to the generic plan when allowed.  The
// tail (walk, tables, emit) is launched behind each plan when `tail`.
// require_ordered (a sharded range slice): a slice whose timestamps decrease must fail
// loudly -- the radix plan would order it locally, not across the shards -- so it is
// refused when the window kernel (f_fail bit 0) or the segmented sort (SEG_DECREASE)
// saw a decrease.  (k_fpart's early verdict, F_LONG, can hide bit 0: then the wide
// windows or the segmented sort report the decrease themselves.)
static int order_fallbacks(const Ctx& C, bool allow_generic, bool tail, ComposeMeta* hm, i64 tgt,
                           bool require_ordered = false) {
  int rc;
  auto unordered = [&]() {
    return set_err(SMX_E_ARG, "sharded merge needs timestamp-ordered branch logs in every shard");
  };
  g_plan = SMX_PLAN_PRESORTED;
  while (hm->f_fail == 2 && !hm->bad_sym && tgt > WIN_TGT_MIN) {  // dense groups: smaller windows
    tgt = (tgt / 2) / CH * CH;
    if ((rc = attempt(C, tail, hm, [&] { return run_presorted(C, tgt); }))) return rc;
  }
  // ordered logs whose equal-timestamp groups no WF_CAP window holds (F_LONG or 6, or 2 at
  // the smallest windows): the wide windows, from their full capacity down (a window
  // holds its target plus the group its end snaps back over; at full capacity each of
  // config 5's windows is one 8192-op group, and no window is empty)
  for (i64 wt = WF_WIDE_CAP; hm->f_fail && !(hm->f_fail & 1) && !hm->bad_sym && wt >= WIN_TGT_MIN; wt /= 2) {
    g_plan = SMX_PLAN_PRESORTED_WIDE;
    rc = attempt(C, tail, hm, [&] {
      return hm->f_fail == F_LONG ? run_presorted_rewide(C, wt) : run_presorted(C, wt, nullptr, WL_WIDE);
    });
    if (rc) return rc;
    if (hm->f_fail != 2) break;  // held, or groups longer than a wide window (6), or unordered (1)
  }
  if (hm->f_fail && !hm->bad_sym && allow_generic) {
    if (C.ops->b_gap != 0)
      return set_err(SMX_E_ARG, hm->f_fail & 1
                                    ? "branch logs not timestamp-ordered: the generic plan needs b_gap = 0"
                                    : "timestamp groups too long for the presorted windows: the generic plan needs "
                                      "b_gap = 0");
    if (require_ordered && (hm->f_fail & 1)) return unordered();
    if (!(hm->f_fail & 1)) {  // ordered, long groups: the segmented sort, tail behind it
      g_plan = SMX_PLAN_SEGMENTED;
      if ((rc = attempt(C, tail, hm, [&] { return run_generic(C, GEN_SEG); }))) return rc;
      if (!hm->seg_over) return SMX_OK;
      if (require_ordered && (hm->seg_over & SEG_DECREASE)) return unordered();
    }
    // the radix sort: no tail before its duplicate-key verdict; the tail runs once, behind
    // the sort that stands (with oid_lo when (ts, oid_hi) had duplicates)
    g_plan = SMX_PLAN_RADIX;
    if ((rc = attempt(C, false, hm, [&] { return run_generic(C, GEN_RADIX); }))) return rc;
    const bool with_lo = hm->dup_key != 0;
    if (with_lo) g_plan = SMX_PLAN_RADIX_LO;
    return attempt(C, tail, hm, [&] { return with_lo ? run_generic(C, GEN_RADIX_LO) : (int)SMX_OK; });
  }
  return SMX_OK;
}

// T order of the merge (plan + window kernels): the presorted plan first, then the
// fallbacks.  hm: the meta after it.
static int run_order(const Ctx& C, bool allow_generic, bool tail, ComposeMeta* hm) {
  const i64 tgt = knob("SMX_WIN_TGT", WIN_TGT);
  const int rc = attempt(C, tail, hm, [&] { return run_presorted(C, tgt); });
  return rc ? rc : order_fallbacks(C, allow_generic, tail, hm, tgt);
}

__global__ void k_counts(const ComposeMeta* meta, u64 n, i64* counts) {
  counts[0] = (i64)(n - meta->n_skip);
  counts[1] = (i64)meta->n_conf;
}

// Moves whose newAddress or newFile is None see the symbol's inclusive prefix of
// non-None values: moves grouped by symbol (radix sort), then a scan per symbol,
// seeded from the lower shards' values (mvpre) in a sharded merge.
static int run_mvprefix(const Ctx& C, const ComposeMeta& hm, const u64* mvpre) {
  hipStream_t st = C.st;
  const u64 nMv = hm.kcnt[KMOVE];
  if (hm.n_move_none == 0 || nMv == 0) return SMX_OK;
  const i64 n_sym = C.n_sym;
  u64* keys = C.ws<u64>(B_RKEY);
  u32* vals = C.ws<u32>(B_RVAL);
  RadixTemp rt{C.ws<u64>(B_RK2), C.ws<u32>(B_RV2), C.ws<u32>(B_RHIST), C.ws<u32>(B_PART)};
  int shifts[4], ns = 0;
  for (int dgt = 0; dgt < 4; ++dgt)
    if (((u64)(n_sym - 1) >> (8 * dgt)) != 0) shifts[ns++] = 8 * dgt;
  hipLaunchKernelGGL(k_mv_init, dim3(grid_for(nMv)), dim3(BLOCK), 0, st, C.ws<u32>(B_MSYM), nMv, keys, vals);
  if (ns) HIP_TRY(radix_sort_pairs(keys, vals, (i64)nMv, shifts, ns, rt, st));
  hipLaunchKernelGGL(k_mv_fix, dim3(grid_for(nMv)), dim3(BLOCK), 0, st, keys, vals, nMv, C.ws<u32>(B_MSYM), mvpre,
                     (u64)n_sym, C.out->addr, C.out->file);
  HIP_TRY(hipGetLastError());
  return SMX_OK;
}

// smx_compose_async: the presorted plan and its tail, enqueued without a host
// sync (hipGraph-capturable).  counts[0] < -1 afterwards asks for
// smx_compose_finish: -2 the plan failed, -3 moves with a None value need their
// prefix fix-up.
// Plan-failed counts without the tail: what k_emit4's first thread writes on a failed plan.
__global__ void k_counts_failed(const ComposeMeta* meta, i64* counts) {
  counts[0] = meta->bad_sym ? -1 : -2;
  counts[1] = meta->bad_sym ? -1 : (i64)meta->n_conf;
}

// The early-failure flag of this host thread on device dev (pinned, coherent).
static int early_fail_of(int dev, EarlyFail* e) {
  struct Slot {
    int dev = -1;
    EarlyFail e;
  };
  struct Slots {  // the pinned flags and events, freed when the host thread exits
    Slot s[4];
    ~Slots() {
      for (auto& x : s) {
        if (x.dev < 0) continue;
        int cur = 0;
        if (hipGetDevice(&cur) == hipSuccess && cur != x.dev) (void)hipSetDevice(x.dev);
        if (x.e.ev) (void)hipEventDestroy(x.e.ev);
        if (x.e.flag_host) (void)hipHostFree(x.e.flag_host);
        if (cur != x.dev) (void)hipSetDevice(cur);
      }
    }
  };
  static thread_local Slots holder;
  Slot* slots = holder.s;
  for (int i = 0; i < 4; ++i)
    if (Slot& s = slots[i]; s.dev == dev) {
      *e = s.e;
      return SMX_OK;
    }
  for (int i = 0; i < 4; ++i)
    if (Slot& s = slots[i]; s.dev < 0) {
      HIP_TRY(hipHostMalloc((void**)&s.e.flag_host, 64, hipHostMallocCoherent | hipHostMallocMapped));
      HIP_TRY(hipHostGetDevicePointer((void**)&s.e.flag_dev, s.e.flag_host, 0));
      // (no system-scope fence: k_khist / k_fpart store the flag itself at system scope,
      // and a missed flag only costs the tail launched behind a plan that then fails)
      HIP_TRY(hipEventCreateWithFlags(&s.e.ev, hipEventDisableTiming | hipEventDisableSystemFence));
      s.dev = dev;
      *e = s.e;
      return SMX_OK;
    }
  return SMX_E_HIP;  // (more than four devices per host thread: no early flag)
}

// smx_compose's one-workgroup plan: the SMALL_N instance of smx_small.h (the header is
// shared with the batch kernels' unit, so the kernel lives with its one launch)
__global__ void __launch_bounds__(SMALL_NT) k_compose_small(smx_ops ops, smx_compose_out out, ComposeMeta* meta,
                                                                u64* hrec, u64 hseq) {
  compose_small<SMALL_N, true>(ops, out, meta, hrec, hseq);
}

// Largest merge (ops) the one-workgroup path takes (smx_set_small_limit; 0: never).
static std::atomic<int64_t> g_small_max{SMALL_N};
// (symbol ids index the small kernel's hash table with 0xffffffff as its empty mark)
static inline bool small_merge(const smx_ops* ops) {
  return ops->n_a + ops->n_b <= g_small_max.load(std::memory_order_relaxed) && ops->n_sym <= 0xffffffffll;
}

#ifndef SMX_EARLY_MIN
#define SMX_EARLY_MIN (1ll << 22)  // ops from which a synchronous merge waits for k_khist's verdict
#endif

// What the synchronous merge's host learned from k_khist before the windows ran.
struct EarlyVerdict {
  bool failed = false;  // the presorted plan fails for sure (f_fail F_LONG)
  bool bad = false;     // ... and k_khist saw an invalid kind
  // the merge's verdict word in mapped pinned host memory (synchronous calls): the
  // last kernel (k_compose_small, k_emit) stores seq << 1 | bit there, and finish reads
  // it after the stream wait instead of copying the meta block back (one copy packet
  // less per call).  bit: the small plan's invalid input; the large plan's "finish
  // has work left" (an error, a failed plan, None-value moves), which reads the meta.
  u64* hrec = nullptr;       // (device address)
  const u64* hrec_host = nullptr;
  u64 hseq = 0;
  bool rec_used = false;
  bool rec_small = false;
};

struct SmallRec {  // one per host thread, freed when the thread exits
  u64* h = nullptr;
  u64* d = nullptr;  // its device address as the device `dev` sees it
  int dev = -1;
  u64 seq = 0;
  ~SmallRec() {
    if (h) (void)hipHostFree(h);
  }
};
// The thread's verdict word: pinned, mapped, portable host memory.  Its device address is
// taken on the device current at the call and taken again when a later call runs on
// another device (no reliance on one address serving every device).
static SmallRec* small_rec() {
  static thread_local SmallRec r;
  int cur = 0;
  if (hipGetDevice(&cur) != hipSuccess) return nullptr;
  if (!r.h) {
    if (hipHostMalloc((void**)&r.h, 64, hipHostMallocMapped | hipHostMallocPortable | hipHostMallocCoherent) !=
        hipSuccess) {
      r.h = nullptr;
      return nullptr;
    }
    *(volatile u64*)r.h = 0;
  }
  if (r.dev != cur) {
    if (hipHostGetDevicePointer((void**)&r.d, r.h, 0) != hipSuccess) {
      (void)hipGetLastError();
      r.d = nullptr;
      r.dev = -1;
      return nullptr;  // (the caller then reads the meta block instead)
    }
    r.dev = cur;
  }
  return &r;
}

static int enqueue_async(const smx_ops* ops, const smx_compose_out* out, void* ws, const Layout& L,
                         hipStream_t st, bool timed, bool early_ok = false, EarlyVerdict* verdict = nullptr) {
  const i64 n = ops->n_a + ops->n_b;
  StageTimer tm(st, timed);
  Ctx C = make_ctx(ops, out, ws, L, st, &tm, 0, ops->n_a);
  int rc;
  if (small_merge(ops)) {  // the whole merge in one workgroup (smx_small.h)
    tm.begin(ST_SMALL);
    u64* hrec = verdict ? verdict->hrec : nullptr;
    if (hrec) verdict->rec_used = verdict->rec_small = true;
    hipLaunchKernelGGL(k_compose_small, dim3(1), dim3(SMALL_NT), 0, st, *ops, *out, C.ws<ComposeMeta>(B_META), hrec,
                       hrec ? verdict->hseq : (u64)0);
    HIP_TRY(hipGetLastError());
    tm.end(ST_SMALL);
    tm.flush();
    return SMX_OK;
  }
  // A large synchronous merge (not captured): the host waits for k_khist's verdict while
  // k_fpart and the column scans run, then launches the normal or the wide windows and
  // the tail; on an invalid kind no window and no tail (smx_compose_finish reports it).
  EarlyFail early;
  bool use_early = false;
  if (early_ok && n >= SMX_EARLY_MIN) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    int dev = 0;
    HIP_TRY(hipStreamIsCapturing(st, &cs));
    HIP_TRY(hipGetDevice(&dev));
    use_early = cs == hipStreamCaptureStatusNone && early_fail_of(dev, &early) == SMX_OK;
    if (use_early) early.flag_host[0] = early.flag_host[1] = 0u;  // (the previous merge on this thread has synced)
  }
  Deferred dw;
  if ((rc = run_presorted(C, first_tgt(C), use_early ? &early : nullptr, first_level(C), &dw))) return rc;
  if (use_early) {
    HIP_TRY(hipEventSynchronize(early.ev));
    const bool lng = ((volatile u32*)early.flag_host)[0] != 0;
    if (dw.on && !((volatile u32*)early.flag_host)[1]) {
      // k_khist's verdict: the windows that hold the log's timestamp groups.  After
      // F_LONG k_fpart has placed the wide plan's boundaries and the scans its window
      // count (config 5: no doomed normal launch, no re-arm, no second k_fpart)
      if (lng) g_plan = SMX_PLAN_PRESORTED_WIDE;
      if ((rc = launch_presorted_windows(C, lng ? dw.W_w : dw.W, dw.CM, lng ? WL_WIDE : first_level(C)))) return rc;
    } else if (lng || ((volatile u32*)early.flag_host)[1]) {
      const bool bad = ((volatile u32*)early.flag_host)[1] != 0;
      if (verdict) {
        verdict->failed = true;
        verdict->bad = bad;
      }
      if (!verdict || bad) {  // (smx_compose's finish runs the fallback plan next: it writes the counts)
        hipLaunchKernelGGL(k_counts_failed, dim3(1), dim3(1), 0, st, C.ws<ComposeMeta>(B_META), out->counts);
        HIP_TRY(hipGetLastError());
      }
      tm.flush();
      return SMX_OK;
    }
  }
  if (verdict && verdict->hrec) {  // k_emit publishes the verdict: finish skips the meta copy
    C.hrec = verdict->hrec;
    C.hseq = verdict->hseq;
    verdict->rec_used = true;
  }
  if (!knob("SMX_ABLATE", 0) && (rc = launch_tail(C))) return rc;  // SMX_ABLATE (diagnostic builds): window only
  tm.flush();
  return SMX_OK;
}

// The library once replayed a merge's ~25 launches as one cached HIP graph from the second
// merge of a (stream, buffers) key on.  On this ROCm the replay measured slower than
// enqueueing the launches (config 2 0.183 -> 0.160 ms, config 3 2.381 -> 2.352 ms without
// it, profiles/r05_x/graph_ab.txt: the graph's first kernel waits for the whole
// submission), so the cache was removed in round 6; a caller's own capture of
// smx_compose_async stays supported (tests/test_gpu_async.py).  smx_release_graphs is
// kept in the ABI and releases nothing.
extern "C" int smx_release_graphs(void* stream) {
  (void)stream;
  return SMX_OK;
}

// An entry point's frame: an earlier call's error is dropped, a C++ exception becomes SMX_E_HIP.
template <typename Body>
static int entry(const smx_ops* ops, Body&& body) {
  if (!ops) return set_err(SMX_E_ARG, "null ops");
  (void)hipGetLastError();  // an earlier call's error (any library's) is not this call's
  try {
    return body();
  } catch (const std::exception& e) {
    return set_err(SMX_E_HIP, e.what());
  }
}

// early_ok: the synchronous smx_compose (a host wait for k_khist's verdict is allowed)
static int compose_async_impl(const smx_ops* ops, const smx_compose_out* out, void* ws, size_t ws_bytes,
                              hipStream_t st, bool early_ok, EarlyVerdict* verdict = nullptr) {
  Layout L{};
  int rc = check_args(ops, out, ws, ws_bytes, &L);
  if (rc) return rc;
  const i64 n = ops->n_a + ops->n_b;
  const bool small = small_merge(ops);
  g_plan = small ? SMX_PLAN_SMALL : SMX_PLAN_PRESORTED;
  if (n == 0) {
    HIP_TRY(hipMemsetAsync(out->counts, 0, 2 * sizeof(int64_t), st));
    return SMX_OK;
  }
  const bool timed = profiling_on() != 0;
  EarlyVerdict ev;
  if (verdict) ev = *verdict;  // (the caller's verdict word, if any)
  if ((rc = enqueue_async(ops, out, ws, L, st, timed, early_ok, &ev))) return rc;
  if (verdict) *verdict = ev;
  return SMX_OK;
}

// smx_compose_finish: one host sync; runs whatever the asynchronous part left
// (the fallback plans, the None-value move prefix) and the final counts.
// known: the synchronous merge's early verdict (the plan failed): no meta read needed
// before the fallback plan -- k_khist was the last kernel to write the meta's flags
static int compose_finish_impl(const smx_ops* ops, const smx_compose_out* out, void* ws, size_t ws_bytes,
                               hipStream_t st, const EarlyVerdict* known = nullptr) {
  Layout L{};
  int rc = check_args(ops, out, ws, ws_bytes, &L);
  if (rc) return rc;
  const i64 n = ops->n_a + ops->n_b;
  if (n == 0 || knob("SMX_ABLATE", 0)) return SMX_OK;
  StageTimer tm(st, profiling_on() != 0);
  Ctx C = make_ctx(ops, out, ws, L, st, &tm, 0, ops->n_a);
  ComposeMeta hm;
  bool have = false;
  if (known && known->failed) {
    std::memset(&hm, 0, sizeof(hm));
    hm.f_fail = F_LONG;
    hm.bad_sym = known->bad ? 1 : 0;
    have = true;
  } else if (known && known->rec_used) {  // the verdict word: no meta copy when there is no work left
    HIP_TRY(stream_wait(st));
    const u64 v = *(volatile const u64*)known->hrec_host;
    if ((v >> 1) == known->hseq) {
      std::memset(&hm, 0, sizeof(hm));
      hm.bad_sym = v & 1;
      have = known->rec_small || !(v & 1);
    }
  }
  if (!have && (rc = read_meta(C, &hm))) {
    return rc;
  }
  if (hm.bad_sym) return set_err(SMX_E_ARG, "invalid input: sym[i] >= n_sym or kind[i] >= 18");
  if (hm.f_fail && (rc = order_fallbacks(C, true, true, &hm, first_tgt(C)))) return rc;
  if (hm.bad_sym) return set_err(SMX_E_ARG, "invalid input: sym[i] >= n_sym or kind[i] >= 18");
  if (hm.n_move_none && hm.kcnt[KMOVE]) {
    tm.begin(ST_MVPREFIX);
    if ((rc = run_mvprefix(C, hm, nullptr))) return rc;
    hipLaunchKernelGGL(k_counts, dim3(1), dim3(1), 0, st, C.ws<ComposeMeta>(B_META), (u64)n, out->counts);
    HIP_TRY(hipGetLastError());
    tm.end(ST_MVPREFIX);
  }
  tm.flush();
  return SMX_OK;
}

#include "smx_shard.h"

extern "C" int smx_compose_async(const smx_ops* ops, const smx_compose_out* out, void* workspace,
                                 size_t workspace_bytes, void* stream) {
  return entry(ops,
               [&] { return compose_async_impl(ops, out, workspace, workspace_bytes, (hipStream_t)stream, false); });
}

extern "C" int smx_compose_finish(const smx_ops* ops, const smx_compose_out* out, void* workspace,
                                  size_t workspace_bytes, void* stream) {
  return entry(ops, [&] { return compose_finish_impl(ops, out, workspace, workspace_bytes, (hipStream_t)stream); });
}

extern "C" int smx_compose(const smx_ops* ops, const smx_compose_out* out, void* workspace,
                           size_t workspace_bytes, void* stream) {
  return entry(ops, [&] {
    EarlyVerdict ev;
    if (SmallRec* r = small_rec()) {
      ev.hrec = r->d;
      ev.hrec_host = r->h;
      ev.hseq = ++r->seq;
    }
    const int rc = compose_async_impl(ops, out, workspace, workspace_bytes, (hipStream_t)stream, true, &ev);
    return rc ? rc : compose_finish_impl(ops, out, workspace, workspace_bytes, (hipStream_t)stream, &ev);
  });
}

extern "C" int smx_last_plan(void) { return g_plan; }

#ifdef SMALL_STAMPS
// diagnostic builds only: the small kernel's phase stamps of its last call (wall clock, 100 MHz)
extern "C" int smx_diag_small_stamps(uint64_t* host16) {
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpyFromSymbol(host16, HIP_SYMBOL(g_small_stamp), 16 * sizeof(u64)));
  return SMX_OK;
}
#endif

extern "C" int64_t smx_set_small_limit(int64_t n) {
  const int64_t v = n < 0 ? 0 : n > SMALL_N ? SMALL_N : n;
  return g_small_max.exchange(v);
}


extern "C" const char* smx_version(void) { return "smx 0.2 gfx950"; }
