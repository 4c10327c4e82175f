// smx_rga.hip — batched RGA replay on gfx950 (semmerge/crdt.py:23-57), C ABI in include/smx.h.
//
// Exact restatement of the sequential list:
//  * The list is always sorted by (key, creation index): insert places the new
//    element before the first strictly greater key (crdt.py:48-57), so equal
//    keys keep insertion order.
//  * An element's fate depends only on the events of its (list, value):
//    move pops the first live element of that value in list order (= the live
//    one with the smallest (key, index)) and always inserts a new element;
//    delete tombstones every present element of that value (crdt.py:33-43).
//  * materialize = live elements in (key, index) order (crdt.py:45-46).
// Pipeline: stable radix partition of 16-byte event records by list id (up to 65536
// lists: the high byte by a global pass, the low byte per high-byte bucket, which also
// gives the list starts; LDS-staged, coalesced) -> one wave per list (k_rga_wave,
// persistent, in LDS): value groups by hashing, one sequential replay per group,
// survivors ordered by (anchor, t, author, opid, index) -> compaction, each list's
// output offset summed by its own wave from per-chunk survivor sums.
// smx_rga_replay_onto (at the end, smx_rga_onto.h): the same list kernels over jobs, each a
// base's events followed by its own, read in place from bases that are stored once.
// smx_rga_replay_chain (after it, smx_rga_chain.h): jobs that are runs of segments stored once.
#include <algorithm>
#include <chrono>
#include <string>

#include "smx_scan.h"
#include "smx_rga_part.h"
#include "smx_rga_onto.h"
#include "smx_rga_chain.h"
#include "smx_wave_sort.h"
#include "smx_rga_list.h"
#include "smx_rga_out.h"

static int g_rr_grid = 0;  // persistent scatter grid (RR_PER_CU per CU of the device)
static int g_cus = 256;

static bool o_ok(const smx_rga_ops* o) {
  return o->list && o->op && o->value && o->anchor && o->t && o->author && o->opid_hi && o->opid_lo;
}

struct RgaLayout { size_t off[20], total; };
enum { R_REC, R_REC2, R_KEYS, R_KEYS2, R_RHIST, R_TV, R_TS, R_BST, R_GP, R_DEF2, R_PART, R_LSTART, R_SCNT, R_SOFF, R_JOBS, R_CMAP, R_LLEN, R_LPOS, R_N };
// R_PART in u32 words: scan_excl's SCAN_NB partials (8 bytes each), then 16 status words (the
// first 8 zeroed per call): the error word, scan_excl's total, the counts of deferred lists;
// smx_rga_replay_onto and _chain zero all 16: the jobs' total length, 64 bits (k_rga_onto_jobs,
// k_rga_chain_check).
enum { RP_ERR = SCAN_NB * 2, RP_TOTALS = RP_ERR + 2, RP_NDEF = RP_ERR + 4, RP_NDEF_BIG = RP_NDEF + 1,
       RP_ONTO_SUM = RP_ERR + 8, RP_WORDS = RP_ERR + 16 };

// RGA_SRC_ONTO (smx_rga_replay_onto): n = n_out, nl = n_jobs; no partition buffers, the jobs'
// descriptors.  RGA_SRC_CHAIN (smx_rga_replay_chain): the same without the descriptors, plus the
// column map (n_out entries) and the links' lengths and first slots (n_links + 1 each).
static RgaLayout rga_layout(i64 n, i64 nl, int src = RGA_SRC_LISTS, i64 n_links = 0) {
  const i64 nn = n > 0 ? n : 1;
  size_t sz[R_N];
  sz[R_REC] = sz[R_REC2] = (size_t)nn * RGA_REC * 8;
  sz[R_KEYS] = sz[R_KEYS2] = sz[R_TV] = sz[R_TS] = sz[R_GP] = (size_t)nn * 4;
  const i64 nblk = SMX_CEIL_DIV(nn, (i64)RREC_TILE);
  sz[R_RHIST] = (size_t)256 * nblk * 4 + hscan_tsum_bytes(nblk, 256) + 260 * 4;
  sz[R_BST] = (size_t)nn;
  sz[R_PART] = (size_t)RP_WORDS * 4;
  sz[R_LSTART] = sz[R_SOFF] = sz[R_DEF2] = (size_t)(nl + 1) * 4;
  // scnt: RGA_CS_MAX chunk sums, then the counts padded to whole 256-list chunks
  sz[R_SCNT] = (size_t)(RGA_CS_MAX + SMX_CEIL_DIV(nl + 1, (i64)RGA_CS_LISTS) * RGA_CS_LISTS) * 4;
  sz[R_JOBS] = sz[R_CMAP] = sz[R_LLEN] = sz[R_LPOS] = 0;
  if (src != RGA_SRC_LISTS) sz[R_REC2] = sz[R_KEYS] = sz[R_KEYS2] = sz[R_RHIST] = 0;
  if (src == RGA_SRC_ONTO) sz[R_JOBS] = (size_t)(nl + 1) * 16;
  if (src == RGA_SRC_CHAIN) {
    sz[R_CMAP] = (size_t)nn * 4;
    sz[R_LLEN] = sz[R_LPOS] = (size_t)(n_links + 1) * 4;
  }
  RgaLayout L;
  L.total = 0;
  for (int i = 0; i < R_N; ++i) {
    L.off[i] = L.total;
    L.total += (sz[i] + 255) & ~(size_t)255;
  }
  return L;
}

// A workspace carved by rga_layout.
struct RgaWs {
  u64 *rec, *rec2;             // event records: rec list-ordered for the list kernels, rec2 the other pass buffer
  u32 *keys, *keys2;           // the records' list ids, pass by pass
  u32 *rhist, *tsum, *dstart;  // a pass's [tile][digit] histogram, hscan's tile sums, the digits' starts
  u32 *tmp_v, *tmp_s;          // each list's survivors (value; event index | RGA_TOMB_BIT) at its start
  u8* bst;                     // k_rga_big: element states
  u32 *gp, *def2;              // k_rga_big: sorted positions; the lists k_rga_wave2 leaves to it
  u32* part;                   // scan_excl's partials
  i32* err;                    // RGA_E_* bits (the gate the list and output kernels read)
  u32 *totals, *ndef, *ndef_big;  // scan_excl's total; deferred lists (ndef: spare), those for k_rga_big
  u32 *lstart, *csum, *scnt, *soff;  // list starts; 256-list survivor sums, just before the counts; output offsets
  uint4* jobs;                   // smx_rga_replay_onto: the jobs' source descriptors (OntoSrc)
  unsigned long long* onto_sum;  // and their total length (smx_rga_replay_chain's jobs' too)
  u32 *cmap, *llen, *lpos;       // smx_rga_replay_chain: the column map; the links' lengths, their first slots
};

static RgaWs rga_carve(void* ws, const RgaLayout& L, i64 n) {
  const auto at = [&](int slot) { return (u32*)((char*)ws + L.off[slot]); };
  const i64 nblk = SMX_CEIL_DIV(n, (i64)RREC_TILE);
  RgaWs w;
  w.rec = (u64*)at(R_REC), w.rec2 = (u64*)at(R_REC2);
  w.keys = at(R_KEYS), w.keys2 = at(R_KEYS2);
  w.rhist = at(R_RHIST), w.tsum = w.rhist + (size_t)256 * nblk;
  w.dstart = w.tsum + hscan_tsum_bytes(nblk, 256) / 4;
  w.tmp_v = at(R_TV), w.tmp_s = at(R_TS);
  w.bst = (u8*)at(R_BST);
  w.gp = at(R_GP), w.def2 = at(R_DEF2);
  w.part = at(R_PART), w.err = (i32*)(w.part + RP_ERR);
  w.totals = w.part + RP_TOTALS, w.ndef = w.part + RP_NDEF, w.ndef_big = w.part + RP_NDEF_BIG;
  w.lstart = at(R_LSTART), w.csum = at(R_SCNT), w.scnt = w.csum + RGA_CS_MAX, w.soff = at(R_SOFF);
  w.jobs = (uint4*)at(R_JOBS), w.onto_sum = (unsigned long long*)(w.part + RP_ONTO_SUM);
  w.cmap = at(R_CMAP), w.llen = at(R_LLEN), w.lpos = at(R_LPOS);
  return w;
}

extern "C" int smx_rga_workspace_bytes(int64_t n_ops, int64_t n_lists, size_t* bytes) {
  if (!bytes || n_ops < 0 || n_lists < 0) return SMX_E_ARG;
  *bytes = rga_layout(n_ops, n_lists).total;
  return SMX_OK;
}

// Host wait for a stream: a short spin on hipStreamQuery, then the blocking sync.  A call
// ends within a millisecond, and a blocking sync wakes the calling thread ~10-20 us after
// the stream's last packet: 10M events 0.520 -> 0.502 ms, grouped 0.297 -> 0.287 ms
// (profiles/r05_x/spin_ab.txt).  The spin is adaptive per calling thread: twice the
// previous call's wait, between RGA_SPIN_MIN_US and RGA_SPIN_US (a long batch, or many
// caller threads, no longer burn a core for a fixed 20 ms; RGA_SPIN_US 0: block at once).
// (smx_compose.hip's stream_wait blocks at once, on its own measurement: not the same wait.)
#ifndef RGA_SPIN_US
#define RGA_SPIN_US 2000
#endif
#ifndef RGA_SPIN_MIN_US
#define RGA_SPIN_MIN_US 200
#endif
static hipError_t rga_stream_wait(hipStream_t st) {
  static thread_local long long last_us = RGA_SPIN_US / 2;  // this thread's previous wait
  if (RGA_SPIN_US <= 0) return hipStreamSynchronize(st);
  const long long budget = std::min<long long>(RGA_SPIN_US, std::max<long long>(RGA_SPIN_MIN_US, 2 * last_us));
  const auto t0 = std::chrono::steady_clock::now();
  const auto us = [&]() -> long long {
    return std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
  };
  hipError_t e = hipStreamQuery(st);
  while (e == hipErrorNotReady && us() <= budget) e = hipStreamQuery(st);
  if (e == hipErrorNotReady) e = hipStreamSynchronize(st);
  last_us = us();
  return e;
}

// One partition pass on the list id's byte at `shift`: the tiles' digit histograms, their
// column scan (each tile's output offsets; dstart = the digits' starts), the stable scatter.
// FIRST: the pass that reads the input columns and packs the records (no kin / rin); a later
// pass moves the one before's.  KO: the keys it writes (u8: the low byte, for k_rrec_local).
template <bool FIRST, typename KO>
static void rga_pass(const smx_rga_ops& o, const RgaWs& w, const u32* kin, const u64* rin, KO* kout, u64* rout,
                     int shift, hipStream_t st) {
  const int nblk = (int)SMX_CEIL_DIV(o.n_ops, (i64)RREC_TILE);
  const int sgrid = nblk < g_rr_grid ? nblk : g_rr_grid;  // persistent scatter workgroups
  hipLaunchKernelGGL(k_rrec_hist<FIRST>, dim3(nblk), dim3(BLOCK), 0, st, o, kin, shift, w.rhist, w.err);
  // (one-launch column scan with the bucket starts from its last workgroup, on a
  // [digit][tile] histogram: 18.7 + 34.3 us against hscan's 22 + 28.8, profiles/r04_ac)
  hscan(w.rhist, nblk, 256u, w.tsum, w.dstart, st);
  hipLaunchKernelGGL((k_rrec_scatter<FIRST, KO>), dim3(sgrid), dim3(RR_NT), 0, st, o, kin, rin, kout, rout, shift,
                     w.rhist, w.err, (u32)nblk);
}

// The device's CU count, once: the persistent grids are sized by it.
static int rga_device_init() {
  if (g_rr_grid == 0) {  // persistent scatter workgroups
    int dev = 0, cus = 0;
    HIP_TRY(hipGetDevice(&dev));
    HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    g_cus = cus > 0 ? cus : 256;
    g_rr_grid = g_cus * RR_PER_CU;
  }
  return SMX_OK;
}

// k_rga_wave's persistent grid for nl lists
static u32 rga_wave_grid(i64 nl) {
  i64 wg = SMX_CEIL_DIV(nl, (i64)RW_WAVES);
  if (RW_PER_CU > 0 && wg > (i64)g_cus * RW_PER_CU) wg = (i64)g_cus * RW_PER_CU;
  return (u32)wg;
}

// The output stage: the lists' survivors from their slices (tmp_v / tmp_s at lstart) to the output.
static int rga_out_stage(const RgaWs& w, i64 nl, const smx_rga_out* out, hipStream_t st) {
  if (nl <= RGA_FUSED_MAX) {  // each list's wave finds its own offset
    hipLaunchKernelGGL(k_rga_out_fused, dim3(SMX_CEIL_DIV(nl, (i64)(BLOCK / WAVE * RGA_OUT_LPW))), dim3(BLOCK), 0, st,
                       w.tmp_v, w.tmp_s, w.lstart, w.scnt, nl, *out, w.err);
  } else {
    HIP_TRY((scan_excl<OpSum, u32, u32>(w.scnt, w.soff, nl, nullptr, w.part, w.totals, st)));
    hipLaunchKernelGGL(k_rga_out, dim3(SMX_CEIL_DIV(nl, (i64)(BLOCK / WAVE))), dim3(BLOCK), 0, st, w.tmp_v, w.tmp_s,
                       w.lstart, w.scnt, w.soff, nl, *out, w.err);
    hipLaunchKernelGGL(k_rga_fin, dim3(1), dim3(1), 0, st, w.totals, nl, *out, w.err);
  }
  HIP_TRY(hipGetLastError());
  return SMX_OK;
}

static int rga_impl(const smx_rga_ops* ops, const smx_rga_out* out, void* ws, size_t wsb, hipStream_t st,
                    bool grouped) {
  const i64 n = ops->n_ops, nl = ops->n_lists;
  if (n < 0 || nl < 0 || n > (i64)RGA_IDX_MASK || nl >= (i64)0x7fffffff)
    return smx_set_error(SMX_E_ARG, "bad sizes");
  if (!out || !out->out_offsets || !out->counts) return smx_set_error(SMX_E_ARG, "null output");
  if (n == 0) {
    HIP_TRY(hipMemsetAsync(out->out_offsets, 0, (size_t)(nl + 1) * 8, st));
    HIP_TRY(hipMemsetAsync(out->counts, 0, 8, st));
    return SMX_OK;
  }
  if (nl < 1) return smx_set_error(SMX_E_ARG, "n_lists must be >= 1");
  if (!o_ok(ops)) return smx_set_error(SMX_E_ARG, "null input pointer");
  const RgaLayout L = rga_layout(n, nl);
  if (!ws || wsb < L.total)
    return smx_set_error(SMX_E_WORKSPACE, ("workspace too small: need " + std::to_string(L.total)).c_str());
  const RgaWs w = rga_carve(ws, L, n);
  const smx_rga_ops o = *ops;
  const int grid = (int)(SMX_CEIL_DIV(n, (i64)BLOCK) < 8192 ? SMX_CEIL_DIV(n, (i64)BLOCK) : 8192);
  HIP_TRY(hipMemsetAsync(w.err, 0, 32, st));
  if (int rc = rga_device_init()) return rc;
  int npass = 1;  // partition passes, 8 bits of the list id each
  while (npass < 4 && ((u64)(nl - 1) >> (8 * npass)) != 0) ++npass;
  if (grouped) {  // the caller's events come list by list: no partition, the list kernels read the columns in place
    hipLaunchKernelGGL(k_rga_gbounds, dim3((int)SMX_CEIL_DIV((i64)grid, (i64)4)), dim3(BLOCK), 0, st, o, w.lstart,
                       w.csum, w.err);
  } else if (npass == 2) {  // high byte by the global pass, low byte (and the list starts) per bucket
    rga_pass<true, u8>(o, w, nullptr, nullptr, (u8*)w.keys2, w.rec2, 8, st);
    hipLaunchKernelGGL(k_rrec_local, dim3(RGA_NDIG * RL_S), dim3(RL_NT), 0, st, (const u8*)w.keys2, w.rec2, w.rec,
                       w.dstart, nl, w.lstart, w.csum);
  } else {  // LSD passes, ping-pong so that the last one lands in rec; the list starts from the sorted ids
    u64* rbuf[2] = {npass % 2 ? w.rec : w.rec2, npass % 2 ? w.rec2 : w.rec};
    u32* kbuf[2] = {w.keys, w.keys2};
    rga_pass<true, u32>(o, w, nullptr, nullptr, kbuf[0], rbuf[0], 0, st);
    for (int p = 1; p < npass; ++p)
      rga_pass<false, u32>(o, w, kbuf[(p - 1) & 1], rbuf[(p - 1) & 1], kbuf[p & 1], rbuf[p & 1], 8 * p, st);
    hipLaunchKernelGGL(k_rga_bounds, dim3(grid), dim3(BLOCK), 0, st, kbuf[(npass - 1) & 1], n, nl, w.lstart, w.csum);
  }

  const int tomb = out->out_tomb != nullptr;
  hipLaunchKernelGGL(grouped ? k_rga_wave<true> : k_rga_wave<false>, dim3(rga_wave_grid(nl)), dim3(WAVE * RW_WAVES), 0, st, o,
                     w.rec, w.lstart, n, nl, w.tmp_v, w.tmp_s, w.scnt, tomb, w.err);
  // lists of more than RW_CAP events (a few, if any).  (On a second stream beside
  // k_rga_wave they measured no faster: their workgroups trail k_rga_wave's, and the
  // join costs ~14 us, round 4.)
  hipLaunchKernelGGL(k_rga_wave2<RGA_SRC_LISTS>, dim3(64), dim3(WAVE * RW_WAVES), 0, st, o, w.rec, w.lstart, n, nl, w.def2,
                     w.ndef_big, w.tmp_v, w.tmp_s, w.scnt, tomb, w.err, (int)grouped);
  hipLaunchKernelGGL(k_rga_big<RGA_SRC_LISTS>, dim3(RGA_BIG_GRID), dim3(1024), 0, st, o, w.rec, w.lstart, n, nl, w.def2, w.ndef_big,
                     w.bst, w.gp, w.tmp_v, w.tmp_s, w.scnt, tomb, w.err);

  if (int rc = rga_out_stage(w, nl, out, st)) return rc;
  i32 herr = 0;
  HIP_TRY(hipMemcpyAsync(&herr, w.err, 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(rga_stream_wait(st));
  if (herr & RGA_E_INPUT) return smx_set_error(SMX_E_ARG, "invalid input: list >= n_lists or op > 2");
  if (herr & RGA_E_UNGROUPED) return rga_impl(ops, out, ws, wsb, st, false);  // (not grouped after all)
  return SMX_OK;
}

extern "C" int smx_rga_replay_ex(const smx_rga_ops* ops, const smx_rga_out* out, void* ws, size_t wsb,
                                 uint32_t flags, void* stream) {
  if (!ops) return SMX_E_ARG;
  if (flags & ~(uint32_t)SMX_RGA_GROUPED) return smx_set_error(SMX_E_ARG, "unknown smx_rga_replay_ex flag");
  (void)hipGetLastError();  // an earlier call's error (any library's) is not this call's
  return rga_impl(ops, out, ws, wsb, (hipStream_t)stream, (flags & SMX_RGA_GROUPED) != 0);
}

extern "C" int smx_rga_replay(const smx_rga_ops* ops, const smx_rga_out* out, void* ws, size_t wsb,
                              void* stream) {
  return smx_rga_replay_ex(ops, out, ws, wsb, 0u, stream);
}

// ---------------------------------------------------------------------------
// smx_rga_replay_onto: many jobs, each a base's events followed by its own, over bases
// stored once (smx_rga_onto.h).  The pre-pass gives each job its length and slice; the
// list kernels' RGA_SRC_ONTO instantiations read a job's events from the two column ranges; the
// output stage is the replay's own, one "list" per job.
static RgaLayout rga_onto_layout(i64 n_jobs, i64 n_out) { return rga_layout(n_out, n_jobs, RGA_SRC_ONTO); }

extern "C" int smx_rga_replay_onto_workspace_bytes(int64_t n_jobs, int64_t n_out, size_t* bytes) {
  if (!bytes || n_jobs < 0 || n_out < 0 || n_jobs >= (i64)0x7fffffff || n_out > (i64)RGA_IDX_MASK)
    return smx_set_error(SMX_E_ARG, "bad sizes");
  *bytes = rga_onto_layout(n_jobs, n_out).total;
  return SMX_OK;
}

extern "C" int smx_rga_replay_onto(const smx_rga_onto* onto, const smx_rga_out* out, void* ws, size_t wsb,
                                   void* stream) {
  if (!onto) return smx_set_error(SMX_E_ARG, "null smx_rga_onto");
  const smx_rga_onto& q = *onto;
  const i64 nj = q.n_jobs;
  if (q.n_total < 0 || q.n_bases < 0 || nj < 0 || q.n_out < 0) return smx_set_error(SMX_E_ARG, "negative size");
  if (q.n_total > (i64)RGA_IDX_MASK) return smx_set_error(SMX_E_ARG, "n_total too large");
  if (q.n_out > (i64)RGA_IDX_MASK) return smx_set_error(SMX_E_ARG, "n_out too large");
  if (q.n_bases >= (i64)0x7fffffff || nj >= (i64)0x7fffffff) return smx_set_error(SMX_E_ARG, "too many bases or jobs");
  if (!out || !out->out_offsets || !out->counts) return smx_set_error(SMX_E_ARG, "null output");
  if (q.n_out > 0 && (!out->out_value || !out->out_src)) return smx_set_error(SMX_E_ARG, "null output");
  if (!q.base_off || !q.own_off || (nj > 0 && !q.job_base)) return smx_set_error(SMX_E_ARG, "null offsets or job_base");
  if (q.n_total > 0 && !(q.op && q.value && q.anchor && q.t && q.author && q.opid_hi && q.opid_lo))
    return smx_set_error(SMX_E_ARG, "null input pointer");
  hipStream_t st = (hipStream_t)stream;
  const RgaLayout L = rga_onto_layout(nj, q.n_out);
  if (nj > 0) {
    if (!ws || wsb < L.total)
      return smx_set_error(SMX_E_WORKSPACE, ("workspace too small: need " + std::to_string(L.total)).c_str());
    if (reinterpret_cast<uintptr_t>(ws) & 15) return smx_set_error(SMX_E_WORKSPACE, "workspace not 16-byte aligned");
  }
  (void)hipGetLastError();  // an earlier call's error (any library's) is not this call's
  if (nj == 0) {
    HIP_TRY(hipMemsetAsync(out->out_offsets, 0, 8, st));
    HIP_TRY(hipMemsetAsync(out->counts, 0, 8, st));
    return SMX_OK;
  }
  const RgaWs w = rga_carve(ws, L, q.n_out > 0 ? q.n_out : 1);
  // the columns as the list kernels take them; in place of the list ids, the jobs' descriptors
  const smx_rga_ops o = {q.n_total, nj, (const u32*)w.jobs, q.op, q.value, q.anchor, q.t, q.author, q.opid_hi, q.opid_lo};
  const RgaOntoJobs jq = {q.n_total, q.n_bases, nj, q.n_out, q.base_off, q.own_off, q.job_base};
  HIP_TRY(hipMemsetAsync(w.err, 0, 64, st));
  if (int rc = rga_device_init()) return rc;
  const i64 top = (q.n_bases > nj ? q.n_bases : nj) + 1;
  const int grid = (int)(SMX_CEIL_DIV(top, (i64)BLOCK) < 2048 ? SMX_CEIL_DIV(top, (i64)BLOCK) : 2048);
  u32* len = w.soff;  // (the output stage's scan writes soff later)
  hipLaunchKernelGGL(k_rga_onto_jobs, dim3(grid), dim3(BLOCK), 0, st, jq, len, w.jobs, w.csum, w.onto_sum, w.err);
  HIP_TRY((scan_excl<OpSum, u32, u32>(len, w.lstart, nj + 1, nullptr, w.part, w.totals, st)));
  hipLaunchKernelGGL(k_rga_onto_fit, dim3(1), dim3(1), 0, st, w.onto_sum, q.n_out, w.err);

  const int tomb = out->out_tomb != nullptr;
  const i64 n = q.n_total;
  hipLaunchKernelGGL((k_rga_wave<true, RGA_SRC_ONTO>), dim3(rga_wave_grid(nj)), dim3(WAVE * RW_WAVES), 0, st, o, w.rec, w.lstart,
                     n, nj, w.tmp_v, w.tmp_s, w.scnt, tomb, w.err);
  hipLaunchKernelGGL(k_rga_wave2<RGA_SRC_ONTO>, dim3(64), dim3(WAVE * RW_WAVES), 0, st, o, w.rec, w.lstart, n, nj, w.def2,
                     w.ndef_big, w.tmp_v, w.tmp_s, w.scnt, tomb, w.err, 1);
  hipLaunchKernelGGL(k_rga_big<RGA_SRC_ONTO>, dim3(RGA_BIG_GRID), dim3(1024), 0, st, o, w.rec, w.lstart, n, nj, w.def2,
                     w.ndef_big, w.bst, w.gp, w.tmp_v, w.tmp_s, w.scnt, tomb, w.err);
  if (int rc = rga_out_stage(w, nj, out, st)) return rc;
  i32 herr = 0;
  HIP_TRY(hipMemcpyAsync(&herr, w.err, 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(rga_stream_wait(st));
  if (herr & RGA_E_INPUT)
    return smx_set_error(SMX_E_ARG, "invalid input: an op > 2, a bad offset or job_base, or more events than n_out");
  return SMX_OK;
}

// ---------------------------------------------------------------------------
// smx_rga_replay_chain: many jobs, each a run of segments stored once (smx_rga_chain.h).  The
// pre-pass checks the tables and gives each job its slice and its part of the column map; the
// list kernels' RGA_SRC_CHAIN instantiations read a job's events through the map; the output
// stage is the replay's own, one "list" per job.
static RgaLayout rga_chain_layout(i64 n_jobs, i64 n_links, i64 n_out) {
  return rga_layout(n_out, n_jobs, RGA_SRC_CHAIN, n_links);
}

extern "C" int smx_rga_replay_chain_workspace_bytes(int64_t n_jobs, int64_t n_links, int64_t n_out, size_t* bytes) {
  if (!bytes || n_jobs < 0 || n_links < 0 || n_out < 0 || n_jobs >= (i64)0x7fffffff || n_links >= (i64)0x7fffffff ||
      n_out > (i64)RGA_IDX_MASK)
    return smx_set_error(SMX_E_ARG, "bad sizes");
  *bytes = rga_chain_layout(n_jobs, n_links, n_out).total;
  return SMX_OK;
}

extern "C" int smx_rga_replay_chain(const smx_rga_chain* chain, const smx_rga_out* out, void* ws, size_t wsb,
                                    void* stream) {
  if (!chain) return smx_set_error(SMX_E_ARG, "null smx_rga_chain");
  const smx_rga_chain& q = *chain;
  const i64 nj = q.n_jobs;
  if (q.n_total < 0 || q.n_segs < 0 || nj < 0 || q.n_links < 0 || q.n_out < 0)
    return smx_set_error(SMX_E_ARG, "negative size");
  if (q.n_total > (i64)RGA_IDX_MASK) return smx_set_error(SMX_E_ARG, "n_total too large");
  if (q.n_out > (i64)RGA_IDX_MASK) return smx_set_error(SMX_E_ARG, "n_out too large");
  if (q.n_segs >= (i64)0x7fffffff || nj >= (i64)0x7fffffff || q.n_links >= (i64)0x7fffffff)
    return smx_set_error(SMX_E_ARG, "too many segments, jobs or links");
  if (!out || !out->out_offsets || !out->counts) return smx_set_error(SMX_E_ARG, "null output");
  if (q.n_out > 0 && (!out->out_value || !out->out_src)) return smx_set_error(SMX_E_ARG, "null output");
  if (!q.seg_off || !q.job_off || (q.n_links > 0 && !q.job_seg))
    return smx_set_error(SMX_E_ARG, "null offsets or job_seg");
  if (q.n_total > 0 && !(q.op && q.value && q.anchor && q.t && q.author && q.opid_hi && q.opid_lo))
    return smx_set_error(SMX_E_ARG, "null input pointer");
  hipStream_t st = (hipStream_t)stream;
  const RgaLayout L = rga_chain_layout(nj, q.n_links, q.n_out);
  if (nj > 0) {
    if (!ws || wsb < L.total)
      return smx_set_error(SMX_E_WORKSPACE, ("workspace too small: need " + std::to_string(L.total)).c_str());
    if (reinterpret_cast<uintptr_t>(ws) & 15) return smx_set_error(SMX_E_WORKSPACE, "workspace not 16-byte aligned");
  }
  (void)hipGetLastError();  // an earlier call's error (any library's) is not this call's
  if (nj == 0) {
    HIP_TRY(hipMemsetAsync(out->out_offsets, 0, 8, st));
    HIP_TRY(hipMemsetAsync(out->counts, 0, 8, st));
    return SMX_OK;
  }
  const RgaWs w = rga_carve(ws, L, q.n_out > 0 ? q.n_out : 1);
  // the columns as the list kernels take them; in place of the list ids, the column map
  const smx_rga_ops o = {q.n_total, nj, w.cmap, q.op, q.value, q.anchor, q.t, q.author, q.opid_hi, q.opid_lo};
  const RgaChainJobs jq = {q.n_total, q.n_segs, nj, q.n_links, q.n_out, q.seg_off, q.job_off, q.job_seg};
  HIP_TRY(hipMemsetAsync(w.err, 0, 64, st));
  if (int rc = rga_device_init()) return rc;
  // a wave per job, then per link; a thread per entry of the offset tables
  const i64 waves = std::max(nj, q.n_links), top = std::max(waves, q.n_segs) + 1;
  const i64 want = std::max(SMX_CEIL_DIV(waves, (i64)(BLOCK / WAVE)), SMX_CEIL_DIV(top, (i64)BLOCK));
  const int grid = (int)std::min<i64>(want, 2048);
  hipLaunchKernelGGL(k_rga_chain_check, dim3(grid), dim3(BLOCK), 0, st, jq, w.llen, w.csum, w.onto_sum, w.err);
  HIP_TRY((scan_excl<OpSum, u32, u32>(w.llen, w.lpos, q.n_links + 1, nullptr, w.part, w.totals, st)));
  hipLaunchKernelGGL(k_rga_onto_fit, dim3(1), dim3(1), 0, st, w.onto_sum, q.n_out, w.err);
  hipLaunchKernelGGL(k_rga_chain_map, dim3(grid), dim3(BLOCK), 0, st, jq, w.lpos, w.lstart, w.cmap, w.err);

  const int tomb = out->out_tomb != nullptr;
  const i64 n = q.n_total;
  hipLaunchKernelGGL((k_rga_wave<true, RGA_SRC_CHAIN>), dim3(rga_wave_grid(nj)), dim3(WAVE * RW_WAVES), 0, st, o, w.rec,
                     w.lstart, n, nj, w.tmp_v, w.tmp_s, w.scnt, tomb, w.err);
  hipLaunchKernelGGL(k_rga_wave2<RGA_SRC_CHAIN>, dim3(64), dim3(WAVE * RW_WAVES), 0, st, o, w.rec, w.lstart, n, nj,
                     w.def2, w.ndef_big, w.tmp_v, w.tmp_s, w.scnt, tomb, w.err, 1);
  hipLaunchKernelGGL(k_rga_big<RGA_SRC_CHAIN>, dim3(RGA_BIG_GRID), dim3(1024), 0, st, o, w.rec, w.lstart, n, nj, w.def2,
                     w.ndef_big, w.bst, w.gp, w.tmp_v, w.tmp_s, w.scnt, tomb, w.err);
  if (int rc = rga_out_stage(w, nj, out, st)) return rc;
  i32 herr = 0;
  HIP_TRY(hipMemcpyAsync(&herr, w.err, 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(rga_stream_wait(st));
  if (herr & RGA_E_INPUT)
    return smx_set_error(SMX_E_ARG, "invalid input: an op > 2, a bad offset or job_seg, segments that do not ascend "
                                    "within a job, or more events than n_out");
  return SMX_OK;
}
