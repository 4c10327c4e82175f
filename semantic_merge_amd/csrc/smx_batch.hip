// smx_batch.hip — the batched entry points of include/smx.h: smx_compose_batch and
// smx_compose_batch_shared with their _ex forms and smx_compose_pairs (kernels in smx_batch.h
// and smx_batch_large.h) and smx_screen /
// smx_screen_ex (kernels in smx_screen.h), and smx_screen_candidates (kernels in smx_cand.h,
// DESIGN.md §14), which has a shape of its own: a sort and a bit matrix, no size classes; and
// smx_compose_train (kernels in smx_train.h), the class launch over trains, with
// smx_train_stage / smx_train_land beside it (kernels in smx_train_step.h, DESIGN.md §23: one
// step of a train of any size, a launch each and no workspace), and
// smx_screen_train (kernels in smx_screen_train.h), the screen's over trains, and
// smx_compose_tree (kernels in smx_tree.h), the class launch once per level of a
// tree of logs, and smx_screen_tree (kernels in smx_screen_tree.h), the screen's
// over such a tree.
//
// All but smx_screen_candidates have one shape: a pre-pass sorts the items (merges, pairs,
// trains, a level's nodes) into three size classes, then one kernel per class runs its list on a
// grid capped by what the device holds at once.  That shape is here once: the residency cache
// (resident_of) and the per-class launch (launch_classes).  The three compose batches go
// further: they have one size function, one argument check and one runner (batch_ws_size,
// batch_check_args, batch_run) over a description of each form (batch_form, batch_prepass).  The
// four entry points over trains and trees share their column, result-array and workspace checks,
// the screen's extraction over every log and the per-level launch (train_columns_set,
// train_compose_arrays, train_ws_check, screen_extract_logs, launch_levels); their size and
// null-pointer checks differ per form in set, order and message, and stay in each entry point.
// Nothing here waits, allocates or reads back.
#include <exception>

// (the small kernel's phase stamps belong to the single merge: smx_compose.hip defines the
// array and reads it, and the batch kernels compiled here keep none)
#undef SMALL_STAMPS
#include "smx_batch_large.h"
#include "smx_screen.h"
#include "smx_cand.h"
#include "smx_train.h"
#include "smx_train_step.h"
#include "smx_screen_train.h"
#include "smx_tree.h"
#include "smx_screen_tree.h"

// The kernels with a residency-capped grid, and the threads of a workgroup of each.
enum {
  R_BATCH = 0,
  R_SHARED = 3,
  R_EXTRACT = 6,
  R_SCREEN = 7,
  R_EXTRACT_LARGE = 10,
  R_STREAM = 11,
  R_LARGE = 12,
  R_LARGE_SHARED = 13,
  R_PAIRS = 14,
  R_LARGE_PAIRS = 17,
  R_TRAIN = 18,
  R_SCREEN_TRAIN = 21,
  R_TREE = 24,
  R_SCREEN_TREE = 27,
  R_N = 30
};
template <typename B>
using BatchKernel = void (*)(B, const u32*, const u32*);
template <typename B>
static constexpr BatchKernel<B> kBatchKernels[BATCH_CLASSES] = {
    k_compose_batch<batch_class_cap(0), B>, k_compose_batch<batch_class_cap(1), B>,
    k_compose_batch<batch_class_cap(2), B>};
typedef void (*ScreenKernel)(ScreenArgs, ScreenWs, const u32*, const u32*);
static constexpr ScreenKernel kScreenKernels[SCREEN_CLASSES] = {
    k_screen_pairs<screen_class_cap(0)>, k_screen_pairs<screen_class_cap(1)>, k_screen_pairs<screen_class_cap(2)>};
typedef void (*TrainKernel)(smx_train, TrainWs, const u32*, const u32*);
static constexpr TrainKernel kTrainKernels[BATCH_CLASSES] = {
    k_compose_train<batch_class_cap(0)>, k_compose_train<batch_class_cap(1)>, k_compose_train<batch_class_cap(2)>};
typedef void (*ScreenTrainKernel)(ScreenTrainArgs, ScreenWs, const u32*, const u32*);
static constexpr ScreenTrainKernel kScreenTrainKernels[SCREEN_CLASSES] = {
    k_screen_train<screen_class_cap(0)>, k_screen_train<screen_class_cap(1)>, k_screen_train<screen_class_cap(2)>};
typedef void (*TreeKernel)(smx_tree, TreeWs, i32, const u32*, const u32*);
static constexpr TreeKernel kTreeKernels[BATCH_CLASSES] = {
    k_compose_tree<batch_class_cap(0)>, k_compose_tree<batch_class_cap(1)>, k_compose_tree<batch_class_cap(2)>};
typedef void (*ScreenTreeKernel)(ScreenTreeArgs, ScreenWs, ScreenTreeWs, i32, const u32*, const u32*);
static constexpr ScreenTreeKernel kScreenTreeKernels[SCREEN_CLASSES] = {
    k_screen_tree<screen_class_cap(0)>, k_screen_tree<screen_class_cap(1)>, k_screen_tree<screen_class_cap(2)>};
static constexpr int kBatchCaps[BATCH_CLASSES] = {batch_class_cap(0), batch_class_cap(1), batch_class_cap(2)};
static constexpr int kScreenCaps[SCREEN_CLASSES] = {screen_class_cap(0), screen_class_cap(1), screen_class_cap(2)};

// Workgroups of each of those kernels that one device holds at once (the grid cap of its
// launch): the runtime's occupancy figure for the kernel times the CU count, asked once
// per device and host thread.
static int resident_of(const int** out) {
  struct Entry {
    int dev = -1;
    int wg[R_N] = {};
  };
  static thread_local Entry g[4];
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  Entry* e = &g[dev & 3];
  if (e->dev != dev) {
    const void* fn[R_N];
    int threads[R_N];
    for (int c = 0; c < BATCH_CLASSES; ++c) {
      fn[R_BATCH + c] = (const void*)kBatchKernels<smx_batch>[c];
      fn[R_SHARED + c] = (const void*)kBatchKernels<smx_batch_shared>[c];
      fn[R_PAIRS + c] = (const void*)kBatchKernels<smx_pairs>[c];
      fn[R_TRAIN + c] = (const void*)kTrainKernels[c];
      fn[R_TREE + c] = (const void*)kTreeKernels[c];
      threads[R_BATCH + c] = threads[R_SHARED + c] = threads[R_PAIRS + c] = threads[R_TRAIN + c] =
          threads[R_TREE + c] = kBatchCaps[c] / 2;
    }
    fn[R_EXTRACT] = (const void*)k_screen_extract;
    threads[R_EXTRACT] = SCREEN_T1;
    for (int c = 0; c < SCREEN_CLASSES; ++c) {
      fn[R_SCREEN + c] = (const void*)kScreenKernels[c];
      fn[R_SCREEN_TRAIN + c] = (const void*)kScreenTrainKernels[c];
      fn[R_SCREEN_TREE + c] = (const void*)kScreenTreeKernels[c];
      threads[R_SCREEN + c] = threads[R_SCREEN_TRAIN + c] = threads[R_SCREEN_TREE + c] = kScreenCaps[c] / 2;
    }
    fn[R_EXTRACT_LARGE] = (const void*)k_screen_extract_large;
    threads[R_EXTRACT_LARGE] = SCREEN_TL;
    fn[R_STREAM] = (const void*)k_screen_stream;
    threads[R_STREAM] = SCREEN_N / 2;
    fn[R_LARGE] = (const void*)k_compose_batch_large<smx_batch>;
    fn[R_LARGE_SHARED] = (const void*)k_compose_batch_large<smx_batch_shared>;
    fn[R_LARGE_PAIRS] = (const void*)k_compose_batch_large<smx_pairs>;
    threads[R_LARGE] = threads[R_LARGE_SHARED] = threads[R_LARGE_PAIRS] = LARGE_NT;
    int cus = 0;
    HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    for (int k = 0; k < R_N; ++k) {
      int per = 0;
      HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, fn[k], threads[k], 0));
      e->wg[k] = (per > 0 ? per : 1) * (cus > 0 ? cus : 1);
    }
    e->dev = dev;
  }
  *out = e->wg;
  return SMX_OK;
}

// min(resident, items) workgroups, at most grid_cap when that is positive.
static dim3 capped_grid(int resident, i64 items, i64 grid_cap) {
  i64 g = resident < items ? (i64)resident : items;
  if (grid_cap > 0 && g > grid_cap) g = grid_cap;
  return dim3((unsigned)g);
}

// One kernel per size class: class c's kernel on cap[c] / 2 threads, with its count
// cnt + c and its list lists + c * stride after the kernel's own arguments.
template <typename K, typename... A>
static int launch_classes(K* const (&kern)[3], const int (&cap)[3], const int* resident, i64 items, i64 grid_cap,
                          hipStream_t st, const u32* cnt, const u32* lists, size_t stride, const A&... args) {
  for (int c = 0; c < 3; ++c) {
    hipLaunchKernelGGL(kern[c], capped_grid(resident[c], items, grid_cap), dim3(cap[c] / 2), 0, st, args..., cnt + c,
                       lists + c * stride);
    HIP_TRY(hipGetLastError());
  }
  return SMX_OK;
}

// The three compose batches' workspace: the class counts, `info` bytes of the form's own, the
// three class lists (base); with SMX_BATCH_LARGE the fourth list and the slices, n_ops result
// entries long, behind them (total).
struct BatchWsSize { size_t base, total; };
static BatchWsSize batch_ws_size(size_t info, int64_t n_items, int64_t n_ops, bool large) {
  const size_t base = BATCH_HDR + info + BATCH_CLASSES * batch_list_bytes(n_items);
  return {base, base + (large ? batch_large_bytes(n_items, n_ops) : 0)};
}

// What the host has to know of a form beside batch_check and batch_merge (smx_batch.h); the
// sizes every form has (its items, n_total, n_sym, grid_cap) are checked in batch_check_args.
struct BatchForm {
  const char* plain_query;          // the size query of its unflagged call, for messages
  int first, first_large;           // its rows of resident_of: the three class kernels', the large kernel's
  bool aligned = false;             // the workspace is 8-byte aligned whatever the flags
  const char* own_error = nullptr;  // what the checks only this struct has object to
  int64_t items, n_ops;             // its merges or pairs; its result entries
  bool empty;                       // nothing to do, whatever else the struct holds
  size_t info = 0;                  // workspace bytes between BATCH_HDR and the class lists
  const char* index_names;          // its own index arrays, and whether all of them are set
  bool index_ok;
};
static BatchForm batch_form(const smx_batch& b) {
  BatchForm f;
  f.plain_query = "smx_compose_batch_workspace_bytes", f.first = R_BATCH, f.first_large = R_LARGE;
  f.items = b.n_merges, f.n_ops = b.n_total, f.empty = b.n_merges == 0;
  f.index_names = "off / n_a", f.index_ok = b.off && b.n_a;
  return f;
}
static BatchForm batch_form(const smx_batch_shared& b) {
  BatchForm f;
  f.plain_query = "smx_compose_batch_shared_workspace_bytes", f.first = R_SHARED, f.first_large = R_LARGE_SHARED;
  f.own_error = b.n_shared < 0 ? "negative size" : b.n_shared > b.n_total ? "n_shared over n_total" : nullptr;
  if (!f.own_error && b.shared_is_b != 0 && b.shared_is_b != 1) f.own_error = "shared_is_b is neither 0 nor 1";
  // (past the checks each factor is <= 2^31: no overflow; before them the value is not used)
  f.n_ops = (int64_t)((uint64_t)b.n_total - (uint64_t)b.n_shared + (uint64_t)b.n_merges * (uint64_t)b.n_shared);
  f.items = b.n_merges, f.empty = b.n_merges == 0, f.index_names = "off", f.index_ok = b.off != nullptr;
  return f;
}
static BatchForm batch_form(const smx_pairs& b) {
  BatchForm f;
  f.plain_query = "smx_compose_pairs_workspace_bytes", f.first = R_PAIRS, f.first_large = R_LARGE_PAIRS;
  f.aligned = true, f.info = pairs_info_bytes(b.n_logs, b.n_pairs);
  if (b.n_logs < 0 || b.n_logs > 0x7fffffffll || b.n_out < 0) f.own_error = "negative size";
  f.items = b.n_pairs, f.n_ops = b.n_out, f.empty = b.n_pairs == 0 || b.n_logs == 0;
  f.index_names = "log_off / pair_a / pair_b / res_off", f.index_ok = b.log_off && b.pair_a && b.pair_b && b.res_off;
  return f;
}

// The launches that fill the class counts and lists (with `large` also large_list, else null)
// from the workspace's `info` region: k_batch_classify, or the pairs form's two kernels.
template <typename B>
static int batch_prepass(const B& b, u32* cnt, char*, u32* lists, size_t stride, u32* large_list, bool large,
                         hipStream_t st) {
  auto* classify = large ? k_batch_classify<B, true> : k_batch_classify<B, false>;
  hipLaunchKernelGGL(classify, dim3(1), dim3(256), 0, st, b, cnt, lists, stride, large_list);
  HIP_TRY(hipGetLastError());
  return SMX_OK;
}
static int batch_prepass(const smx_pairs& b, u32* cnt, char* info, u32* lists, size_t stride, u32* large_list,
                         bool large, hipStream_t st) {
  i32* linfo = (i32*)info;
  i32* rinfo = (i32*)(info + batch_list_bytes(b.n_logs));
  hipLaunchKernelGGL(k_pairs_offsets, dim3(1), dim3(1024), 0, st, b, cnt, linfo, rinfo);
  HIP_TRY(hipGetLastError());
  auto* classify = large ? k_pairs_classify<true> : k_pairs_classify<false>;
  hipLaunchKernelGGL(classify, dim3((unsigned)SMX_CEIL_DIV(b.n_pairs, (i64)BATCH_CHUNK)), dim3(256), 0, st, b, cnt,
                     (const i32*)linfo, (const i32*)rinfo, lists, stride, large_list);
  HIP_TRY(hipGetLastError());
  return SMX_OK;
}

// The size queries of smx_batch and smx_batch_shared (n_shared 0).  Without the flag the size
// depends on n_merges alone, and n_total and n_shared are not looked at.
static int batch_ws_query(int64_t n_merges, int64_t n_total, int64_t n_shared, uint32_t flags, size_t* bytes) {
  if (flags & ~(uint32_t)SMX_BATCH_LARGE) return smx_set_error(SMX_E_ARG, "unknown smx_compose_batch_ex flag");
  if (!bytes) return smx_set_error(SMX_E_ARG, "null bytes");
  if (n_merges < 0 || n_merges > 0x7fffffffll) return smx_set_error(SMX_E_ARG, "n_merges outside 0 .. 2^31 - 1");
  const bool large = (flags & SMX_BATCH_LARGE) != 0;
  int64_t n_out = 0;
  if (large) {
    if (n_total < 0 || n_shared < 0 || n_shared > n_total)
      return smx_set_error(SMX_E_ARG, "n_total negative, or n_shared outside 0 .. n_total");
    n_out = n_total - n_shared + n_merges * n_shared;
    if (n_total > 0x7fffffffll || n_out > 0x7fffffffll)
      return smx_set_error(SMX_E_ARG, "SMX_BATCH_LARGE: n_total (shared: or n_out) over 2^31 - 1");
  }
  *bytes = batch_ws_size(0, n_merges, n_out, large).total;
  return SMX_OK;
}

extern "C" int smx_compose_batch_ex_workspace_bytes(int64_t n_merges, int64_t n_total, uint32_t flags, size_t* bytes) {
  return batch_ws_query(n_merges, n_total, 0, flags, bytes);
}

extern "C" int smx_compose_batch_shared_ex_workspace_bytes(int64_t n_merges, int64_t n_total, int64_t n_shared,
                                                           uint32_t flags, size_t* bytes) {
  return batch_ws_query(n_merges, n_total, n_shared, flags, bytes);
}

extern "C" int smx_compose_batch_workspace_bytes(int64_t n_merges, size_t* bytes) {
  return smx_compose_batch_ex_workspace_bytes(n_merges, 0, 0u, bytes);
}

extern "C" int smx_compose_batch_shared_workspace_bytes(int64_t n_merges, size_t* bytes) {
  return smx_compose_batch_shared_ex_workspace_bytes(n_merges, 0, 0, 0u, bytes);  // the same class counts and lists
}

extern "C" int smx_compose_pairs_workspace_bytes(int64_t n_logs, int64_t n_pairs, int64_t n_out, uint32_t flags,
                                                 size_t* bytes) {
  if (flags & ~(uint32_t)SMX_BATCH_LARGE) return smx_set_error(SMX_E_ARG, "unknown smx_compose_pairs flag");
  if (!bytes) return smx_set_error(SMX_E_ARG, "null bytes");
  if (n_logs < 0 || n_logs > 0x7fffffffll || n_pairs < 0 || n_pairs > 0x7fffffffll || n_out < 0)
    return smx_set_error(SMX_E_ARG, "n_logs or n_pairs outside 0 .. 2^31 - 1, or n_out negative");
  const bool large = (flags & SMX_BATCH_LARGE) != 0;
  if (large && n_out > 0x7fffffffll) return smx_set_error(SMX_E_ARG, "SMX_BATCH_LARGE: n_out over 2^31 - 1");
  *bytes = batch_ws_size(pairs_info_bytes(n_logs, n_pairs), n_pairs, n_out, large).total;
  return SMX_OK;
}

// What the three structs are checked for, in the order that decides which failure a caller
// sees; `name`: the entry point; *form: the struct's batch_form, for batch_run.  (An empty batch
// is valid whatever else it holds; batch_run returns at once on it.)
template <typename B>
static int batch_check_args(const char* name, const B* b, const void* workspace, size_t workspace_bytes,
                            uint32_t flags, BatchForm* form) {
  const bool large = (flags & SMX_BATCH_LARGE) != 0;
  if (flags & ~(uint32_t)SMX_BATCH_LARGE)
    return smx_set_error(SMX_E_ARG, (std::string("unknown ") + name + " flag").c_str());
  if (!b) return smx_set_error(SMX_E_ARG, "null batch struct");
  const BatchForm& f = *form = batch_form(*b);
  if (f.items < 0 || f.items > 0x7fffffffll || b->n_total < 0 || b->n_sym < 0 || b->grid_cap < 0)
    return smx_set_error(SMX_E_ARG, "negative size");
  if (f.own_error) return smx_set_error(SMX_E_ARG, f.own_error);
  if (b->n_sym > 0xffffffffll) return smx_set_error(SMX_E_ARG, "n_sym over 2^32 - 1");
  if (large && (b->n_total > 0x7fffffffll || f.n_ops > 0x7fffffffll))
    return smx_set_error(SMX_E_ARG, "SMX_BATCH_LARGE: n_total or n_out (the result entries) over 2^31 - 1");
  if (f.empty) return SMX_OK;
  if (!f.index_ok || !b->conf_off || !b->counts || !b->conflicts)
    return smx_set_error(SMX_E_ARG,
                         (std::string("null ") + f.index_names + " / conf_off / counts / conflicts").c_str());
  if (b->n_total > 0 && (!b->kind || !b->ts || !b->oid_hi || !b->oid_lo || !b->sym || !b->v0 || !b->v1))
    return smx_set_error(SMX_E_ARG, "null column");
  // (a shared batch of at least one merge has result entries exactly when n_total > 0)
  if (f.n_ops > 0 && (!b->order || !b->addr || !b->file || !b->ctx))
    return smx_set_error(SMX_E_ARG, "null result array");
  const bool aligned = large || f.aligned;
  if (!workspace || workspace_bytes < batch_ws_size(f.info, f.items, f.n_ops, large).total ||
      (aligned && ((uintptr_t)workspace & 7)))
    return smx_set_error(SMX_E_WORKSPACE,
                         (std::string("workspace too small") + (aligned ? " or not 8-byte aligned (" : " (") +
                          (flags ? std::string(name) + "_workspace_bytes" : f.plain_query) + ")").c_str());
  (void)hipGetLastError();  // an earlier call's error (any library's) is not this call's
  return SMX_OK;
}

// The checks; then the form's pre-pass and the three classes' k_compose_batch, with
// SMX_BATCH_LARGE the fourth list's k_compose_batch_large after them.
template <typename B>
static int batch_run(const char* name, const B* b, void* workspace, size_t workspace_bytes, uint32_t flags,
                     void* stream) {
  BatchForm f;
  if (int rc = batch_check_args(name, b, workspace, workspace_bytes, flags, &f)) return rc;
  if (f.empty) return SMX_OK;
  try {
    const int* resident;
    if (int rc = resident_of(&resident)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const bool large = (flags & SMX_BATCH_LARGE) != 0;
    const size_t stride = batch_list_bytes(f.items) / 4;
    u32* cnt = (u32*)workspace;
    char* info = (char*)workspace + BATCH_HDR;
    u32* lists = (u32*)(info + f.info);
    const size_t base = batch_ws_size(f.info, f.items, f.n_ops, large).base;
    const BatchLargeWs x = large ? batch_large_ws((char*)workspace + base, f.items, f.n_ops) : BatchLargeWs{};
    if (int rc = batch_prepass(*b, cnt, info, lists, stride, x.list, large, st)) return rc;
    if (int rc = launch_classes(kBatchKernels<B>, kBatchCaps, resident + f.first, f.items, b->grid_cap, st, cnt, lists,
                                stride, *b))
      return rc;
    if (large) {
      hipLaunchKernelGGL(k_compose_batch_large<B>, capped_grid(resident[f.first_large], f.items, b->grid_cap),
                         dim3(LARGE_NT), 0, st, *b, (const u32*)(cnt + BATCH_CLASSES), x);
      HIP_TRY(hipGetLastError());
    }
    return SMX_OK;
  } catch (const std::exception& e) {
    return smx_set_error(SMX_E_HIP, e.what());
  }
}

extern "C" int smx_compose_batch_ex(const smx_batch* b, void* workspace, size_t workspace_bytes, uint32_t flags,
                                    void* stream) {
  return batch_run(__func__, b, workspace, workspace_bytes, flags, stream);
}

extern "C" int smx_compose_batch(const smx_batch* b, void* workspace, size_t workspace_bytes, void* stream) {
  return smx_compose_batch_ex(b, workspace, workspace_bytes, 0u, stream);
}

extern "C" int smx_compose_batch_shared_ex(const smx_batch_shared* b, void* workspace, size_t workspace_bytes,
                                           uint32_t flags, void* stream) {
  return batch_run(__func__, b, workspace, workspace_bytes, flags, stream);
}

extern "C" int smx_compose_batch_shared(const smx_batch_shared* b, void* workspace, size_t workspace_bytes,
                                        void* stream) {
  return smx_compose_batch_shared_ex(b, workspace, workspace_bytes, 0u, stream);
}

extern "C" int smx_compose_pairs(const struct smx_pairs* b, void* workspace, size_t workspace_bytes, uint32_t flags,
                                 void* stream) {
  return batch_run(__func__, b, workspace, workspace_bytes, flags, stream);
}

// ---- what the four entry points over trains and trees (smx_compose_train, smx_compose_tree,
// smx_screen_train, smx_screen_tree) share on the host ----

// The six columns every form reads, n_total > 0 of them (the compose forms read v1 too).
template <typename B>
static bool train_columns_set(const B* b) {
  return b->kind && b->ts && b->oid_hi && b->oid_lo && b->sym && b->v0;
}

// What the two compose forms check of their columns and result arrays alike.
template <typename B>
static int train_compose_arrays(const B* b) {
  if (b->n_total > 0 && !(train_columns_set(b) && b->v1)) return smx_set_error(SMX_E_ARG, "null column");
  if (b->n_total > 0 && b->empty_str >= 0 && !b->v1_alt) return smx_set_error(SMX_E_ARG, "null v1_alt with empty_str set");
  if (b->n_out > 0 && (!b->src || !b->addr || !b->file || !b->ctx)) return smx_set_error(SMX_E_ARG, "null result array");
  return SMX_OK;
}

// The workspace check, the last one of each; `query` names the entry point's own size query.
static int train_ws_check(const void* workspace, size_t workspace_bytes, size_t need, const char* query) {
  if (!workspace || ((uintptr_t)workspace & 7) || workspace_bytes < need)
    return smx_set_error(SMX_E_WORKSPACE,
                         (std::string("workspace too small or not 8-byte aligned (") + query + ")").c_str());
  (void)hipGetLastError();  // an earlier call's error (any library's) is not this call's
  return SMX_OK;
}

// min(resident, items) workgroups as capped_grid, and one where there is no item: the per-log
// launches of a call whose trains name no log.
static dim3 capped_grid_min1(int resident, i64 items, i64 grid_cap) {
  return capped_grid(resident, items > 0 ? items : 1, grid_cap);
}

// The screen's two extraction kernels over every log of a screen of trains or of a tree.
template <typename B>
static int screen_extract_logs(const B& b, const int* resident, hipStream_t st, const ScreenWs& w,
                               const ScreenLargeWs& x) {
  const ScreenArgs s = screen_step_logs(b);
  hipLaunchKernelGGL(k_screen_extract, capped_grid_min1(resident[R_EXTRACT], b.n_logs, b.grid_cap), dim3(SCREEN_T1), 0,
                     st, s, w);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_screen_extract_large, capped_grid_min1(resident[R_EXTRACT_LARGE], b.n_logs, b.grid_cap),
                     dim3(SCREEN_TL), 0, st, s, w, x);
  HIP_TRY(hipGetLastError());
  return SMX_OK;
}

// The class launch once per level of a tree: level d's counts are lcnt + 4 * d, and the kernels
// take d after their own arguments.
template <typename K, typename... A>
static int launch_levels(K* const (&kern)[3], const int (&cap)[3], const int* resident, i64 n_levels, i64 items,
                         i64 grid_cap, hipStream_t st, const u32* lcnt, const u32* lists, size_t stride,
                         const A&... args) {
  for (i32 d = 0; d < (i32)n_levels; ++d)
    if (int rc = launch_classes(kern, cap, resident, items, grid_cap, st, lcnt + 4 * d, lists, stride, args..., d))
      return rc;
  return SMX_OK;
}

extern "C" int smx_compose_train_workspace_bytes(int64_t n_logs, int64_t n_trains, int64_t n_steps, int64_t n_out,
                                                 uint32_t flags, size_t* bytes) {
  if (flags) return smx_set_error(SMX_E_ARG, "unknown smx_compose_train flag");
  if (!bytes) return smx_set_error(SMX_E_ARG, "null bytes");
  if (n_logs < 0 || n_logs > 0x7fffffffll || n_trains < 0 || n_trains > 0x7fffffffll || n_steps < 0 ||
      n_steps > 0x7fffffffll || n_out < 0 || n_out > 0x7fffffffll)
    return smx_set_error(SMX_E_ARG, "n_logs, n_trains, n_steps or n_out outside 0 .. 2^31 - 1");
  *bytes = train_ws_bytes(n_logs, n_trains, n_out);
  return SMX_OK;
}

// The checks; then the pre-pass (k_train_offsets, k_train_classify) and the three classes'
// k_compose_train.
extern "C" int smx_compose_train(const struct smx_train* b, void* workspace, size_t workspace_bytes, uint32_t flags,
                                 void* stream) {
  if (flags) return smx_set_error(SMX_E_ARG, "unknown smx_compose_train flag");
  if (!b) return smx_set_error(SMX_E_ARG, "null train struct");
  if (b->n_logs < 0 || b->n_total < 0 || b->n_trains < 0 || b->n_steps < 0 || b->n_sym < 0 || b->n_out < 0 ||
      b->grid_cap < 0 || b->empty_str < SMX_NONE)
    return smx_set_error(SMX_E_ARG, "negative size, or empty_str below SMX_NONE");
  if (b->n_sym > 0xffffffffll) return smx_set_error(SMX_E_ARG, "n_sym over 2^32 - 1");
  if (b->n_logs > 0x7fffffffll || b->n_trains > 0x7fffffffll || b->n_steps > 0x7fffffffll)
    return smx_set_error(SMX_E_ARG, "n_logs, n_trains or n_steps over 2^31 - 1");
  if (b->n_total > 0x7fffffffll || b->n_out > 0x7fffffffll)
    return smx_set_error(SMX_E_ARG, "n_total or n_out over 2^31 - 1");
  if (b->n_trains == 0) return SMX_OK;
  if (!b->train_off || !b->res_off || !b->counts) return smx_set_error(SMX_E_ARG, "null train_off / res_off / counts");
  if (b->n_logs > 0 && !b->log_off) return smx_set_error(SMX_E_ARG, "null log_off");
  if (b->n_steps > 0 && (!b->train_log || !b->conf_off || !b->step_counts || !b->conflicts))
    return smx_set_error(SMX_E_ARG, "null train_log / conf_off / step_counts / conflicts");
  if (int rc = train_compose_arrays(b)) return rc;
  if (int rc = train_ws_check(workspace, workspace_bytes, train_ws_bytes(b->n_logs, b->n_trains, b->n_out),
                              "smx_compose_train_workspace_bytes"))
    return rc;
  try {
    const int* resident;
    if (int rc = resident_of(&resident)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const TrainWs w = train_ws(workspace, b->n_logs, b->n_trains, b->n_out);
    hipLaunchKernelGGL(k_train_offsets, dim3(1), dim3(1024), 0, st, *b, w);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_train_classify, dim3((unsigned)SMX_CEIL_DIV(b->n_trains, (i64)256)), dim3(256), 0, st, *b, w);
    HIP_TRY(hipGetLastError());
    return launch_classes(kTrainKernels, kBatchCaps, resident + R_TRAIN, b->n_trains, b->grid_cap, st, w.cnt, w.lists,
                          w.stride, *b, w);
  } catch (const std::exception& e) {
    return smx_set_error(SMX_E_HIP, e.what());
  }
}

extern "C" int smx_compose_tree_workspace_bytes(int64_t n_logs, int64_t n_nodes, int64_t n_levels, int64_t n_out,
                                                uint32_t flags, size_t* bytes) {
  if (flags) return smx_set_error(SMX_E_ARG, "unknown smx_compose_tree flag");
  if (!bytes) return smx_set_error(SMX_E_ARG, "null bytes");
  if (n_logs < 0 || n_logs > 0x7fffffffll || n_nodes < 0 || n_nodes > 0x7fffffffll || n_out < 0 ||
      n_out > 0x7fffffffll)
    return smx_set_error(SMX_E_ARG, "n_logs, n_nodes or n_out outside 0 .. 2^31 - 1");
  if (n_levels < 0 || n_levels > TREE_MAX_LEVELS)
    return smx_set_error(SMX_E_ARG, "n_levels outside 0 .. SMX_TREE_MAX_LEVELS");
  *bytes = tree_ws_bytes(n_logs, n_nodes, n_levels, n_out);
  return SMX_OK;
}

// The checks; then the pre-pass (k_tree_prepass) and, level by level, the three classes'
// k_compose_tree.
extern "C" int smx_compose_tree(const struct smx_tree* b, void* workspace, size_t workspace_bytes, uint32_t flags,
                                void* stream) {
  if (flags) return smx_set_error(SMX_E_ARG, "unknown smx_compose_tree flag");
  if (!b) return smx_set_error(SMX_E_ARG, "null tree struct");
  if (b->n_logs < 0 || b->n_total < 0 || b->n_nodes < 0 || b->n_levels < 0 || b->n_sym < 0 || b->n_out < 0 ||
      b->grid_cap < 0 || b->empty_str < SMX_NONE)
    return smx_set_error(SMX_E_ARG, "negative size, or empty_str below SMX_NONE");
  if (b->n_levels > TREE_MAX_LEVELS) return smx_set_error(SMX_E_ARG, "n_levels over SMX_TREE_MAX_LEVELS");
  if (b->n_sym > 0xffffffffll) return smx_set_error(SMX_E_ARG, "n_sym over 2^32 - 1");
  if (b->n_logs > 0x7fffffffll || b->n_nodes > 0x7fffffffll) return smx_set_error(SMX_E_ARG, "n_logs or n_nodes over 2^31 - 1");
  if (b->n_total > 0x7fffffffll || b->n_out > 0x7fffffffll)
    return smx_set_error(SMX_E_ARG, "n_total or n_out over 2^31 - 1");
  if (b->n_nodes == 0) return SMX_OK;
  if (!b->level_off || !b->node_parent || !b->node_log || !b->res_off || !b->conf_off || !b->conflicts ||
      !b->node_counts || !b->node_acc)
    return smx_set_error(SMX_E_ARG,
                         "null level_off / node_parent / node_log / res_off / conf_off / conflicts / node_counts / node_acc");
  if (b->n_logs > 0 && !b->log_off) return smx_set_error(SMX_E_ARG, "null log_off");
  if (int rc = train_compose_arrays(b)) return rc;
  if (int rc = train_ws_check(workspace, workspace_bytes, tree_ws_bytes(b->n_logs, b->n_nodes, b->n_levels, b->n_out),
                              "smx_compose_tree_workspace_bytes"))
    return rc;
  try {
    const int* resident;
    if (int rc = resident_of(&resident)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const TreeWs w = tree_ws(workspace, b->n_logs, b->n_nodes, b->n_levels, b->n_out);
    hipLaunchKernelGGL(k_tree_prepass, dim3(1), dim3(1024), 0, st, *b, w);
    HIP_TRY(hipGetLastError());
    return launch_levels(kTreeKernels, kBatchCaps, resident + R_TREE, b->n_levels, b->n_nodes, b->grid_cap, st, w.lcnt,
                         w.lists, w.stride, *b, w);
  } catch (const std::exception& e) {
    return smx_set_error(SMX_E_HIP, e.what());
  }
}

// What smx_train_stage and smx_train_land check alike: the struct's sizes.  *n: n_acc + log_n.
static int train_step_sizes(const char* name, const smx_train_step* s, i64* n) {
  if (!s) return smx_set_error(SMX_E_ARG, (std::string(name) + ": null train step struct").c_str());
  if (s->n_total < 0 || s->n_sym < 0 || s->n_acc < 0 || s->log_lo < 0 || s->log_n < 0 || s->conflict_cap < 0 ||
      s->record_cap < 0 || s->empty_str < SMX_NONE)
    return smx_set_error(SMX_E_ARG, (std::string(name) + ": negative size, or empty_str below SMX_NONE").c_str());
  if (s->n_total > 0x7fffffffll || s->n_acc > 0x7fffffffll || s->log_n > 0x7fffffffll ||
      s->n_acc + s->log_n > 0x7fffffffll)
    return smx_set_error(SMX_E_ARG, (std::string(name) + ": n_total or n_acc + log_n over 2^31 - 1").c_str());
  if (s->log_lo + s->log_n > s->n_total)  // (both at most 2^31 - 1 here, or log_lo alone is past n_total)
    return smx_set_error(SMX_E_ARG, (std::string(name) + ": the log [log_lo, log_lo + log_n) leaves the columns").c_str());
  if (s->n_sym > 0xffffffffll) return smx_set_error(SMX_E_ARG, (std::string(name) + ": n_sym over 2^32 - 1").c_str());
  if (s->n_total > 0 && s->empty_str >= 0 && !s->v1_alt)
    return smx_set_error(SMX_E_ARG, (std::string(name) + ": null v1_alt with empty_str set").c_str());
  *n = s->n_acc + s->log_n;
  return SMX_OK;
}

// The checks; then status[0] cleared and k_train_stage, a thread per staged entry.
extern "C" int smx_train_stage(const struct smx_train_step* s, void* stream) {
  i64 n = 0;
  if (int rc = train_step_sizes(__func__, s, &n)) return rc;
  if (n == 0) return SMX_OK;
  if (!s->status) return smx_set_error(SMX_E_ARG, "smx_train_stage: null status");
  if (s->n_total > 0 && (!s->kind || !s->ts || !s->oid_hi || !s->oid_lo || !s->sym || !s->v0 || !s->v1))
    return smx_set_error(SMX_E_ARG, "smx_train_stage: null column");
  if (s->n_acc > 0 && (!s->acc_src || !s->acc_addr || !s->acc_file))
    return smx_set_error(SMX_E_ARG, "smx_train_stage: null accumulator array");
  if (!s->st_kind || !s->st_ts || !s->st_oid_hi || !s->st_oid_lo || !s->st_sym || !s->st_v0 || !s->st_v1)
    return smx_set_error(SMX_E_ARG, "smx_train_stage: null staged column");
  (void)hipGetLastError();  // an earlier call's error (any library's) is not this call's
  try {
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(s->status, 0, sizeof(int64_t), st));
    hipLaunchKernelGGL(k_train_stage, dim3(train_step_grid(n)), dim3(TRAIN_STEP_T), 0, st, *s);
    HIP_TRY(hipGetLastError());
    return SMX_OK;
  } catch (const std::exception& e) {
    return smx_set_error(SMX_E_HIP, e.what());
  }
}

// The checks; then k_train_land, a thread per entry of the accumulator out (or per record).
extern "C" int smx_train_land(const struct smx_train_step* s, void* stream) {
  i64 n = 0;
  if (int rc = train_step_sizes(__func__, s, &n)) return rc;
  if (n == 0) return SMX_OK;
  if (!s->status || !s->counts) return smx_set_error(SMX_E_ARG, "smx_train_land: null status / counts");
  if (!s->order || !s->addr || !s->file || !s->ctx) return smx_set_error(SMX_E_ARG, "smx_train_land: null result array");
  if (!s->out_src || !s->out_addr || !s->out_file || !s->out_ctx)
    return smx_set_error(SMX_E_ARG, "smx_train_land: null accumulator out");
  if (s->n_acc > 0 && (!s->acc_src || !s->acc_addr || !s->acc_file || !s->acc_ctx))
    return smx_set_error(SMX_E_ARG, "smx_train_land: null accumulator array");
  if (s->conflict_cap > 0 && !s->conflicts) return smx_set_error(SMX_E_ARG, "smx_train_land: null conflicts");
  if (s->record_cap > 0 && !s->records) return smx_set_error(SMX_E_ARG, "smx_train_land: null records");
  const int32_t* const in[4] = {s->acc_src, s->acc_addr, s->acc_file, s->acc_ctx};
  const int32_t* const out[4] = {s->out_src, s->out_addr, s->out_file, s->out_ctx};
  for (const int32_t* o : out)
    for (const int32_t* i : in)
      if (o == i) return smx_set_error(SMX_E_ARG, "smx_train_land: the accumulator out aliases the accumulator in");
  (void)hipGetLastError();  // an earlier call's error (any library's) is not this call's
  try {
    hipLaunchKernelGGL(k_train_land, dim3(train_step_grid(n)), dim3(TRAIN_STEP_T), 0, (hipStream_t)stream, *s);
    HIP_TRY(hipGetLastError());
    return SMX_OK;
  } catch (const std::exception& e) {
    return smx_set_error(SMX_E_HIP, e.what());
  }
}

extern "C" int smx_screen_train_workspace_bytes(int64_t n_logs, int64_t n_total, int64_t n_trains, int64_t n_steps,
                                                int64_t n_acc, uint32_t flags, size_t* bytes) {
  if (flags) return smx_set_error(SMX_E_ARG, "unknown smx_screen_train flag");
  if (!bytes) return smx_set_error(SMX_E_ARG, "null bytes");
  for (int64_t v : {n_logs, n_total, n_trains, n_steps, n_acc})
    if (v < 0 || v > 0x7fffffffll)
      return smx_set_error(SMX_E_ARG, "n_logs, n_total, n_trains, n_steps or n_acc outside 0 .. 2^31 - 1");
  *bytes = screen_train_ws_bytes(n_logs, n_total, n_trains, n_acc);
  return SMX_OK;
}

// The checks; then the pre-pass (k_screen_train_offsets), the screen's two extraction kernels
// over every log, k_screen_train_classify and the three classes' k_screen_train.
extern "C" int smx_screen_train(const struct smx_screen_train* b, void* workspace, size_t workspace_bytes,
                                uint32_t flags, void* stream) {
  if (flags) return smx_set_error(SMX_E_ARG, "unknown smx_screen_train flag");
  if (!b) return smx_set_error(SMX_E_ARG, "null screen train struct");
  if (b->n_logs < 0 || b->n_total < 0 || b->n_trains < 0 || b->n_steps < 0 || b->n_acc < 0 || b->grid_cap < 0)
    return smx_set_error(SMX_E_ARG, "negative size");
  if (b->n_logs > 0x7fffffffll || b->n_total > 0x7fffffffll || b->n_trains > 0x7fffffffll ||
      b->n_steps > 0x7fffffffll || b->n_acc > 0x7fffffffll)
    return smx_set_error(SMX_E_ARG, "n_logs, n_total, n_trains, n_steps or n_acc over 2^31 - 1");
  if ((b->conflicts == nullptr) != (b->conf_off == nullptr))
    return smx_set_error(SMX_E_ARG, "conflicts and conf_off are both null or both set");
  if (b->n_trains == 0) return SMX_OK;
  if (!b->train_off || !b->acc_off || !b->counts) return smx_set_error(SMX_E_ARG, "null train_off / acc_off / counts");
  if (b->n_logs > 0 && !b->log_off) return smx_set_error(SMX_E_ARG, "null log_off");
  if (b->n_steps > 0 && (!b->train_log || !b->step_counts))
    return smx_set_error(SMX_E_ARG, "null train_log / step_counts");
  if (b->n_total > 0 && !train_columns_set(b)) return smx_set_error(SMX_E_ARG, "null column");
  if (int rc = train_ws_check(workspace, workspace_bytes,
                              screen_train_ws_bytes(b->n_logs, b->n_total, b->n_trains, b->n_acc),
                              "smx_screen_train_workspace_bytes"))
    return rc;
  try {
    const int* resident;
    if (int rc = resident_of(&resident)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const ScreenWs w = screen_ws(workspace, b->n_logs, screen_train_records(b->n_total, b->n_acc), b->n_trains);
    const ScreenTrainWs y = screen_train_ws(workspace, b->n_logs, b->n_total, b->n_trains, b->n_acc);
    hipLaunchKernelGGL(k_screen_train_offsets, dim3(1), dim3(1024), 0, st, *b, w, y);
    HIP_TRY(hipGetLastError());
    if (int rc = screen_extract_logs(*b, resident, st, w, y.x)) return rc;
    hipLaunchKernelGGL(k_screen_train_classify, dim3((unsigned)SMX_CEIL_DIV(b->n_trains, (i64)256)), dim3(256), 0, st,
                       *b, w, y);
    HIP_TRY(hipGetLastError());
    return launch_classes(kScreenTrainKernels, kScreenCaps, resident + R_SCREEN_TRAIN, b->n_trains, b->grid_cap, st,
                          w.cnt, w.lists, w.list_stride, *b, w);
  } catch (const std::exception& e) {
    return smx_set_error(SMX_E_HIP, e.what());
  }
}

extern "C" int smx_screen_tree_workspace_bytes(int64_t n_logs, int64_t n_total, int64_t n_nodes, int64_t n_levels,
                                               int64_t n_acc, uint32_t flags, size_t* bytes) {
  if (flags) return smx_set_error(SMX_E_ARG, "unknown smx_screen_tree flag");
  if (!bytes) return smx_set_error(SMX_E_ARG, "null bytes");
  for (int64_t v : {n_logs, n_total, n_nodes, n_acc})
    if (v < 0 || v > 0x7fffffffll)
      return smx_set_error(SMX_E_ARG, "n_logs, n_total, n_nodes or n_acc outside 0 .. 2^31 - 1");
  if (n_levels < 0 || n_levels > TREE_MAX_LEVELS)
    return smx_set_error(SMX_E_ARG, "n_levels outside 0 .. SMX_TREE_MAX_LEVELS");
  *bytes = screen_tree_ws_bytes(n_logs, n_total, n_nodes, n_levels, n_acc);
  return SMX_OK;
}

// The checks; then the offsets' pre-pass (k_screen_tree_offsets), the screen's two extraction
// kernels over every log, the nodes' pre-pass (k_screen_tree_prepass) and, level by level, the
// three classes' k_screen_tree.
extern "C" int smx_screen_tree(const struct smx_screen_tree* b, void* workspace, size_t workspace_bytes,
                               uint32_t flags, void* stream) {
  if (flags) return smx_set_error(SMX_E_ARG, "unknown smx_screen_tree flag");
  if (!b) return smx_set_error(SMX_E_ARG, "null screen tree struct");
  if (b->n_logs < 0 || b->n_total < 0 || b->n_nodes < 0 || b->n_levels < 0 || b->n_acc < 0 || b->grid_cap < 0)
    return smx_set_error(SMX_E_ARG, "negative size");
  if (b->n_levels > TREE_MAX_LEVELS) return smx_set_error(SMX_E_ARG, "n_levels over SMX_TREE_MAX_LEVELS");
  if (b->n_logs > 0x7fffffffll || b->n_total > 0x7fffffffll || b->n_nodes > 0x7fffffffll || b->n_acc > 0x7fffffffll)
    return smx_set_error(SMX_E_ARG, "n_logs, n_total, n_nodes or n_acc over 2^31 - 1");
  if ((b->conflicts == nullptr) != (b->conf_off == nullptr))
    return smx_set_error(SMX_E_ARG, "conflicts and conf_off are both null or both set");
  if (b->n_nodes == 0) return SMX_OK;
  if (!b->level_off || !b->node_parent || !b->node_log || !b->acc_off || !b->node_counts)
    return smx_set_error(SMX_E_ARG, "null level_off / node_parent / node_log / acc_off / node_counts");
  if (b->n_logs > 0 && !b->log_off) return smx_set_error(SMX_E_ARG, "null log_off");
  if (b->n_total > 0 && !train_columns_set(b)) return smx_set_error(SMX_E_ARG, "null column");
  if (int rc = train_ws_check(workspace, workspace_bytes,
                              screen_tree_ws_bytes(b->n_logs, b->n_total, b->n_nodes, b->n_levels, b->n_acc),
                              "smx_screen_tree_workspace_bytes"))
    return rc;
  try {
    const int* resident;
    if (int rc = resident_of(&resident)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const ScreenWs w = screen_ws(workspace, b->n_logs, b->n_total + b->n_acc, b->n_nodes);
    const ScreenTreeWs y = screen_tree_ws(workspace, b->n_logs, b->n_total, b->n_nodes, b->n_levels, b->n_acc);
    hipLaunchKernelGGL(k_screen_tree_offsets, dim3(1), dim3(1024), 0, st, *b, w, y);
    HIP_TRY(hipGetLastError());
    if (int rc = screen_extract_logs(*b, resident, st, w, y.x)) return rc;
    hipLaunchKernelGGL(k_screen_tree_prepass, dim3(1), dim3(1024), 0, st, *b, w, y);
    HIP_TRY(hipGetLastError());
    return launch_levels(kScreenTreeKernels, kScreenCaps, resident + R_SCREEN_TREE, b->n_levels, b->n_nodes, b->grid_cap,
                         st, y.lcnt, w.lists, w.list_stride, *b, w, y);
  } catch (const std::exception& e) {
    return smx_set_error(SMX_E_HIP, e.what());
  }
}

extern "C" int smx_screen_ex_workspace_bytes(int64_t n_logs, int64_t n_total, int64_t n_pairs, uint32_t flags,
                                             size_t* bytes) {
  if (flags & ~(uint32_t)SMX_SCREEN_LARGE) return smx_set_error(SMX_E_ARG, "unknown smx_screen_ex flag");
  if (!bytes) return smx_set_error(SMX_E_ARG, "null bytes");
  if (n_logs < 0 || n_logs > 0x7fffffffll || n_pairs < 0 || n_pairs > 0x7fffffffll || n_total < 0)
    return smx_set_error(SMX_E_ARG, "n_logs or n_pairs outside 0 .. 2^31 - 1, or n_total negative");
  const bool large = (flags & SMX_SCREEN_LARGE) != 0;
  if (large && n_total > 0x7fffffffll) return smx_set_error(SMX_E_ARG, "SMX_SCREEN_LARGE: n_total over 2^31 - 1");
  *bytes = screen_ws_bytes(n_logs, n_total, n_pairs) + (large ? screen_large_bytes(n_total, n_pairs) : 0);
  return SMX_OK;
}

extern "C" int smx_screen_workspace_bytes(int64_t n_logs, int64_t n_total, int64_t n_pairs, size_t* bytes) {
  return smx_screen_ex_workspace_bytes(n_logs, n_total, n_pairs, 0u, bytes);
}

extern "C" int smx_screen_ex(const struct smx_screen* s, void* workspace, size_t workspace_bytes, uint32_t flags,
                             void* stream) {
  if (flags & ~(uint32_t)SMX_SCREEN_LARGE) return smx_set_error(SMX_E_ARG, "unknown smx_screen_ex flag");
  const bool large = (flags & SMX_SCREEN_LARGE) != 0;
  if (!s) return smx_set_error(SMX_E_ARG, "null screen");
  if (s->n_logs < 0 || s->n_logs > 0x7fffffffll || s->n_pairs < 0 || s->n_pairs > 0x7fffffffll || s->n_total < 0 ||
      s->grid_cap < 0)
    return smx_set_error(SMX_E_ARG, "negative size");
  if (large && s->n_total > 0x7fffffffll) return smx_set_error(SMX_E_ARG, "SMX_SCREEN_LARGE: n_total over 2^31 - 1");
  if ((s->conflicts == nullptr) != (s->conf_off == nullptr))
    return smx_set_error(SMX_E_ARG, "conflicts and conf_off are both null or both set");
  if (s->n_pairs == 0 || s->n_logs == 0) return SMX_OK;
  if (!s->log_off || !s->pair_a || !s->pair_b || !s->counts)
    return smx_set_error(SMX_E_ARG, "null log_off / pair_a / pair_b / counts");
  if (s->n_total > 0 && (!s->kind || !s->ts || !s->oid_hi || !s->oid_lo || !s->sym || !s->v0))
    return smx_set_error(SMX_E_ARG, "null column");
  const size_t need = screen_ws_bytes(s->n_logs, s->n_total, s->n_pairs) +
                      (large ? screen_large_bytes(s->n_total, s->n_pairs) : 0);
  if (!workspace || ((uintptr_t)workspace & 7) || workspace_bytes < need)
    return smx_set_error(SMX_E_WORKSPACE, large ? "workspace too small or not 8-byte aligned (smx_screen_ex_workspace_bytes)"
                                                : "workspace too small or not 8-byte aligned (smx_screen_workspace_bytes)");
  (void)hipGetLastError();  // an earlier call's error (any library's) is not this call's
  try {
    const int* resident;
    if (int rc = resident_of(&resident)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const ScreenWs w = screen_ws(workspace, s->n_logs, s->n_total, s->n_pairs);
    const ScreenLargeWs x = large ? screen_large_ws(workspace, s->n_logs, s->n_total, s->n_pairs) : ScreenLargeWs{};
    const dim3 classify_grid((unsigned)SMX_CEIL_DIV(s->n_pairs, (i64)SCREEN_CHUNK));
    hipLaunchKernelGGL(k_screen_logs, dim3(1), dim3(1024), 0, st, *s, w);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_screen_extract, capped_grid(resident[R_EXTRACT], s->n_logs, s->grid_cap), dim3(SCREEN_T1), 0,
                       st, *s, w);
    HIP_TRY(hipGetLastError());
    if (large) {
      hipLaunchKernelGGL(k_screen_extract_large, capped_grid(resident[R_EXTRACT_LARGE], s->n_logs, s->grid_cap),
                         dim3(SCREEN_TL), 0, st, *s, w, x);
      HIP_TRY(hipGetLastError());
      hipLaunchKernelGGL(k_screen_classify<true>, classify_grid, dim3(256), 0, st, *s, w, x.list);
    } else {
      hipLaunchKernelGGL(k_screen_classify<false>, classify_grid, dim3(256), 0, st, *s, w, (u32*)nullptr);
    }
    HIP_TRY(hipGetLastError());
    if (int rc = launch_classes(kScreenKernels, kScreenCaps, resident + R_SCREEN, s->n_pairs, s->grid_cap, st, w.cnt,
                                w.lists, w.list_stride, *s, w))
      return rc;
    if (large) {
      hipLaunchKernelGGL(k_screen_stream, capped_grid(resident[R_STREAM], s->n_pairs, s->grid_cap), dim3(SCREEN_N / 2),
                         0, st, *s, w, w.cnt + SCREEN_CLASSES, x.list);
      HIP_TRY(hipGetLastError());
    }
    return SMX_OK;
  } catch (const std::exception& e) {
    return smx_set_error(SMX_E_HIP, e.what());
  }
}

extern "C" int smx_screen(const struct smx_screen* s, void* workspace, size_t workspace_bytes, void* stream) {
  return smx_screen_ex(s, workspace, workspace_bytes, 0u, stream);
}

extern "C" int smx_screen_candidates_workspace_bytes(int64_t n_logs, int64_t n_total, size_t* bytes) {
  if (!bytes) return smx_set_error(SMX_E_ARG, "null bytes");
  if (n_logs < 0 || n_logs > SMX_CAND_MAX_LOGS || n_total < 0 || n_total > 0x7fffffffll)
    return smx_set_error(SMX_E_ARG, "n_logs outside 0 .. SMX_CAND_MAX_LOGS or n_total outside 0 .. 2^31 - 1");
  *bytes = cand_ws_bytes(n_logs, n_total);
  return SMX_OK;
}

// Workgroups of BLOCK threads for `items` items, one each; at most `most`, and at most
// grid_cap when that is positive; at least one.
static dim3 cand_grid(i64 items, i64 most, i64 grid_cap) {
  i64 g = SMX_CEIL_DIV(items, (i64)BLOCK);
  if (g > most) g = most;
  if (grid_cap > 0 && g > grid_cap) g = grid_cap;
  return dim3((unsigned)(g > 0 ? g : 1));
}

extern "C" int smx_screen_candidates(const struct smx_candidates* c, void* workspace, size_t workspace_bytes,
                                     void* stream) {
  if (!c) return smx_set_error(SMX_E_ARG, "null candidates");
  if (c->n_logs < 0 || c->n_total < 0 || c->pair_cap < 0 || c->grid_cap < 0)
    return smx_set_error(SMX_E_ARG, "negative size");
  if (c->n_logs > SMX_CAND_MAX_LOGS || c->n_total > 0x7fffffffll)
    return smx_set_error(SMX_E_ARG, "n_logs over SMX_CAND_MAX_LOGS or n_total over 2^31 - 1");
  if (c->n_logs == 0) return SMX_OK;
  if (!c->log_off || !c->counts) return smx_set_error(SMX_E_ARG, "null log_off / counts");
  if (c->n_total > 0 && (!c->kind || !c->sym || !c->v0)) return smx_set_error(SMX_E_ARG, "null column");
  if (c->pair_cap > 0 && (!c->pair_a || !c->pair_b))
    return smx_set_error(SMX_E_ARG, "null pair_a / pair_b with pair_cap > 0");
  if (!workspace || ((uintptr_t)workspace & 7) || workspace_bytes < cand_ws_bytes(c->n_logs, c->n_total))
    return smx_set_error(SMX_E_WORKSPACE,
                         "workspace too small or not 8-byte aligned (smx_screen_candidates_workspace_bytes)");
  (void)hipGetLastError();  // an earlier call's error (any library's) is not this call's
  try {
    hipStream_t st = (hipStream_t)stream;
    const CandWs w = cand_ws(workspace, c->n_logs, c->n_total);
    const i64 n = c->n_total, cap = c->grid_cap;
    const int bits = cand_log_bits(c->n_logs);
    if (n > 0) HIP_TRY(hipMemsetAsync(w.keys, 0xff, (size_t)n * 8, st));  // CAND_NONE everywhere
    HIP_TRY(hipMemsetAsync(w.mat, 0, w.n_words * 4, st));
    hipLaunchKernelGGL(k_cand_logs, dim3(1), dim3(1024), 0, st, *c, w);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_cand_records, cand_grid(c->n_logs * BLOCK, c->n_logs, cap), dim3(BLOCK), 0, st, *c, w, bits);
    HIP_TRY(hipGetLastError());
    int shifts[8], nshift = 0;  // 33 + bits key bits: the records' and the sentinel's bit above them
    for (int s = 0; s < 33 + bits; s += 8) shifts[nshift++] = s;
    const RadixTemp tmp = {w.k2, w.v2, w.hist, nullptr};
    HIP_TRY(radix_sort_pairs(w.keys, w.vals, n, shifts, nshift, tmp, st));
    hipLaunchKernelGGL(k_cand_heads, cand_grid(n, 4096, cap), dim3(BLOCK), 0, st, w, n);
    HIP_TRY(hipGetLastError());
    HIP_TRY((scan_excl<OpSum, u32, u32>(w.flag, w.v2, n, nullptr, w.partials, w.n_ent, st)));
    hipLaunchKernelGGL(k_cand_entries, cand_grid(n, 4096, cap), dim3(BLOCK), 0, st, w, n);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_cand_pairs, cand_grid(n * (WAVE), CAND_PAIR_BLOCKS, cap), dim3(BLOCK), 0, st, *c, w, bits);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_cand_popc, cand_grid((i64)w.n_words, 4096, cap), dim3(BLOCK), 0, st, w);
    HIP_TRY(hipGetLastError());
    HIP_TRY((scan_excl<OpSum, u32, u32>(w.pop, w.wpos, (i64)w.n_words, nullptr, w.partials, w.n_cand, st)));
    hipLaunchKernelGGL(k_cand_emit, cand_grid((i64)w.n_words, 4096, cap), dim3(BLOCK), 0, st, *c, w);
    HIP_TRY(hipGetLastError());
    return SMX_OK;
  } catch (const std::exception& e) {
    return smx_set_error(SMX_E_HIP, e.what());
  }
}
