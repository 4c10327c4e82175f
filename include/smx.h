/*
 * smx.h — C ABI of the MI355X op-log composition library (libsmx.so).
 *
 * Replaces, as a drop-in behind the unchanged Python entry points:
 *   smx_compose   <- semmerge/compose.py:11-114  compose_oplogs(delta_a, delta_b)
 *                    (sort_key/_precedence :16-21,130-149; merge loop :51-112;
 *                     DivergentRename check :60-70,88-98 with conflict.py:34-49;
 *                     rename/move chains :27-28,71-82,99-110; materialize :30-49)
 *   smx_compose_batch <- the same loop for many independent merges of at most 2048 ops
 *                    each, in one call (a merge queue, a rebase, a monorepo)
 *   smx_compose_batch_shared <- the same, for merges that all have one log on one side,
 *                    stored once
 *   smx_compose_pairs <- the same, for pairs (i, j) over logs stored once, laid out as
 *                    smx_screen takes them
 *   smx_compose_train <- that loop in a loop: a merge train over such logs, each log
 *                    composed against what landed before it, conflicting logs put off
 *                    (what semmerge/__main__.py:65-69 does to one merge, per step)
 *   smx_compose_tree <- the same for trains that share prefixes (a speculative merge queue,
 *                    every prefix of a commit stack): a tree of logs, every node composed once
 *   smx_train_stage, smx_train_land <- one step of that loop for trains of any size: the
 *                    materialise, marshal and copy between two compose_oplogs calls, as two
 *                    gathers on either side of smx_compose
 *   smx_screen    <- the conflict list of the same loop alone (what semmerge/__main__.py
 *                    looks at first), for many pairs of logs, from the logs' renames
 *   smx_screen_train <- the conflict lists of smx_compose_train's steps alone, from the
 *                    logs' renames, for trains of any size
 *   smx_screen_tree <- the same for trains that share prefixes: smx_compose_tree's tree, every
 *                    node screened once, no size refused
 *   smx_rga_replay <- semmerge/crdt.py:23-57  RGA.insert/move/delete/materialize,
 *                    batched over many independent lists
 *   smx_rga_replay_onto <- the same, for many event streams replayed onto base lists that
 *                    are stored once (RGA._fold's shape, many branches per base list)
 *   smx_rga_replay_chain <- the same, for jobs that are runs of segments stored once (a
 *                    three-way reconcile base ++ target ++ pull request, what a merge train
 *                    landed, every prefix of a commit stack)
 *
 * Plain C types only.  All device pointers are HIP device (or managed) memory
 * owned by the caller; the library never allocates: temporary space comes from a
 * caller-provided workspace sized by the *_workspace_bytes queries.  Calls are
 * stream-ordered on `stream` (a hipStream_t passed as void*; NULL = the null
 * stream).  smx_compose performs one stream synchronisation (in smx_compose_finish)
 * to check its plan; smx_compose_batch performs none; read device-side counts only after
 * synchronising the stream.
 *
 * Reentrant: host threads may compose concurrently, each on its own stream and
 * workspace (the library's side stream and fork/join events are kept per caller
 * stream; tests/test_gpu_async.py runs two threads on one GPU).
 *
 * The library keeps no handle to the caller's stream after a call returns, so the
 * stream may be destroyed at any time.
 *
 * Return value: 0 on success, a negative SMX_E* code otherwise; the message is
 * available from smx_last_error() (thread-local).  Nothing aborts the process.
 */
#ifndef SMX_H
#define SMX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SMX_OK 0
#define SMX_E_ARG (-1)      /* bad argument / shape */
/* More conflicts than smx_compose_out.conflict_cap.  No entry point of the library returns
 * it: a merge is enqueued, not waited for, so the overflow shows in counts[1] (see
 * smx_compose_out), and the code is kept for callers that turn that into an error (the
 * Python wrapper's SmxError). */
#define SMX_E_CAPACITY (-2)
#define SMX_E_HIP (-3)      /* a HIP runtime call failed */
#define SMX_E_WORKSPACE (-4) /* workspace too small */

/* Dense precedence ranks (compose.py:130-149; unknown type -> 99 -> rank 17). */
#define SMX_KIND_MOVE 0     /* moveDecl, precedence 10 */
#define SMX_KIND_RENAME 1   /* renameSymbol, precedence 11 */
#define SMX_N_KINDS 18
#define SMX_NONE (-1)

/*
 * One merge's input: ops of branch A (indices [0, n_a)) followed by ops of
 * branch B (indices [n_a, n_a + n_b)), struct-of-arrays, device memory.
 *   kind[i]   precedence rank 0..17 of ops[i].type
 *   ts[i]     order-preserving key of str(provenance["timestamp"])
 *   oid_hi/lo order-preserving 128-bit key of ops[i].id
 *   sym[i]    interned target.symbolId, < n_sym
 *   v0[i]     rename: equality class of params["newName"] (conflict test)
 *             move:   string id of str(params["newAddress"]) or SMX_NONE
 *   v1[i]     rename: string id of str(params["newName"]) (rename chain value)
 *             move:   string id of str(params["newFile"] or params["file"]) or SMX_NONE
 *             other kinds: ignored
 */
typedef struct smx_ops {
  int64_t n_a;
  int64_t n_b;
  int64_t n_sym;
  const uint8_t* kind;
  const uint64_t* ts;
  const uint64_t* oid_hi;
  const uint64_t* oid_lo;
  const uint32_t* sym;
  const int32_t* v0;
  const int32_t* v1;
  /* B op j (j >= n_a) is stored at index j + b_gap of every field array (0: right
   * after A); the b_gap entries between the branches are not part of the merge.  A sharded merge
   * keeps headroom between its A and B ranges so its exchange moves only the ops that
   * change shard.  The presorted, presorted-wide and small plans take any b_gap >= 0;
   * the sorting plans (segmented, radix) need b_gap = 0: with b_gap > 0, smx_compose
   * returns SMX_E_ARG for branch logs that are not timestamp-ordered and for ordered
   * logs whose equal-timestamp groups no presorted window holds. */
  int64_t b_gap;
} smx_ops;

/*
 * Composed output, device memory, capacity n_a + n_b for the per-op arrays.
 *   order[k]      source index (into A||B) of the k-th composed op
 *   addr[k]       string id of the move-chain newAddress it sees, or SMX_NONE
 *   file[k]       string id of the move-chain newFile it sees, or SMX_NONE
 *   ctx[k]        string id of its renameContext (non-renames), or SMX_NONE
 *   conflicts     (a_idx, b_idx) pairs in the reference's discovery order;
 *                 capacity conflict_cap pairs, >= 0 (min(n_a, n_b) always suffices)
 *   counts[0]     number of composed ops, counts[1] number of conflicts
 * A conflict_cap smaller than the number of conflicts is not an error of the call (it
 * returns SMX_OK): counts[1] is the full number of conflicts, the first conflict_cap pairs
 * are written, nothing is written at or after conflicts[2 * conflict_cap], and the
 * composed ops (order, addr, file, ctx, counts[0]) are complete.  The caller compares
 * counts[1] with conflict_cap after synchronising the stream.
 */
typedef struct smx_compose_out {
  int32_t* order;
  int32_t* addr;
  int32_t* file;
  int32_t* ctx;
  int32_t* conflicts;
  int64_t conflict_cap;
  int64_t* counts;
} smx_compose_out;

/* Workspace needed by smx_compose for these sizes. */
int smx_compose_workspace_bytes(int64_t n_a, int64_t n_b, int64_t n_sym, size_t* bytes);

/* Compose one merge on the GPU (see the header comment for semantics).
 * = smx_compose_async followed by smx_compose_finish. */
int smx_compose(const smx_ops* ops, const smx_compose_out* out, void* workspace,
                size_t workspace_bytes, void* stream);

/* The same composition in two halves.  smx_compose_async enqueues the plan for
 * timestamp-ordered branch logs (what lift.ts emits) and every later stage with no
 * host synchronisation, so it can be captured in a hipGraph; after the stream has
 * run it, counts[0] >= 0 means the results are complete, -2 that the logs need
 * another plan and -3 that moves with a None newAddress/newFile still need their
 * prefix fix-up: smx_compose_finish (one stream synchronisation) then completes
 * them.  smx_compose_finish on complete results only checks them. */
int smx_compose_async(const smx_ops* ops, const smx_compose_out* out, void* workspace,
                      size_t workspace_bytes, void* stream);
int smx_compose_finish(const smx_ops* ops, const smx_compose_out* out, void* workspace,
                       size_t workspace_bytes, void* stream);

/* Kept for callers of rounds 3-5 (which cached merge graphs per stream): the library
 * caches none now; returns SMX_OK. */
int smx_release_graphs(void* stream);

/* The order plan the last composition on this thread ran (bench reporting). */
#define SMX_PLAN_PRESORTED 0 /* timestamp-ordered logs: presorted windows */
#define SMX_PLAN_SEGMENTED 1 /* ordered logs with long equal-timestamp groups */
#define SMX_PLAN_RADIX 2     /* unordered logs: radix sort on (ts, oid_hi) */
#define SMX_PLAN_RADIX_LO 3  /* ... and oid_lo (duplicate (ts, oid_hi) pairs) */
#define SMX_PLAN_PRESORTED_WIDE 4 /* ordered logs, groups up to 8192 ops: wide presorted windows */
#define SMX_PLAN_SMALL 5     /* merges of at most 2048 ops (any order): one workgroup, one launch */
int smx_last_plan(void);

/* Merges of at most n ops (clamped to 0..2048; default 2048) run as SMX_PLAN_SMALL, one
 * workgroup and one launch; 0 sends every merge through the window plans.  Process-wide;
 * returns the previous limit. */
int64_t smx_set_small_limit(int64_t n);

/*
 * Batched compose: n_merges independent merges of at most 2048 ops each in one call (a
 * merge queue, a rebase, a monorepo merged package by package).  The merges' columns lie
 * one after another in shared arrays; a device pre-pass sorts the merges into size classes
 * (256, 1024, 2048 ops) and one launch per class spreads them over the chip, several
 * workgroups per CU for the small classes.  The call only enqueues on `stream`: no host
 * synchronisation, no allocation, no read-back (read counts after synchronising).
 *
 * Per merge m the results equal smx_compose on that merge alone: counts[2m] composed ops
 * in order/addr/file/ctx at off[m].., order[] local to the merge (0 .. len-1, A first);
 * counts[2m+1] the full number of conflicts, of which the first
 * conf_off[m+1] - conf_off[m] pairs are written at conflicts[2 * conf_off[m]] and nothing at
 * or past the merge's conflict region.  String and symbol ids are opaque and local to a
 * merge (every merge's symbols are < n_sym <= 2^32 - 1).
 *
 * Checked on the device, per merge, before any of its columns is read:
 *   counts[2m] = counts[2m+1] = -1  off[m] < 0, off[m+1] < off[m] or > n_total, n_a[m]
 *                                   outside [0, len], conf_off decreasing or negative; or
 *                                   an op with kind >= 18 or sym >= n_sym
 *   counts[2m] = counts[2m+1] = -2  len > 2048: send that merge through smx_compose
 * A failed merge writes nothing else and does not affect its neighbours.
 */
typedef struct smx_batch {
  int64_t n_merges, n_total, n_sym;      /* n_sym: bound for every merge's symbol ids */
  const int64_t* off;                    /* device [n_merges+1]: merge m's ops are
                                            [off[m], off[m+1]) of the columns, A first */
  const int64_t* n_a;                    /* device [n_merges] */
  const uint8_t* kind; const uint64_t* ts, *oid_hi, *oid_lo;
  const uint32_t* sym; const int32_t* v0, *v1;     /* as smx_ops, n_total entries */
  int32_t* order, *addr, *file, *ctx;    /* n_total entries; merge m's results at off[m]..,
                                            order[] local to the merge (0 .. len-1) */
  int32_t* conflicts; const int64_t* conf_off;  /* device [n_merges+1], in pairs: merge m's
                                            capacity is conf_off[m+1]-conf_off[m] */
  int64_t* counts;                       /* [2*n_merges]: composed ops, conflicts */
  int32_t grid_cap;                      /* 0: library's choice; >0: at most this many
                                            workgroups per class (tuning, tests) */
} smx_batch;
/* Workspace for a batch of n_merges (0 .. 2^31 - 1) merges. */
int smx_compose_batch_workspace_bytes(int64_t n_merges, size_t* bytes);
/* SMX_E_ARG (negative sizes, grid_cap < 0, n_sym > 2^32 - 1, a null pointer with
 * n_merges > 0 -- the column and result arrays may be null only when n_total = 0) and
 * SMX_E_WORKSPACE are reported before any HIP call; n_merges = 0 returns SMX_OK and
 * launches nothing. */
int smx_compose_batch(const smx_batch* b, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Batched compose against one shared log: n_merges merges that all have the same log on one
 * side (a merge queue composing every pull request's delta against the target branch's, a
 * rebase composing every commit of a stack against the upstream delta).  The shared log is
 * stored once, as ops [0, n_shared) of the columns; merge m's own ops are [off[m], off[m+1]).
 * Merge m composes (shared, own_m) when shared_is_b = 0 and (own_m, shared) when it is 1, and
 * its results are exactly those of smx_compose on that pair alone:
 *   order[]    local to the merge: A's ops are 0 .. n_a-1 and B's follow (with shared_is_b = 0
 *              the shared ops are 0 .. n_shared-1, with 1 they are len_m .. len_m+n_shared-1)
 *   results    counts[2m] entries of order/addr/file/ctx starting at
 *              r(m) = off[m] + (m - 1) * n_shared: every merge has room for n_shared + len_m
 *              entries, in input order; the result arrays hold
 *              n_out = n_total - n_shared + n_merges * n_shared entries
 *   conflicts  conf_off, counts[2m+1] and truncation exactly as in smx_batch; pairs are
 *              (A index, B index), local to the merge
 * String and symbol ids form one domain for the whole batch (the shared log is stored once):
 * n_sym bounds all of them.  The size classes, the launches and the stream-ordered contract
 * (no host synchronisation, no allocation, no read-back) are those of smx_compose_batch.
 *
 * Checked on the device, per merge, before any of its own columns is read:
 *   counts[2m] = counts[2m+1] = -1  off[m] < n_shared, off[m+1] < off[m] or > n_total,
 *                                   conf_off decreasing or negative; or an op of the merge
 *                                   with kind >= 18 or sym >= n_sym -- an op of the shared
 *                                   log included: every merge then reports -1
 *   counts[2m] = counts[2m+1] = -2  n_shared + len_m > 2048: send that merge through
 *                                   smx_compose
 * A failed merge writes nothing else and does not affect its neighbours.
 */
typedef struct smx_batch_shared {
  int64_t n_merges, n_total, n_sym;
  int64_t n_shared;                      /* ops [0, n_shared) of every column: the shared log */
  const int64_t* off;                    /* device [n_merges+1], off[0] >= n_shared: merge m's
                                            own ops are [off[m], off[m+1]) of the columns */
  const uint8_t* kind; const uint64_t* ts, *oid_hi, *oid_lo;
  const uint32_t* sym; const int32_t* v0, *v1;     /* as smx_ops, n_total entries */
  int32_t* order, *addr, *file, *ctx;    /* n_out entries; merge m's results at r(m).. */
  int32_t* conflicts; const int64_t* conf_off;  /* as smx_batch */
  int64_t* counts;                       /* [2*n_merges]: composed ops, conflicts */
  int32_t grid_cap;                      /* as smx_batch */
  int32_t shared_is_b;                   /* 0: the shared log is branch A of every merge;
                                            1: branch B */
} smx_batch_shared;
/* Workspace for a batch of n_merges (0 .. 2^31 - 1) merges. */
int smx_compose_batch_shared_workspace_bytes(int64_t n_merges, size_t* bytes);
/* SMX_E_ARG (negative sizes, n_shared > n_total, grid_cap < 0, shared_is_b not 0 or 1,
 * n_sym > 2^32 - 1, a null pointer with n_merges > 0 -- the column and result arrays may be
 * null only when n_total = 0) and SMX_E_WORKSPACE are reported before any HIP call;
 * n_merges = 0 returns SMX_OK and launches nothing. */
int smx_compose_batch_shared(const smx_batch_shared* b, void* workspace, size_t workspace_bytes, void* stream);

/*
 * smx_compose_batch and smx_compose_batch_shared with flags.  flags = 0 is the unflagged call
 * bit for bit -- the same launches, workspace size and results, counts -2 included:
 * smx_compose_batch(...) == smx_compose_batch_ex(..., 0, stream), and
 * smx_compose_batch_workspace_bytes(n, bytes) == smx_compose_batch_ex_workspace_bytes(n, any, 0,
 * bytes); the shared forms alike.  A flag bit that is not defined here gives SMX_E_ARG before
 * any HIP call (and before any other check).
 *
 * SMX_BATCH_LARGE lifts the limit of 2048 ops per merge: counts -2 is never reported, and a
 * merge of any length (the shared form counts n_shared + len_m) gets exactly what smx_compose
 * gives on that merge alone -- counts[2m], order/addr/file/ctx, counts[2m+1] and the conflict
 * pairs, in the same order and at the same places of the struct.  Everything else is the
 * unflagged contract: the -1 rules (bounds checked before any column of the merge is read; a
 * kind >= 18 or sym >= n_sym anywhere in the merge found before anything is written for it),
 * truncation by conf_off, nothing written at or past a merge's regions, failed merges that do
 * not touch their neighbours, grid_cap (which also caps the added launch), shared_is_b.
 *
 * How: a merge over 2048 ops is one 1024-thread workgroup's work, through global memory: its op
 * indices sorted in tiles of 2048 (in LDS) and merge levels between two index arrays, the
 * DivergentRename walk in rounds of up to 1024 renames per side from the two heads (as
 * SMX_SCREEN_LARGE), the chains in an exact open-addressing table on the 32-bit symbol, emit.
 * Merges of at most 2048 ops run in the three size classes as before, in the same call.
 *
 * Stream-ordered as smx_compose_batch: five launches with SMX_BATCH_LARGE (four with flags = 0)
 * whatever the data, no host synchronisation, no allocation, no read-back; the call clears the
 * workspace state it needs, so one workspace serves any sequence of calls with either flags.
 *
 * Limits with SMX_BATCH_LARGE: n_total <= 2^31 - 1, and for the shared form the result size
 * n_out = n_total - n_shared + n_merges * n_shared too (SMX_E_ARG above it).  One workgroup
 * runs a large merge, so one merge of millions of ops is served slowly (smx_compose spreads it
 * over the chip); many merges spread over the chip.
 */
#define SMX_BATCH_LARGE 1u
/* Workspace for the _ex calls with the same flags (8-byte aligned with SMX_BATCH_LARGE).  With
 * SMX_BATCH_LARGE it is linear in the result size: the unflagged bytes, 4 bytes per merge, and
 * 64 bytes per op of n_total (shared: per entry of n_out); a large merge works in the slice at
 * its own result offset, so there are no per-workgroup slots and no cap on a merge's length. */
int smx_compose_batch_ex_workspace_bytes(int64_t n_merges, int64_t n_total, uint32_t flags, size_t* bytes);
int smx_compose_batch_shared_ex_workspace_bytes(int64_t n_merges, int64_t n_total, int64_t n_shared, uint32_t flags,
                                                size_t* bytes);
/* SMX_E_ARG (an unknown flag; then the unflagged calls'; with SMX_BATCH_LARGE n_total or n_out
 * over 2^31 - 1) and SMX_E_WORKSPACE (too small for these flags, or with SMX_BATCH_LARGE not
 * 8-byte aligned) are reported before any HIP call; n_merges = 0 returns SMX_OK and launches
 * nothing. */
int smx_compose_batch_ex(const smx_batch* b, void* workspace, size_t workspace_bytes, uint32_t flags, void* stream);
int smx_compose_batch_shared_ex(const smx_batch_shared* b, void* workspace, size_t workspace_bytes, uint32_t flags,
                                void* stream);

/*
 * Conflict screen: which of n_pairs pairs of logs, taken from n_logs logs stored once, have
 * DivergentRename conflicts, and which ones -- without composing any pair (a merge queue asking
 * which pull requests conflict with the target branch, or with each other).  The conflict
 * list of smx_compose on two logs is a function of the two logs' renames alone: each log's
 * renames in (ts, oid_hi, oid_lo, index) order, merged A first on equal keys, and the
 * reference's two-head walk over them (compose.py:16-21, 60-70, 88-98).  So each log's
 * renames are extracted and sorted once, however many pairs hold the log, and a pair costs
 * one merge and one walk of two short lists.  The limits are on renames, not on ops.
 *
 * Log l's ops are [log_off[l], log_off[l+1]) of the columns (entries that no log of a pair
 * covers are never read).  Pair p screens (log pair_a[p] as A, log pair_b[p] as B);
 * pair_a[p] == pair_b[p] is an ordinary pair.  For every valid pair, counts[p] and the written
 * conflict pairs equal counts[1] and conflicts of smx_compose on that pair alone, in the same
 * order: (A index, B index) into A||B, the A index in [0, len_a), the B index len_a + j.
 * counts[p] is the full number of conflicts; the first conf_off[p+1] - conf_off[p] pairs are
 * written at conflicts[2 * conf_off[p]] and nothing at or past the pair's region.  conflicts
 * and conf_off both NULL: capacity 0 for every pair (counts only).
 *
 * kind is read for every op of a log that a call holds; ts, oid_hi, oid_lo, sym and v0 are
 * read for renames only.  sym is only compared for equality, so it has no bound (there is
 * no n_sym), and there is no v1.
 *
 * Checked on the device:
 *   counts[p] = -1  pair_a[p] or pair_b[p] outside [0, n_logs); conf_off[p] negative or
 *                   conf_off[p+1] < conf_off[p]; or either log is invalid: log_off[l] < 0 or
 *                   below an earlier offset (log_off decreases: the log that ends early and
 *                   every log that starts before an earlier offset), log_off[l+1] < log_off[l]
 *                   or > n_total, or an op with kind >= 18
 *   counts[p] = -2  a log of the pair has more than 2048 renames, or the pair's renames
 *                   together exceed 2048: send that pair through smx_compose
 * A failed pair writes nothing else and does not affect its neighbours.
 *
 * Stream-ordered as smx_compose_batch: six launches whatever the data, no host
 * synchronisation, no allocation, no read-back.  A device pre-pass sorts the pairs into
 * size classes by their renames (128, 512, 2048) and one launch per class runs them.  One
 * workgroup extracts a log's renames, so a log of many millions of ops is served slowly.
 *
 * The struct and the function share their name, so C callers write `struct smx_screen`.
 */
struct smx_screen {
  int64_t n_logs, n_total, n_pairs;
  const int64_t* log_off;          /* device [n_logs+1]: log l's ops are [log_off[l], log_off[l+1]) */
  const uint8_t* kind; const uint64_t* ts, *oid_hi, *oid_lo;
  const uint32_t* sym; const int32_t* v0;          /* as smx_ops, n_total entries; no v1 */
  const int32_t* pair_a, *pair_b;  /* device [n_pairs]: pair p screens (log pair_a[p], log pair_b[p]) */
  int32_t* conflicts; const int64_t* conf_off;     /* as smx_batch, per pair; both NULL: capacity 0 everywhere */
  int64_t* counts;                 /* device [n_pairs] */
  int32_t grid_cap;                /* as smx_batch; also caps the per-log launch */
};
/* Workspace (8-byte aligned) for n_logs and n_pairs in 0 .. 2^31 - 1: about 36 bytes per op. */
int smx_screen_workspace_bytes(int64_t n_logs, int64_t n_total, int64_t n_pairs, size_t* bytes);
/* SMX_E_ARG (negative sizes, grid_cap < 0, exactly one of conflicts / conf_off null, a null
 * log_off / pair_a / pair_b / counts, a null column with n_total > 0) and SMX_E_WORKSPACE are
 * reported before any HIP call; n_pairs = 0 or n_logs = 0 returns SMX_OK and launches nothing. */
int smx_screen(const struct smx_screen* s, void* workspace, size_t workspace_bytes, void* stream);

/*
 * smx_screen with flags.  flags = 0 is smx_screen bit for bit -- the same launches, workspace
 * size and results, counts -2 included: smx_screen(...) == smx_screen_ex(..., 0, stream), and
 * smx_screen_workspace_bytes(...) == smx_screen_ex_workspace_bytes(..., 0, bytes).  A flag bit
 * that is not defined here gives SMX_E_ARG before any HIP call (and before any other check).
 *
 * SMX_SCREEN_LARGE lifts the limit of 2048 renames: counts[p] = -2 is never reported, and a
 * pair of any number of renames gets exactly what smx_compose reports for it -- counts[p] and
 * the conflict pairs of smx_screen's contract above, in the same order.  Everything else is
 * smx_screen's: the struct, the -1 rules (a kind >= 18 anywhere in a log, also past its 2048th
 * rename, fails every pair that holds the log), truncation per pair (the full count in
 * counts[p], the first conf_off[p+1] - conf_off[p] pairs written, nothing at or past the
 * region), the counts-only form with conflicts = conf_off = NULL, self pairs, a pair with a
 * side without renames (counts 0), grid_cap (which also caps the two added launches).
 *
 * How: a log over 2048 renames is sorted by one workgroup in tiles of 2048 (in LDS) and merge
 * levels over two index arrays in the workspace; a pair whose renames together exceed 2048 is
 * walked by one workgroup in rounds of up to 1024 sorted renames per side, each round starting
 * at the pair of heads where the round before used up one side's 1024, so at most
 * ceil(renames of A / 1024) + ceil(renames of B / 1024) rounds.  Pairs of at most 2048 renames
 * run in smx_screen's three size classes as before, in the same call.
 *
 * Stream-ordered as smx_screen: eight launches with SMX_SCREEN_LARGE (six with flags = 0)
 * whatever the data, no host synchronisation, no allocation, no read-back; the call clears the
 * workspace state it needs, so one workspace serves any sequence of calls with either flags.
 *
 * Limits with SMX_SCREEN_LARGE: n_total <= 2^31 - 1 (SMX_E_ARG above it), which bounds every
 * log's renames.  One workgroup sorts a large log and one workgroup walks a large pair, so one
 * pair of two logs of millions of renames is served slowly; many pairs spread over the chip.
 */
#define SMX_SCREEN_LARGE 1u
/* Workspace (8-byte aligned) for smx_screen_ex with the same flags.  With SMX_SCREEN_LARGE:
 * smx_screen's and 8 bytes per op and 4 bytes per pair more (about 44 bytes per op). */
int smx_screen_ex_workspace_bytes(int64_t n_logs, int64_t n_total, int64_t n_pairs, uint32_t flags, size_t* bytes);
/* SMX_E_ARG (an unknown flag; then smx_screen's: negative sizes, grid_cap < 0, exactly one of
 * conflicts / conf_off null, a null log_off / pair_a / pair_b / counts, a null column with
 * n_total > 0; with SMX_SCREEN_LARGE n_total > 2^31 - 1) and SMX_E_WORKSPACE (too small for
 * these flags or not 8-byte aligned) are reported before any HIP call; n_pairs = 0 or
 * n_logs = 0 returns SMX_OK and launches nothing. */
int smx_screen_ex(const struct smx_screen* s, void* workspace, size_t workspace_bytes, uint32_t flags, void* stream);

/*
 * Candidate pairs for the screen: which pairs (i, j), i < j, of n_logs logs stored once can
 * have DivergentRename conflicts at all -- so that "which of these N pull requests conflict
 * with each other" does not start from all N (N - 1) / 2 pairs.  A DivergentRename needs a
 * rename in each log on the same symbolId with different newName (compose.py:60-70, 88-98):
 * in the columns, the same sym with a different v0.  That is a necessary condition, not the
 * answer: a candidate may turn out to have no conflict; a pair of valid logs that is not a
 * candidate has none, in either orientation -- smx_compose, and so smx_screen, reports zero
 * conflicts for (i, j) and for (j, i).
 *
 * Log l's ops are [log_off[l], log_off[l+1]) of the columns, and a log is valid under exactly
 * smx_screen's rules: log_off[l] is not negative and not below any earlier offset,
 * log_off[l+1] is not below log_off[l] and not above n_total, and no op of the log has
 * kind >= 18.  Entries that no log covers are never read.  Only kind, sym and v0 are read (sym
 * and v0 for renames only); ts, the ids and v1 are not part of the call.  sym has no bound and
 * is only compared for equality; v0 is compared as a 32-bit pattern, as smx_screen does.
 *
 * Pair (i, j) with i < j is a candidate when both logs are valid and some symbol s has a
 * rename in log i and a rename in log j whose v0 differ.  Self pairs (i, i) are not produced
 * (a log can conflict with itself; screen (i, i) directly if that is asked).  A log takes
 * part whatever its number of renames: the 2048-rename limit belongs to the later smx_screen.
 *
 *   pair_a, pair_b  the candidates in ascending (i, j) order, lexicographic and deterministic,
 *                   each pair once however many symbols produce it: the first pair_cap of them
 *                   are written and nothing at or past pair_cap.  pair_cap = 0 with both
 *                   arrays NULL asks for the count alone.
 *   counts[0]       the full number of candidates, whatever pair_cap is
 *   counts[1]       the number of invalid logs; an invalid log appears in no pair and does not
 *                   affect its neighbours
 *   log_info        (or NULL) every log's entry is written: -1 for an invalid log, else its
 *                   number of renames
 *
 * Stream-ordered as smx_screen: the call only enqueues -- no host synchronisation, no
 * allocation, no read-back -- and the number of launches depends on n_logs alone (through the
 * width of the sort key), never on the data.  It clears the workspace state it needs itself,
 * so one workspace serves any sequence of calls.  Cost beyond the sort of the renames: a symbol
 * renamed in g logs sets g (g - 1) / 2 bits of an n_logs x n_logs bit matrix, and one
 * workgroup walks a log's kind bytes.
 *
 * To chain into smx_screen with no synchronisation at all: pre-fill pair_a / pair_b with -1,
 * then call smx_screen on the same columns with these arrays as its pair_a / pair_b,
 * n_pairs = pair_cap and conflicts = conf_off = NULL.  The entries past counts[0] still hold
 * -1 and report counts -1 by smx_screen's rule for a pair index outside [0, n_logs).
 */
#define SMX_CAND_MAX_LOGS 16384
struct smx_candidates {
  int64_t n_logs, n_total;
  const int64_t* log_off;                 /* device [n_logs+1], as smx_screen */
  const uint8_t* kind; const uint32_t* sym; const int32_t* v0;   /* n_total entries; ts, ids, v1 are not read */
  int32_t* pair_a, *pair_b;               /* device [pair_cap], out; both NULL only with pair_cap = 0 */
  int64_t pair_cap;
  int64_t* counts;                        /* device [2]: candidates (full number), invalid logs */
  int32_t* log_info;                      /* device [n_logs] or NULL: -1 invalid log, else its number of renames */
  int32_t grid_cap;                       /* as smx_batch: caps the call's own per-log, per-entry and matrix launches */
};
/* Workspace (8-byte aligned) for n_logs in 0 .. SMX_CAND_MAX_LOGS and n_total in 0 .. 2^31 - 1:
 * about 48 bytes per op and 3 * n_logs^2 / 8 bytes (96 MB at the limit). */
int smx_screen_candidates_workspace_bytes(int64_t n_logs, int64_t n_total, size_t* bytes);
/* SMX_E_ARG (negative sizes, n_logs > SMX_CAND_MAX_LOGS, n_total > 2^31 - 1, pair_cap < 0,
 * grid_cap < 0, a null log_off or counts, a null column with n_total > 0, a null pair array
 * with pair_cap > 0) and SMX_E_WORKSPACE (too small or not 8-byte aligned) are reported before
 * any HIP call; n_logs = 0 returns SMX_OK and launches nothing (counts is not written). */
int smx_screen_candidates(const struct smx_candidates* c, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Batched compose of pairs of logs stored once: n_pairs merges over n_logs logs, laid out as
 * smx_screen takes them (log_off, pair_a, pair_b), so that the pairs a screen left clean, M
 * pull requests against K release branches or every pair of a merge train are composed without
 * repeating a log once per pair that holds it.  Pair p composes (log pair_a[p] as A, log
 * pair_b[p] as B).  Self pairs (i, i), (i, j) together with (j, i), the same pair listed twice
 * and a log b stored before log a are all ordinary pairs.  Symbol and string ids form one
 * domain for all the logs; n_sym bounds all the symbols.
 *
 * For every valid pair the results are exactly those of smx_compose on (log a, log b) alone:
 *   results    counts[2p] entries of order/addr/file/ctx starting at res_off[p]; the pair's
 *              region [res_off[p], res_off[p+1]) has room for len_a + len_b entries at least
 *   order[]    local to the pair: A's ops are 0 .. len_a-1, B's are len_a + j (smx_screen's
 *              indices)
 *   conflicts  conf_off, counts[2p+1] and truncation exactly as in smx_batch: the full number
 *              in counts[2p+1], the first conf_off[p+1] - conf_off[p] pairs written at
 *              conflicts[2 * conf_off[p]], nothing at or past the pair's regions
 *
 * Checked on the device, per pair, before any column of the pair is read:
 *   counts[2p] = counts[2p+1] = -1  pair_a[p] or pair_b[p] outside [0, n_logs); either log
 *                                   invalid under smx_screen's log_off rules (log_off[l] < 0 or
 *                                   below an earlier offset, log_off[l+1] < log_off[l] or
 *                                   > n_total); res_off[p] < 0 or below an earlier res_off entry
 *                                   (the same rule: valid pairs' regions never overlap),
 *                                   res_off[p+1] - res_off[p] < len_a + len_b, res_off[p+1] >
 *                                   n_out; conf_off negative or decreasing; or an op with
 *                                   kind >= 18 or sym >= n_sym in either log, which fails
 *                                   every pair that holds the log, and only those
 *   counts[2p] = counts[2p+1] = -2  len_a + len_b > 2048 without SMX_BATCH_LARGE: send that
 *                                   pair through smx_compose
 * A failed pair writes nothing else and does not affect its neighbours.
 *
 * flags is 0 or SMX_BATCH_LARGE; any other bit gives SMX_E_ARG before every other check.  With
 * SMX_BATCH_LARGE counts -2 is never reported: a pair over 2048 ops is one 1024-thread
 * workgroup's work through global memory, as in smx_compose_batch_ex, in the workspace slice
 * at res_off[p].
 *
 * Stream-ordered as smx_compose_batch: five launches with flags = 0, six with SMX_BATCH_LARGE,
 * whatever the data; no host synchronisation, no allocation, no read-back; the call clears the
 * workspace state it needs, so one workspace serves any sequence of calls with either flags.
 * A device pre-pass checks the log and result offsets (a running maximum each) and sorts the
 * pairs into smx_compose_batch's size classes.  Each pair sorts its two logs again: a log held
 * by k pairs is loaded and ordered k times (only the copy to the device and its columns are
 * shared).
 */
typedef struct smx_pairs {
  int64_t n_logs, n_total, n_pairs, n_sym, n_out;
  const int64_t* log_off;                 /* device [n_logs+1], as smx_screen */
  const uint8_t* kind; const uint64_t* ts, *oid_hi, *oid_lo;
  const uint32_t* sym; const int32_t* v0, *v1;     /* as smx_ops, n_total entries, one id domain for all logs */
  const int32_t* pair_a, *pair_b;         /* device [n_pairs]: pair p composes (log pair_a[p] as A, log pair_b[p] as B) */
  const int64_t* res_off;                 /* device [n_pairs+1]: pair p's results at [res_off[p], res_off[p+1]) of
                                             the result arrays */
  int32_t* order, *addr, *file, *ctx;     /* n_out entries */
  int32_t* conflicts; const int64_t* conf_off;     /* as smx_batch, per pair */
  int64_t* counts;                        /* [2*n_pairs]: composed ops, conflicts */
  int32_t grid_cap;                       /* as smx_batch */
} smx_pairs;
/* Workspace (8-byte aligned) for n_logs and n_pairs in 0 .. 2^31 - 1 and these flags: 4 bytes
 * per log and 16 per pair; with SMX_BATCH_LARGE 4 bytes per pair and 64 per entry of n_out
 * more (n_out <= 2^31 - 1; without the flag n_out only has to be >= 0). */
int smx_compose_pairs_workspace_bytes(int64_t n_logs, int64_t n_pairs, int64_t n_out, uint32_t flags, size_t* bytes);
/* SMX_E_ARG (an unknown flag; then a null struct, negative sizes, n_logs or n_pairs over
 * 2^31 - 1, grid_cap < 0, n_sym > 2^32 - 1; with SMX_BATCH_LARGE n_total or n_out over
 * 2^31 - 1; a null log_off / pair_a / pair_b / res_off / conflicts / conf_off / counts, a null
 * column with n_total > 0, a null result array with n_out > 0) and SMX_E_WORKSPACE (too small
 * for these flags, or not 8-byte aligned) are reported before any HIP call; n_pairs = 0 or
 * n_logs = 0 returns SMX_OK and launches nothing. */
int smx_compose_pairs(const struct smx_pairs* p, void* workspace, size_t workspace_bytes, uint32_t flags, void* stream);

/*
 * Merge trains over logs stored once: each log composed against what landed before it
 * (DESIGN.md §21).  The logs are laid out as smx_screen / smx_pairs take them.  Train r is the
 * logs train_log[train_off[r] .. train_off[r+1]), in that order; step g = train_off[r] + s is
 * its s-th log.  A log may be in any number of trains, and more than once in one.
 *
 * The accumulator of a train starts empty.  Step g composes (accumulator as A, log as B)
 * exactly as smx_compose would on those two logs.  With zero conflicts the step lands: the
 * accumulator becomes the composed log -- the columns that marshalling the composed ops would
 * give: the source ops' columns in composed order, a move's v0 replaced by the step's addr[k]
 * where that is not SMX_NONE and its v1 by file[k] alike -- except where file[k] is empty_str,
 * the id of the empty string: marshalling reads a move's file as `newFile or file`, so an empty
 * newFile falls through to the op's own `file`, and v1 becomes v1_alt[src] (the id of
 * str(params["file"]), or SMX_NONE without one).  With empty_str = SMX_NONE (no empty string
 * among the ids) v1_alt is not read and may be NULL.  Any other step (conflicts, -1, -2
 * below) leaves the accumulator as it was, and the train goes on with its next log.
 *
 * Every accumulator entry carries its source column index (log_off[l] + i: it names log and
 * op) and its accumulated addr / file / ctx: per field the last value that was not SMX_NONE
 * over the steps it went through.  Applied to a clone of the source op they give the op that
 * materialising step after step gives.
 *
 *   results      per train r, counts[2r] entries of src / addr / file / ctx from res_off[r]: the
 *                final accumulator; the region [res_off[r], res_off[r+1]) has room for the sum
 *                of the lengths of the train's logs at least; counts[2r+1]: the steps that landed
 *   step_counts  [2g]: the accumulator's length after step g, whatever happened;
 *                [2g+1]: >= 0 the step's conflicts (0: it landed);
 *                        -1 a log index outside [0, n_logs), a log invalid under smx_screen's
 *                           log_off rules, or an op with kind >= 18 or sym >= n_sym in it;
 *                        -2 accumulator plus log exceed 2048 ops
 *   conflicts    per step g the first conf_off[g+1] - conf_off[g] records at conflicts[4 *
 *                conf_off[g]], the full number in step_counts[2g+1], nothing past the capacity
 *                (a negative or decreasing conf_off gives the step none).  A record is four
 *                int32: the A op's column index, the B op's column index, and the addr and the
 *                file the A op carried when the step began.
 *
 * A train whose train_off or res_off entries are negative, below an earlier entry, decreasing
 * or past n_steps / n_out, or whose region is too small, reports counts -1, -1 and writes
 * nothing else.  Failed trains and steps never touch their neighbours.
 *
 * Stream-ordered as smx_compose_batch: five launches whatever the data, no host
 * synchronisation, no allocation, no read-back; the call clears the workspace state it needs,
 * so one workspace serves any sequence of calls.  One workgroup runs a train's steps one after
 * another.  flags must be 0.
 */
typedef struct smx_train {
  int64_t n_logs, n_total, n_trains, n_steps, n_sym, n_out;
  const int64_t* log_off;                 /* device [n_logs+1], as smx_screen */
  const uint8_t* kind; const uint64_t* ts, *oid_hi, *oid_lo;
  const uint32_t* sym; const int32_t* v0, *v1;     /* as smx_ops, n_total entries, one id domain for all logs */
  const int32_t* v1_alt;                  /* n_total entries, read for moves only: see above; NULL with empty_str < 0 */
  const int64_t* train_off;               /* device [n_trains+1], into train_log */
  const int32_t* train_log;               /* device [n_steps]: log indices */
  const int64_t* res_off;                 /* device [n_trains+1]: train r's results at [res_off[r], res_off[r+1]) */
  int32_t* src, *addr, *file, *ctx;       /* n_out entries */
  int32_t* conflicts; const int64_t* conf_off;     /* 4 int32 per record; conf_off [n_steps+1], in records */
  int64_t* counts;                        /* [2*n_trains]: final accumulator length, landed steps */
  int64_t* step_counts;                   /* [2*n_steps]: accumulator length after the step, its outcome */
  int32_t grid_cap;                       /* as smx_batch */
  int32_t empty_str;                      /* the id of the empty string in the v1 / file domain, or SMX_NONE */
} smx_train;
/* Workspace (8-byte aligned), linear in its arguments: 4 bytes per log, 36 per train and 89 per
 * entry of n_out (n_logs, n_trains, n_steps, n_out in 0 .. 2^31 - 1; flags 0). */
int smx_compose_train_workspace_bytes(int64_t n_logs, int64_t n_trains, int64_t n_steps, int64_t n_out,
                                      uint32_t flags, size_t* bytes);
/* SMX_E_ARG (a non-zero flag; then a null struct, negative sizes, n_logs, n_trains, n_steps,
 * n_total or n_out over 2^31 - 1, grid_cap < 0, empty_str < -1, n_sym > 2^32 - 1; a null v1_alt
 * with empty_str >= 0 and n_total > 0; a null train_off / res_off /
 * counts, a null log_off with n_logs > 0, a null train_log / conf_off / step_counts /
 * conflicts with n_steps > 0, a null column with n_total > 0, a null result array with
 * n_out > 0) and SMX_E_WORKSPACE (too small, or not 8-byte aligned) are reported before any HIP
 * call; n_trains = 0 returns SMX_OK and launches nothing. */
int smx_compose_train(const struct smx_train* t, void* workspace, size_t workspace_bytes, uint32_t flags,
                      void* stream);

/*
 * Merge trains that share prefixes, composed once.  A speculative merge queue
 * wants the state after pull request 1, after 1+2, ... and the fallbacks that drop a member; a
 * rebase wants the composed log after every commit of a stack.  Those trains form a tree, and a
 * root-to-node path of the tree is a train of smx_compose_train.  Here every node is composed
 * once, its accumulator is a result, and it is where all its children start.  The logs are laid
 * out as smx_train takes them.
 *
 * The n_nodes nodes are stored level by level: level d is the nodes [level_off[d],
 * level_off[d+1]).  node_parent[n] is SMX_NONE for a node of level 0 and a node of level d-1 for
 * a node of level d; node_log[n] is its log.  A log may be in any number of nodes, and more than
 * once on a path.
 *
 * Node n composes (the accumulator of its parent as A, log node_log[n] as B) exactly as step g
 * of smx_compose_train does: the same staging rule (v1_alt, empty_str), the same landing rule,
 * the same records.  A node of level 0 starts from the empty accumulator.  With zero conflicts
 * the node lands, and its accumulator, the composed log, is written as src / addr / file / ctx
 * entries into its own region [res_off[n], res_off[n+1]).  Any other outcome (conflicts, -1,
 * -2 below) leaves the node's accumulator as its parent's, and nothing is copied.
 *
 *   node_acc     [n]: the node whose region holds n's accumulator: n itself if it landed, else
 *                node_acc[parent]; SMX_NONE if no node of its root path landed (the accumulator
 *                is empty)
 *   node_counts  [2n]: the accumulator's length after the node, whatever happened;
 *                [2n+1]: >= 0 the node's conflicts (0: it landed);
 *                        -1 a log index outside [0, n_logs), a log invalid under smx_screen's
 *                           log_off rules, or an op with kind >= 18 or sym >= n_sym in it;
 *                        -2 accumulator plus log exceed 2048 ops
 *   conflicts    per node n the first conf_off[n+1] - conf_off[n] records at conflicts[4 *
 *                conf_off[n]], the full number in node_counts[2n+1], nothing at or past the
 *                capacity (a negative or decreasing conf_off gives the node none).  A record is
 *                smx_train's: the A op's column index, the B op's column index, and the addr and
 *                the file the A op carried in the parent's accumulator.
 *
 * So for every valid node n, node_counts[2n], node_counts[2n+1], its records and the accumulator
 * reached through node_acc[n] equal what smx_compose_train reports for the last step and the
 * final accumulator of the train that is n's root path.
 *
 * A node fails structurally -- node_counts[2n] = node_counts[2n+1] = -1, node_acc[n] = SMX_NONE,
 * nothing else written -- when
 *   - it lies in no valid level.  Level d is valid when level_off[d] is not negative and not
 *     below an earlier entry, level_off[d+1] is not below level_off[d] and not past n_nodes,
 *     level 0 starts at node 0 and the last level ends at n_nodes;
 *   - its parent is not in the level before (no node is in an invalid level), or it is of
 *     level 0 and has a parent;
 *   - its res_off entries are negative, below an earlier entry, decreasing or past n_out;
 *   - its region is smaller than min(2048, the sum of the valid logs' lengths on its root path);
 *   - its parent failed structurally.
 * All of this is checked on the device before any column of the node is read through an
 * unchecked index.  Failed nodes never touch their neighbours.
 *
 * Stream-ordered: a pre-pass, then per level one launch for each of the three size classes of
 * smx_compose_batch (256 / 1024 / 2048 ops, by min(path sum, 2048)): 1 + 3 * n_levels launches
 * whatever the data.  A level depends on the level before through stream order alone: no
 * workgroup waits for another one.  No host synchronisation, no allocation, no read-back; the
 * call clears the workspace state it needs, so one workspace serves any sequence of calls.
 * grid_cap caps every launch.  flags must be 0.
 */
#define SMX_TREE_MAX_LEVELS 4096
typedef struct smx_tree {
  int64_t n_logs, n_total, n_nodes, n_levels, n_sym, n_out;   /* n_levels: a host scalar */
  const int64_t* log_off;                 /* device [n_logs+1], as smx_screen */
  const uint8_t* kind; const uint64_t* ts, *oid_hi, *oid_lo;
  const uint32_t* sym; const int32_t* v0, *v1;     /* as smx_ops, n_total entries, one id domain for all logs */
  const int32_t* v1_alt;                  /* as smx_train */
  const int64_t* level_off;               /* device [n_levels+1], into the nodes */
  const int32_t* node_parent;             /* device [n_nodes]: a node of the level before, or SMX_NONE */
  const int32_t* node_log;                /* device [n_nodes]: log indices */
  const int64_t* res_off;                 /* device [n_nodes+1]: node n's accumulator at [res_off[n], res_off[n+1]) */
  int32_t* src, *addr, *file, *ctx;       /* n_out entries */
  int32_t* conflicts; const int64_t* conf_off;     /* 4 int32 per record; conf_off [n_nodes+1], in records */
  int64_t* node_counts;                   /* [2*n_nodes]: accumulator length after the node, its outcome */
  int32_t* node_acc;                      /* [n_nodes]: the node whose region holds the accumulator */
  int32_t grid_cap;                       /* as smx_batch */
  int32_t empty_str;                      /* as smx_train */
} smx_tree;
/* Workspace (8-byte aligned), linear in its arguments, each term rounded up to 256 bytes: 4
 * bytes per log, 20 per node (two verdicts and the three class lists), 20 per level (its class
 * counts and a verdict) and 57 per entry of n_out (37 of staged columns, 16 of a step's scratch
 * result, 4 of its conflict pairs); no state buffers: the accumulators live in the result
 * regions.  n_logs, n_nodes, n_out in 0 .. 2^31 - 1, n_levels in 0 .. SMX_TREE_MAX_LEVELS;
 * flags 0. */
int smx_compose_tree_workspace_bytes(int64_t n_logs, int64_t n_nodes, int64_t n_levels, int64_t n_out,
                                     uint32_t flags, size_t* bytes);
/* SMX_E_ARG (a non-zero flag; then a null struct, negative sizes, n_levels over
 * SMX_TREE_MAX_LEVELS, n_logs, n_nodes, n_total or n_out over 2^31 - 1, grid_cap < 0,
 * empty_str < -1, n_sym > 2^32 - 1; a null v1_alt with empty_str >= 0 and n_total > 0; a null
 * level_off / node_parent / node_log / res_off / conf_off / conflicts / node_counts / node_acc,
 * a null log_off with n_logs > 0, a null column with n_total > 0, a null result array with
 * n_out > 0) and SMX_E_WORKSPACE (too small, or not 8-byte aligned) are reported before any HIP
 * call; n_nodes = 0 returns SMX_OK and launches nothing. */
int smx_compose_tree(const struct smx_tree* t, void* workspace, size_t workspace_bytes, uint32_t flags,
                     void* stream);

/*
 * One step of a merge train of any size, as two calls on either side of smx_compose (DESIGN.md
 * §23).  smx_compose_train runs a train inside one workgroup and reports -2 for a step over
 * 2048 ops.  What leads from one compose to the next is a gather, and smx_compose composes a
 * merge of any size, so such a train is a host loop over columns that stay on the device:
 *
 *   smx_train_stage   the step's input columns, from the accumulator and the next log
 *   smx_compose       on the staged columns: an smx_ops with n_a = n_acc, n_b = log_n, b_gap = 0
 *   smx_train_land    the result folded into the accumulator, or its conflicts as records
 *
 * The struct describes one step of one train.  Every pointer is device memory that the caller
 * owns; there is no workspace and nothing is allocated.  The accumulator is what smx_train's is:
 * per entry the op's column index (src) and its accumulated addr / file / ctx.
 *
 * smx_train_stage writes staged entry e, for e in [0, n_acc + log_n), by the rule of
 * smx_compose_train's steps.  For e < n_acc: the columns of op acc_src[e]; a move's v0 is
 * acc_addr[e] where that is not SMX_NONE; a move's v1 is acc_file[e] where that is not SMX_NONE,
 * and v1_alt[acc_src[e]] where acc_file[e] == empty_str.  For e >= n_acc: the columns of op
 * log_lo + e - n_acc as they are.  It sets status[0]: 0 for a well-formed step; -1 when an op
 * of the step has kind >= 18 or sym >= n_sym, or an acc_src[e] lies outside [0, n_total).  Such
 * an acc_src[e] is not read through: the staged entry gets kind 0xFF and sym 0xFFFFFFFF, which
 * smx_compose refuses, and its other columns are left as they were.
 *
 * smx_train_land reads counts and status[0] on the device:
 *   counts[0] < 0 or status[0] != 0   status[1] = -1; nothing else is written
 *   counts[1] > 0   the step does not land: status[1] = counts[1], status[2] = n_acc, and the
 *                   first min(counts[1], conflict_cap, record_cap) records are written, nothing
 *                   at or past record_cap; the accumulator out is untouched.  A record is
 *                   smx_train's: the A op's column index, the B op's column index, and the addr
 *                   and the file the A op carried when the step began.
 *   counts[1] == 0  the step lands: status[1] = 0, status[2] = counts[0], and entry k of the
 *                   accumulator out, for k < counts[0], is the old entry order[k] -- or a fresh
 *                   one of the log, src = log_lo + order[k] - n_acc and SMX_NONE in the three
 *                   fields -- with the step's addr[k] / file[k] / ctx[k] folded in per field:
 *                   the step's value where it is not SMX_NONE, else the old one.
 * smx_train_land does not read the staged columns.  An element index in order or conflicts
 * that names no entry of the step is not read through (its entry or record is not written).
 *
 * Each call is one kernel launch on `stream` (smx_train_stage clears status[0] ahead of its
 * kernel, stream-ordered): no host synchronisation, no allocation, no read-back, so the three
 * calls of a step follow each other without waiting.  Both are valid with n_acc = 0 and with
 * log_n = 0; with n_acc + log_n = 0 they launch nothing, write nothing and return SMX_OK.
 */
typedef struct smx_train_step {
  /* the log store, as smx_train takes it */
  int64_t n_total, n_sym;
  const uint8_t* kind; const uint64_t* ts, *oid_hi, *oid_lo;
  const uint32_t* sym; const int32_t* v0, *v1;     /* as smx_ops, n_total entries */
  const int32_t* v1_alt;                  /* n_total entries, read for moves only; NULL with empty_str < 0 */
  /* the accumulator in */
  int64_t n_acc;
  const int32_t* acc_src, *acc_addr, *acc_file, *acc_ctx;   /* n_acc entries */
  /* the step's log: ops [log_lo, log_lo + log_n) of the columns */
  int64_t log_lo, log_n;
  /* the staged merge, written by smx_train_stage: capacity n_acc + log_n */
  uint8_t* st_kind; uint64_t* st_ts, *st_oid_hi, *st_oid_lo;
  uint32_t* st_sym; int32_t* st_v0, *st_v1;
  /* the compose result that smx_train_land reads: smx_compose_out's fields */
  const int32_t* order, *addr, *file, *ctx;
  const int32_t* conflicts; int64_t conflict_cap;
  const int64_t* counts;
  /* the accumulator out, written by smx_train_land: capacity n_acc + log_n, not the
   * accumulator in (the caller alternates between two sets) */
  int32_t* out_src, *out_addr, *out_file, *out_ctx;
  int32_t* records; int64_t record_cap;   /* 4 int32 per record */
  int64_t* status;                        /* device [3]: stage's verdict, the step's outcome, the
                                             accumulator's length after the step */
  int32_t empty_str;                      /* as smx_train */
} smx_train_step;
/* Both calls return SMX_E_ARG before any HIP call for: a null struct; a negative size, log_lo,
 * conflict_cap or record_cap; n_total or n_acc + log_n over 2^31 - 1; log_lo + log_n > n_total;
 * n_sym > 2^32 - 1; empty_str < -1; a null v1_alt with empty_str >= 0 and n_total > 0; and,
 * with n_acc + log_n > 0, a null pointer that the call would use.  smx_train_stage uses status,
 * the columns (n_total > 0), acc_src / acc_addr / acc_file (n_acc > 0) and the staged columns.
 * smx_train_land uses status, counts, order / addr / file / ctx, the accumulator out, the four
 * arrays of the accumulator in (n_acc > 0), conflicts (conflict_cap > 0) and records
 * (record_cap > 0); an array of the accumulator out that is one of the accumulator in is
 * SMX_E_ARG too. */
int smx_train_stage(const struct smx_train_step* s, void* stream);
int smx_train_land(const struct smx_train_step* s, void* stream);

/*
 * Conflict screen of merge trains: which steps of smx_compose_train's trains have
 * DivergentRename conflicts, and which ones, from the logs' renames alone.
 * The logs and the trains are laid out as smx_train takes them, the columns as smx_screen
 * takes them (no v1, no n_sym).  A pair's conflict list is a function of the two logs' renames
 * (smx_screen above), and a step that lands leaves every rename's timestamp, id, symbol and
 * newName as they were.  So, as far as conflicts go, a train's accumulator is a sorted list of
 * rename records: a step is smx_screen's walk of that list (A) against the log's sorted renames
 * (B), and a step without conflicts merges the two stably, A first on equal (ts, oid_hi,
 * oid_lo).  Nothing is composed, and no size is refused: there is no -2.
 *
 * For every valid train and step g, step_counts[2g+1] and the written records equal what
 * smx_compose_train reports for that step wherever it reports a count: the number of conflicts,
 * and per conflict the first two words of its record -- the A op's column index and the B op's
 * column index, in the reference's order.
 *
 *   step_counts  [2g]: the renames in the accumulator after step g, whatever happened;
 *                [2g+1]: >= 0 the step's conflicts (0: it landed; a log without renames
 *                        lands and leaves the accumulator's renames as they were);
 *                        -1 a log index outside [0, n_logs), a log invalid under smx_screen's
 *                           log_off rules, or an op with kind >= 18 in it: the accumulator
 *                           stays and the train goes on with its next log
 *   conflicts    per step g the first conf_off[g+1] - conf_off[g] records at conflicts[2 *
 *                conf_off[g]], two int32 each, the full number in step_counts[2g+1], nothing at
 *                or past the step's region (a negative or decreasing conf_off gives the step
 *                none).  conflicts and conf_off both NULL: capacity 0 everywhere (counts only).
 *   counts       [2r]: the renames in train r's final accumulator; [2r+1]: the steps that landed
 *   acc_off      train r may hold acc_off[r+1] - acc_off[r] renames: at least the sum of the
 *                rename counts of its steps' valid logs (a log counted once per step)
 *
 * A train whose train_off or acc_off entries are negative, below an earlier entry, decreasing
 * or past n_steps / n_acc, or whose region is smaller than that sum (checked on the device from
 * the extracted counts), reports counts -1, -1 and writes nothing else.  Failed trains and steps
 * never touch their neighbours.
 *
 * Stream-ordered as smx_compose_train: seven launches whatever the data, no host
 * synchronisation, no allocation, no read-back; the call clears the workspace state it needs,
 * so one workspace serves any sequence of calls, smx_screen_ex's among them where it is large
 * enough.  Every log's renames are extracted and sorted once, as with SMX_SCREEN_LARGE; one
 * workgroup runs a train's steps one after another, a step of more than 2048 renames in rounds.
 * flags must be 0.
 */
struct smx_screen_train {
  int64_t n_logs, n_total, n_trains, n_steps, n_acc;
  const int64_t* log_off;                 /* device [n_logs+1], as smx_screen */
  const uint8_t* kind; const uint64_t* ts, *oid_hi, *oid_lo;
  const uint32_t* sym; const int32_t* v0;          /* as smx_screen: n_total entries, no v1, no n_sym */
  const int64_t* train_off;               /* device [n_trains+1], into train_log, as smx_train */
  const int32_t* train_log;               /* device [n_steps]: log indices */
  const int64_t* acc_off;                 /* device [n_trains+1]: train r's room in renames, entries up to n_acc */
  int32_t* conflicts; const int64_t* conf_off;     /* 2 int32 per record; conf_off [n_steps+1], in records;
                                                      both NULL: counts only */
  int64_t* counts;                        /* [2*n_trains]: renames in the final accumulator, landed steps */
  int64_t* step_counts;                   /* [2*n_steps]: the accumulator's renames after the step, its outcome */
  int32_t grid_cap;                       /* as smx_batch; also caps the per-log launches */
};
/* Workspace (8-byte aligned), monotone in its arguments: 4 bytes per log, 20 per train, 44 per
 * op and 72 per entry of n_acc (all five sizes in 0 .. 2^31 - 1; n_steps is not stored; flags 0). */
int smx_screen_train_workspace_bytes(int64_t n_logs, int64_t n_total, int64_t n_trains, int64_t n_steps,
                                     int64_t n_acc, uint32_t flags, size_t* bytes);
/* SMX_E_ARG (a non-zero flag; then a null struct, negative sizes, a size over 2^31 - 1,
 * grid_cap < 0, exactly one of conflicts / conf_off null; a null train_off / acc_off / counts, a
 * null log_off with n_logs > 0, a null train_log / step_counts with n_steps > 0, a null column
 * with n_total > 0) and SMX_E_WORKSPACE (too small, or not 8-byte aligned) are reported before
 * any HIP call; n_trains = 0 returns SMX_OK and launches nothing. */
int smx_screen_train(const struct smx_screen_train* t, void* workspace, size_t workspace_bytes, uint32_t flags,
                     void* stream);

/*
 * Conflict screen of merge trains that share prefixes: which nodes of smx_compose_tree's tree
 * have DivergentRename conflicts, and which ones, from the logs' renames alone.
 * The logs and the columns are laid out as smx_screen_train takes them, the nodes as smx_tree
 * takes them: level by level, node_parent[n] SMX_NONE for a node of level 0 and a node of level
 * d-1 for a node of level d, node_log[n] its log.  As far as conflicts go an accumulator is a
 * sorted list of rename records (smx_screen_train above).  Node n walks its parent's list (A)
 * against its log's sorted renames (B); without conflicts it merges the two stably, A first on
 * equal (ts, oid_hi, oid_lo), into its own region, where all its children start.  Every log's
 * renames are extracted and sorted once and every node is walked once, however many root paths
 * run through it.  Nothing is composed, and no size is refused: there is no -2.
 *
 * For every valid node n, node_counts[2n], node_counts[2n+1] and the written records equal what
 * smx_screen_train reports (step_counts and records) for the last step of the train that is n's
 * root path.  So they also equal, wherever smx_compose_tree / smx_compose_train report a count,
 * that count and the first two words of each of their records.
 *
 *   node_counts  [2n]: the renames in the accumulator after the node, whatever happened;
 *                [2n+1]: >= 0 the node's conflicts (0: it landed; a log without renames lands
 *                        and leaves the accumulator's renames as they were);
 *                        -1 a log index outside [0, n_logs), a log invalid under smx_screen's
 *                           log_off rules, or an op with kind >= 18 in it: the accumulator
 *                           stays the parent's, and the children go on from it
 *   conflicts    per node n the first conf_off[n+1] - conf_off[n] records at conflicts[2 *
 *                conf_off[n]], two int32 each (the A op's column index, the B op's column index),
 *                the full number in node_counts[2n+1], nothing at or past the node's region (a
 *                negative or decreasing conf_off gives the node none).  conflicts and conf_off
 *                both NULL: capacity 0 everywhere (counts only).
 *   acc_off      node n may hold acc_off[n+1] - acc_off[n] renames.  Let P(n) be the sum, over
 *                the nodes of n's root path with valid logs (n included), of their logs' rename
 *                counts.  A node whose own log is valid and has renames needs at least P(n); any
 *                other node needs nothing (it writes no accumulator: the list stays where its
 *                parent's is).  Region space is quadratic in the depth of a stack, and
 *                rename-free logs, the common ones, cost none.
 *
 * A node fails structurally -- node_counts[2n] = node_counts[2n+1] = -1, nothing else written --
 * when
 *   - it lies in no valid level (smx_tree's rules: level_off[d] not negative and not below an
 *     earlier entry, level_off[d+1] not below level_off[d] and not past n_nodes, level 0 starts
 *     at node 0 and the last level ends at n_nodes);
 *   - its parent is not in the level before (no node is in an invalid level), or it is of
 *     level 0 and has a parent;
 *   - its acc_off entries are negative, below an earlier entry, decreasing or past n_acc;
 *   - its region is below the room rule (checked on the device from the extracted counts);
 *   - its parent failed structurally.
 * All of this is checked on the device before any index is read through.  Failed nodes never
 * touch their neighbours.
 *
 * Stream-ordered: the offsets' check, the two extraction launches of SMX_SCREEN_LARGE over every
 * log, a pre-pass over the nodes, then per level one launch for each of the three size classes
 * of smx_screen (128 / 512 / 2048 renames, by min(P(n), 2048); a node whose own log is invalid
 * or has no renames is of the smallest class): 4 + 3 * n_levels launches whatever the data.  A
 * node of more than 2048 renames runs in rounds.  A level depends on the level before through
 * stream order alone: no workgroup waits for another one.  No host synchronisation, no
 * allocation, no read-back; the call clears the workspace state it needs, so one workspace
 * serves any sequence of smx_screen_tree, smx_screen_train and smx_screen_ex calls it is large
 * enough for.  grid_cap caps every launch.  flags must be 0.
 */
struct smx_screen_tree {
  int64_t n_logs, n_total, n_nodes, n_levels, n_acc;   /* n_levels: a host scalar, as smx_tree */
  const int64_t* log_off;                 /* device [n_logs+1], as smx_screen */
  const uint8_t* kind; const uint64_t* ts, *oid_hi, *oid_lo;
  const uint32_t* sym; const int32_t* v0;          /* as smx_screen: n_total entries, no v1, no n_sym */
  const int64_t* level_off;               /* device [n_levels+1], into the nodes, as smx_tree */
  const int32_t* node_parent;             /* device [n_nodes]: a node of the level before, or SMX_NONE */
  const int32_t* node_log;                /* device [n_nodes]: log indices */
  const int64_t* acc_off;                 /* device [n_nodes+1]: node n's room in renames, entries up to n_acc */
  int32_t* conflicts; const int64_t* conf_off;     /* 2 int32 per record; conf_off [n_nodes+1], in records;
                                                      both NULL: counts only */
  int64_t* node_counts;                   /* [2*n_nodes]: the accumulator's renames after the node, its outcome */
  int32_t grid_cap;                       /* as smx_batch; also caps the per-log launches */
};
/* Workspace (8-byte aligned), linear in its arguments, each term rounded up to 256 bytes: a
 * 256-byte header, 4 bytes per log, 28 per node (the three class lists, two verdicts and the node
 * that holds its accumulator), 20 per level (its class counts and a verdict), 44 per op (36 of
 * rename records, 8 of the large logs' index arrays) and 36 per entry of n_acc.  n_logs,
 * n_total, n_nodes, n_acc in 0 .. 2^31 - 1, n_levels in 0 .. SMX_TREE_MAX_LEVELS; flags 0. */
int smx_screen_tree_workspace_bytes(int64_t n_logs, int64_t n_total, int64_t n_nodes, int64_t n_levels,
                                    int64_t n_acc, uint32_t flags, size_t* bytes);
/* SMX_E_ARG (a non-zero flag; then a null struct, negative sizes, n_levels over
 * SMX_TREE_MAX_LEVELS, n_logs, n_total, n_nodes or n_acc over 2^31 - 1, grid_cap < 0, exactly one
 * of conflicts / conf_off null; a null level_off / node_parent / node_log / acc_off /
 * node_counts, a null log_off with n_logs > 0, a null column with n_total > 0) and
 * SMX_E_WORKSPACE (too small, or not 8-byte aligned) are reported before any HIP call;
 * n_nodes = 0 returns SMX_OK and launches nothing. */
int smx_screen_tree(const struct smx_screen_tree* t, void* workspace, size_t workspace_bytes, uint32_t flags,
                    void* stream);

/*
 * Sharded single merge: one process per GPU, shard r of G.
 * Replaces the same reference loop as smx_compose (compose.py:11-114) for a merge
 * too large for one GPU.  Shard r holds, for both branches, the ops whose
 * timestamp keys fall in its key range [tau_r, tau_{r+1}): contiguous index
 * ranges of the global branch logs (branch logs must be timestamp-ordered, as
 * lift.ts emits them; the host's all-to-all puts them there).  For each kind
 * the shards' T-ordered segments follow each other in shard order, so the
 * global composed log is, kind by kind, the shards' outputs concatenated.
 *
 * The host drives four steps on the same workspace, exchanging the small
 * per-shard summaries (and the partial tables) between them with collectives:
 *   SMX_SHARD_ORDER   plan + window kernels; writes summary[0..21] and the
 *                     first halo_cap renames of each branch (export_*).  With
 *                     src_map == NULL it is asynchronous (no host sync): the
 *                     presorted plan only; a failure shows in summary[21]
 *                     (bit 0 not ordered, bit 1 invalid input, bit 2 a window
 *                     overflowed on dense timestamp ties) and is repaired by
 *   SMX_SHARD_ORDER_FIX  the plan fallbacks (smaller windows; with b_gap = 0 the
 *                     segmented or radix plan, never for a slice whose timestamps
 *                     decrease: that returns SMX_E_ARG); rewrites summary[0..21]
 *                     and the exports
 *   SMX_SHARD_WALK    DivergentRename walk with the halo (the next shards'
 *                     exports) and an incoming open region (in_ahead, in_d);
 *                     may be re-run when the incoming region changes;
 *                     writes summary[22..27]
 *   SMX_SHARD_TABLES  this shard's last writers -> part_tab (MAX-reduce them
 *                     over shards next); writes summary[28..30].  ORDER and
 *                     ORDER_FIX already bucket the table records (beside the
 *                     walk); TABLES applies the walk's skips to them, which it can
 *                     do once (a second TABLES without ORDER / ORDER_FIX / SCATTER
 *                     in between returns SMX_E_ARG):
 *   SMX_SHARD_SCATTER re-buckets the records, for a TABLES after a WALK re-run
 *   SMX_SHARD_EMIT    composed output from the reduced tables (fin_tab) and
 *                     the global value widths (glob[0..2]); mv_prefix (or NULL
 *                     when no move has a None value) = [2][n_sym] last non-None
 *                     move values of the lower shards.  With summary_host set
 *                     (this shard's summary as the host last gathered it) the
 *                     step needs no host sync.
 * Source indices in order[] and conflicts are global: local A op j is
 * src_a + j, local B op j is src_b + j.  summary (int64):
 *   [0..17] ops per kind  [18..19] renames of A, B  [20] moves with a None value
 *   [21] plan failure (not timestamp-ordered / invalid input)
 *   [22] outgoing region open  [23] its ahead branch  [24] its d
 *   [25] conflicts  [26] skipped renames  [27] halo too short
 *   [28..30] bit widths of (value + 1) for addr, file, ctx
 *   [31] a value too wide for the tab32 entries (TABLES with tab32 > 0)
 */
#define SMX_SHARD_ORDER 0
#define SMX_SHARD_WALK 1
#define SMX_SHARD_TABLES 2
#define SMX_SHARD_EMIT 3
#define SMX_SHARD_ORDER_FIX 4
#define SMX_SHARD_SCATTER 5
#define SMX_SHARD_SUMMARY 32

typedef struct smx_shard {
  int32_t rank;
  int32_t world;
  int64_t src_a;
  int64_t src_b;
  /* walk: the renames of each branch after this shard's (device) */
  int64_t halo_n[2];
  int32_t halo_more[2];
  const uint32_t* halo_sym[2];
  const int32_t* halo_cls[2];
  const int32_t* halo_src[2];
  int32_t in_ahead;
  int64_t in_d;
  /* outputs of the steps (device) */
  int64_t* summary;
  int64_t halo_cap;
  uint32_t* export_sym; /* [2][halo_cap] */
  int32_t* export_cls;
  int32_t* export_src;
  uint64_t* part_tab;   /* [3][n_sym] */
  /* inputs of the emit step (device) */
  const uint64_t* fin_tab;   /* [3][n_sym], MAX-reduced part_tab */
  const int64_t* glob;       /* [3] value bit widths, MAX over shards */
  const uint64_t* mv_prefix; /* [2][n_sym] or NULL */
  /* Device-held alternatives, so a step needs no host round trip (NULL: the host
   * fields above are used). */
  const int64_t* halo_dev;     /* [4] halo_n[0], halo_n[1], halo_more[0], halo_more[1] */
  const int64_t* in_state_dev; /* [2] in_ahead, in_d */
  /* A shard built by a sample-sort exchange (branch logs in any order; b_gap = 0):
   * the global source index of each local op j, [n_a + n_b]; replaces src_a/src_b
   * and lets the ORDER step use the generic (sorting) plan.  NULL otherwise. */
  const int32_t* src_map;
  /* host memory: this shard's summary [SMX_SHARD_SUMMARY] after WALK, or NULL */
  const int64_t* summary_host;
  /* Device, or NULL: the all-gather of every shard's ORDER outputs, row q =
   * shard q's summary [SMX_SHARD_SUMMARY] then its exports (export_sym, export_cls,
   * export_src, each [2][halo_cap] 32-bit) -- [world][SMX_SHARD_SUMMARY + 3 * halo_cap]
   * int64.  When set, the WALK step first assembles this shard's halo from it on the
   * device: halo_sym / halo_cls / halo_src ([halo_cap] each, writable) and halo_dev
   * (writable) are then outputs, so the host needs no read of the summaries. */
  const int64_t* order_gather;
  /* 0: part_tab / fin_tab are uint64 [3][n_sym] (+ glob, int64 [3]), entries
   * (rank + 1) << 32 | (value + 1).  tab32 > 0: half the MAX all-reduce -- they are
   * int32 [3 * n_sym + 3], entries (rank + 1) << (31 - tab32) | (value + 1) (a tag of
   * tab32 bits under a clear sign bit, so an int32 MAX keeps the last writer), the
   * three value widths after them (glob unused); a value too wide for the 31 - tab32
   * bits sets summary[31] and the caller redoes the step with tab32 = 0. */
  int32_t tab32;
} smx_shard;

int smx_shard_step(const smx_ops* ops, const smx_shard* shard, const smx_compose_out* out,
                   void* workspace, size_t workspace_bytes, void* stream, int step);

/*
 * The range plan's per-rank info for the sharded exchange (shard.py _range_info), in
 * two launches instead of a dozen tensor operations.  ts: the rank's timestamp buffer;
 * its A slice is ts[off_a, off_a + n_a), its B slice ts[off_b, off_b + n_b).  out
 * (int64, 9 + 4 * rh, device): n_a, n_b; the first and last key of the A slice, of the B
 * slice (keys: the u64 timestamp with its top bit flipped, so that int64 order is u64
 * order; 0 for an empty slice); 1 if both slices are non-decreasing (check_order = 0:
 * not checked, 1); signed_a, signed_b; then rh keys from the head of the A slice and rh
 * from its tail (right-aligned), the same for B (a slice shorter than rh pads with its
 * first key).
 */
int smx_shard_range_info(const uint64_t* ts, int64_t off_a, int64_t n_a, int64_t off_b, int64_t n_b, int32_t rh,
                         int32_t check_order, int32_t signed_a, int32_t signed_b, int64_t* out, void* stream);

/*
 * Per-stage device timing of the last smx_compose calls on this thread, for the
 * benchmark: when enabled, each stage is bracketed by hipEvents on the call's
 * stream and the elapsed milliseconds are accumulated per stage.
 * smx_stage_times copies up to `cap` entries and returns the number of stages;
 * smx_stage_name(i) names stage i.  smx_set_profiling_stages limits the timing to the
 * stages whose bit (1 << i) is set (default: all), so that a benchmark can time one
 * kernel without an event pair around every stage of every merge.
 */
int smx_set_profiling(int enabled);
int smx_set_profiling_stages(uint32_t mask);
int smx_stage_times(double* ms, int64_t* calls, int cap);
const char* smx_stage_name(int i);
int smx_reset_stage_times(void);

/*
 * Batched RGA replay (crdt.py:23-57): n_ops events over n_lists independent
 * lists, events of one list in stream order (list[i] non-decreasing is NOT
 * required; stream order is the index order).
 *   list[i]   list id < n_lists
 *   op[i]     0 = insert(key, value), 1 = move(value, key), 2 = delete(value)
 *   value[i]  interned value (equality class of the value string)
 *   key_*[i]  order-preserving image of Key(anchor, t, author, opid):
 *             anchor rank (u32), t (i64, compared signed), author rank (u32),
 *             opid 128-bit key; ignored for delete
 * Output: out_value[k] for the surviving elements of every list in list order
 * then list-position order, out_offsets[l] = first output index of list l
 * (n_lists + 1 entries), out_src[k] = index of the event that created element k.
 */
typedef struct smx_rga_ops {
  int64_t n_ops;
  int64_t n_lists;
  const uint32_t* list;
  const uint8_t* op;
  const uint32_t* value;
  const uint32_t* anchor;
  const int64_t* t;
  const uint32_t* author;
  const uint64_t* opid_hi;
  const uint64_t* opid_lo;
} smx_rga_ops;

typedef struct smx_rga_out {
  uint32_t* out_value;
  int32_t* out_src;
  int64_t* out_offsets;
  int64_t* counts; /* counts[0] = surviving elements */
  /* NULL: the output is materialize() (live elements only).  Non-NULL: the output is
   * the whole list state RGA.list (crdt.py:26-27) -- the live elements and the ones
   * delete() tombstoned, in list order -- and out_tomb[k] = 1 marks the tombstoned
   * ones (0 the live ones); counts[0] = elements in the lists. */
  uint8_t* out_tomb;
} smx_rga_out;

int smx_rga_workspace_bytes(int64_t n_ops, int64_t n_lists, size_t* bytes);
int smx_rga_replay(const smx_rga_ops* ops, const smx_rga_out* out, void* workspace,
                   size_t workspace_bytes, void* stream);

/* smx_rga_replay with flags.  SMX_RGA_GROUPED: the caller's events come list by list
 * (list ids never decrease -- what crdt.replay and the RGA drop-in build, one stream
 * after another), so the library packs the records in place instead of partitioning
 * them by list.  The claim is checked on the device: a list id that decreases makes the
 * call redo itself through the partition (same results, the partition's cost).
 * smx_rga_replay(...) == smx_rga_replay_ex(..., 0, stream). */
#define SMX_RGA_GROUPED 1u
int smx_rga_replay_ex(const smx_rga_ops* ops, const smx_rga_out* out, void* workspace,
                      size_t workspace_bytes, uint32_t flags, void* stream);

/*
 * RGA replay of many jobs onto base lists stored once (a merge queue, a rebase, a
 * three-way list reconcile: the same base list takes many branches' events).  The events
 * of job j are the events of base job_base[j] followed by the job's own events, in stream
 * order, and the job's results are exactly those of smx_rga_replay on that concatenated
 * stream as one list, in both output modes -- but a base's events are stored, copied and
 * read from one place however many jobs name it.
 *   base_off  [n_bases + 1]: base b's events are columns [base_off[b], base_off[b + 1])
 *   own_off   [n_jobs + 1]:  job j's own events are columns [own_off[j], own_off[j + 1])
 *   job_base  [n_jobs]:      a base index < n_bases, or SMX_NONE for a job without a base
 *   op .. opid_lo            the event columns of smx_rga_ops, n_total entries each; values,
 *                            anchors and authors form one id domain for the whole call (an
 *                            own move or delete reaches a base element of the same value id)
 * The bases lie before the own events: base_off[n_bases] <= own_off[0].  The creation index
 * that breaks ties between equal keys is the column index, so a base's elements come before
 * a job's own and, among own events, column order decides.  A base named by no job is never
 * read; jobs may name their bases in any order; a base or an own range may be empty.
 * Output: smx_rga_out with one "list" per job: out_offsets has n_jobs + 1 entries,
 * out_value / out_src / out_tomb have capacity n_out (at least the sum over the jobs of
 * their base's and their own events), out_src[k] is the COLUMN index of the event that
 * created element k (a base's or an own one), counts[0] the total.
 * Stream-ordered on `stream`; ends, as smx_rga_replay does, with the read-back of one
 * error word and a stream wait: SMX_E_ARG for an op > 2 among a job's events, an offset that
 * is negative, decreasing or past n_total, bases that do not lie before the own events, a
 * job_base outside [-1, n_bases), or job lengths that sum to more than n_out (all found on
 * the device before a column is read out of bounds).  Sizes that are negative, n_total or
 * n_out above 2^30 - 1, a null pointer with a non-zero size and a workspace that is too
 * small or not 16-byte aligned come back (SMX_E_ARG / SMX_E_WORKSPACE) before any HIP call.
 * n_jobs = 0 writes out_offsets[0] = 0 and counts[0] = 0.  One workspace serves any
 * sequence of calls, smx_rga_replay's included when it is large enough for each.
 */
typedef struct smx_rga_onto {
  int64_t n_total; /* events in the columns */
  int64_t n_bases;
  int64_t n_jobs;
  int64_t n_out;
  const int64_t* base_off;
  const int64_t* own_off;
  const int32_t* job_base;
  const uint8_t* op;
  const uint32_t* value;
  const uint32_t* anchor;
  const int64_t* t;
  const uint32_t* author;
  const uint64_t* opid_hi;
  const uint64_t* opid_lo;
} smx_rga_onto;

int smx_rga_replay_onto_workspace_bytes(int64_t n_jobs, int64_t n_out, size_t* bytes);
int smx_rga_replay_onto(const smx_rga_onto* onto, const smx_rga_out* out, void* workspace,
                        size_t workspace_bytes, void* stream);

/*
 * RGA replay of many jobs that are runs of segments stored once (a three-way list reconcile
 * base ++ target ++ pull request over K targets and M pull requests; the list a merge train
 * leaves, base ++ the landed logs' events; the states after commits 1, 1..2, ... 1..n of a
 * stack).  smx_rga_replay_onto's job is two column ranges; here it is any number.  The events
 * of job j are the events of its segments, one segment after another in job_seg order, and the
 * job's results are exactly those of smx_rga_replay on that concatenated stream as one list,
 * in both output modes -- but a segment's events are stored, copied and read from one place
 * however many jobs name it.
 *   seg_off   [n_segs + 1]: segment s is columns [seg_off[s], seg_off[s + 1])
 *   job_off   [n_jobs + 1]: job j's segments are job_seg[job_off[j] .. job_off[j + 1])
 *   job_seg   [n_links]:    segment indices < n_segs
 *   op .. opid_lo           the event columns of smx_rga_ops, n_total entries each; values,
 *                           anchors and authors form one id domain for the whole call (a move
 *                           or delete in one segment reaches an element of the same value id
 *                           that an earlier segment of the job created)
 * Within a job the segment indices strictly ascend, and seg_off does not decrease.  The
 * creation index that breaks ties between equal keys is the column index, and column order is
 * the concatenated stream's order only if a job's segments ascend; it also means that no job
 * names a segment twice.  (Store the base, then the targets, then the pull requests; or the
 * commits in stack order.)  A job may skip segments; jobs may come in any order; a segment may
 * be in any number of jobs or in none, and one that no job names is never read; a segment or
 * a job may be empty.
 * Output: smx_rga_out with one "list" per job: out_offsets has n_jobs + 1 entries,
 * out_value / out_src / out_tomb have capacity n_out (at least the sum over the jobs of their
 * segments' events), out_src[k] is the COLUMN index of the event that created element k,
 * counts[0] the total.
 * Stream-ordered on `stream`, in a number of launches that does not depend on the data; ends,
 * as smx_rga_replay_onto does, with the read-back of one error word and a stream wait:
 * SMX_E_ARG ("invalid input") for a seg_off or job_off entry that is negative, decreasing or
 * past n_total / n_links, a job_seg outside [0, n_segs), segment indices that do not strictly
 * ascend within a job, an op > 2 in a segment that some job names, or job lengths that sum to
 * more than n_out (all found on the device before a column is read through an unchecked
 * offset); the next call on the same workspace is served.  A null struct or output, sizes that
 * are negative, n_total or n_out above 2^30 - 1, n_segs, n_jobs or n_links at or above
 * 2^31 - 1, a null pointer with a non-zero size and a workspace that is too small or not
 * 16-byte aligned come back (SMX_E_ARG / SMX_E_WORKSPACE) before any HIP call.
 * n_jobs = 0 writes out_offsets[0] = 0 and counts[0] = 0 and needs no workspace.
 * Workspace: smx_rga_replay_onto's for (n_jobs, n_out) without its 16 bytes per job, plus the
 * column map, 4 bytes per entry of n_out, and the link scan's two arrays, 4 (n_links + 1) bytes
 * each; every part rounded up to 256 bytes.  Each call clears the state it needs, so one
 * workspace serves any sequence of smx_rga_replay_ex, smx_rga_replay_onto and
 * smx_rga_replay_chain calls that it is large enough for.
 */
typedef struct smx_rga_chain {
  int64_t n_total; /* events in the columns */
  int64_t n_segs;
  int64_t n_jobs;
  int64_t n_links;
  int64_t n_out;
  const int64_t* seg_off;
  const int64_t* job_off;
  const int32_t* job_seg;
  const uint8_t* op;
  const uint32_t* value;
  const uint32_t* anchor;
  const int64_t* t;
  const uint32_t* author;
  const uint64_t* opid_hi;
  const uint64_t* opid_lo;
} smx_rga_chain;

int smx_rga_replay_chain_workspace_bytes(int64_t n_jobs, int64_t n_links, int64_t n_out, size_t* bytes);
int smx_rga_replay_chain(const smx_rga_chain* c, const smx_rga_out* out, void* workspace,
                         size_t workspace_bytes, void* stream);

const char* smx_last_error(void);
const char* smx_version(void);

#ifdef __cplusplus
}
#endif

#endif /* SMX_H */
