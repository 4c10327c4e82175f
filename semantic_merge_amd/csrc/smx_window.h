// smx_window.h — per-window T-order construction (the dominant kernel).
//
// T = stable order of A||B by (precedence, timestamp, id, side, index)
// (semmerge/compose.py:16-21 sorted() per branch + the A-first merge of :51-56).
// A window is a pair of contiguous ranges, one per branch, such that every op of
// the window precedes, in (timestamp, id, side, index) order, every op of the
// next window.  An op's T position = base[kind] + (ops of that kind in earlier
// windows) + its place among the window's ops of that kind.
//
// The presorted kernel (k_window_f) handles branch logs whose timestamps never
// decrease (lift.ts emits them in order).  Its order is run-grouped: no merge, no
// multisplit, all in LDS.  Inside a branch part the timestamps never decrease, so the
// equal-timestamp ops of both parts form one run of the merged order S, which starts
// at S position spos(v) = #{A ops < v} + #{B ops < v} (A first on ties, compose.py:54).
// Each run's heads (the first op of its value in a part) find spos by a 64-way search
// of the other part; the runs' dense index r comes from an occupancy mask over S
// positions.  An op's group is (kind, r) and the groups laid out kind-major ARE the
// window's T order of groups (T is ordered by kind, then timestamp): one histogram +
// scan of KD * R counters gives every group's start, then each group is ordered by
// (id, side, index) with interpolation buckets on the top 32 bits of the id (one op
// per bucket on random ids) and a rank inside the bucket, equal 32-bit keys on the full
// ids.  A window with more than GMAX groups (very many distinct timestamps) fails the
// plan as a window too large (f_fail 2): the host retries with smaller windows.
//
// The generic kernel (k_window_g) is the one that merges: it handles branch logs that
// the generic path pre-sorted by (timestamp, id), with a merge path over the full keys
// (A first on ties) and a stable multisplit of the merged order by kind (wave64
// ballots); no order inside a group is left to find.
//
// What a window writes, T-ordered:
//   moves (T < nMv)     the FINAL composed records: no skip precedes the rename
//                       block, so a move's output index is T, and it carries its own
//                       newAddress / newFile (compose.py:37-43; a None value is
//                       patched later from the symbol's prefix, k_mv_fix); plus
//                       msym[T] = sym | has-address << 30 | has-file << 31 for the
//                       last-writer tables
//   every other op      tsrc / tsym at P = T - nMv (renames first, then the rest):
//                       the source op and the symbol that k_emit needs
//   renames             Rstr[m] (the rename-chain value, compose.py:71-72), m = P
//   DivergentRename     the natural-head test (compose.py:60-70, 88-98 at d = 0) of
//                       each rename against the other branch's next rename inside
//                       the window; flagged positions go to the window's candidate
//                       slots; the renames after the other branch's last rename of
//                       the window are tested by k_boundary (smx_walk.h)
//   per window          wren (renames / A renames before it), wbnd (where its
//                       boundary renames start)
#pragma once

#include "smx_common.h"

#define WIN_CAP 2048               // max ops per window held in LDS
#ifndef WIN_TGT
#define WIN_TGT 1792               // default target window size, presorted path (SMX_WIN_TGT)
#endif
#define WIN_TGT_MIN 256
#define NCNT (SMX_N_KINDS + 3)     // kinds, renames per branch, moves with a None value
#define CNT_REN_A SMX_N_KINDS
#define CNT_REN_B (SMX_N_KINDS + 1)
#define CNT_NONE_MV (SMX_N_KINDS + 2)
#define KMOVE SMX_KIND_MOVE
#define KREN SMX_KIND_RENAME
#define NCHUNK (WIN_CAP / WAVE)
#define CH 256                     // chunk of the presorted kind histogram
#define SYM_MASK 0x3fffffffu       // msym: symbol bits (n_sym <= 2^30)
#define MS_HAS_A (1u << 30)
#define MS_HAS_F (1u << 31)

// Four consecutive i32 stores as one 16-byte store (4-byte aligned address).
typedef i32 __attribute__((ext_vector_type(4))) win_v4i;
typedef win_v4i __attribute__((aligned(4))) win_v4i_a4;
__device__ __forceinline__ void st4(i32* p, i32 a, i32 b, i32 c, i32 d) {
  *reinterpret_cast<win_v4i_a4*>(p) = win_v4i{a, b, c, d};
}

struct WinArgs {
  const u8* kind;
  const u32* sym;
  const i32* v0;
  const i32* v1;
  // branch view: presorted -> keys at op index j; generic -> sorted copies at j
  const u64* kts;
  const u64* khi;
  const u64* klo;
  const u32* perm;  // generic only: op index of sorted position (A at [0,na), B at [na,n))
  i64 na;
  i64 nb;
  i64 bgap;         // B op j is stored at j + bgap of the field arrays (presorted plan)
  i64 W;
  i64 n_sym;
  i64 src_a, src_b; // global source index of local op j (sharded merge; 0 / na otherwise)
  const i32* src_map;  // sample-sorted shard: global source of local op j, or null
  int ablate;       // diagnostic builds only (SMX_ABLATE): skip phases, results invalid
  const i64* bnd;
  const u32* woff;  // [NCNT][W] exclusive offsets over windows (generic plan)
  const u32* cpre;  // presorted plan: [2][kinds][CM] chunk prefixes (256-op chunks)
  i64 CM;
  ComposeMeta* meta;
  // outputs (module comment)
  i32* out_order;
  i32* out_addr;
  i32* out_file;
  i32* out_ctx;
  u32* msym;
  i32* tsrc;
  u32* tsym;
  i32* Rstr;
  u32* wren;        // [W][2]
  u32* wbnd;        // [W]: first boundary rename (window-local) | its branch << 31
  u32* cslot;       // candidate M positions, window w's from M offset wren[2w]
  u32* wcand;       // [W] in-window candidates
  u64* dbg;         // diagnostics only: phase timestamps (k_window_f<true>)
};

// OR of the per-wave value widths into meta->vbits (k_tb_reduce packs the final-state
// table with them); an atomic only when it adds bits.
__device__ __forceinline__ void win_publish_widths(ComposeMeta* meta, const u32* vbw, int nw) {
  for (int q = 0; q < 3; ++q) {
    u32 m = 0;
    for (int w = 0; w < nw; ++w) m |= vbw[w * 3 + q];
    const u32 cur = __hip_atomic_load(&meta->vbits[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if ((cur | m) != cur) atomicOr(&meta->vbits[q], m);
  }
}
// ... with the published widths read beforehand (cur[3]): no global round trip here
__device__ __forceinline__ void win_publish_widths(ComposeMeta* meta, const u32* vbw, int nw, const u32* cur) {
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    u32 m = 0;
    for (int w = 0; w < nw; ++w) m |= vbw[w * 3 + q];
    if ((cur[q] | m) != cur[q]) atomicOr(&meta->vbits[q], m);
  }
}

__device__ __forceinline__ i32 win_gsrc(const WinArgs& P, i64 j) {
  if (P.src_map) return P.src_map[j];
  return j < P.na ? (i32)(P.src_a + j) : (i32)(P.src_b + (j - P.na));
}

// The window's renames in final order, x = 0 .. RN-1: branch s(x), rank own(x) in
// its branch's renames of the window, posl = the window-local x of each branch's
// renames (A's first, then B's).  Natural head of x: the other branch's next
// rename, the (x - own(x))-th of that branch in the window if there is one.
// Flags -> candidate slots in M order; thread 0 writes where the boundary renames
// (after the other branch's last rename of the window) start.
// SymCls(x) -> (symbol, newName class) of rename x.
template <int NT, int NCHK, typename SideOwn, typename SymCls>
__device__ __forceinline__ void win_rename_flags(const WinArgs& P, i64 w, u64 Mbase, int RN, int cntA,
                                                 int cntB, const u16* posl, u64* cb, SideOwn side_own,
                                                 SymCls sym_cls) {
  constexpr int NW = NT / WAVE;
  const int t = threadIdx.x, lane = t & (WAVE - 1), wv = t / WAVE;
  const int nrc = (RN + WAVE - 1) / WAVE;
  for (int c = wv; c < nrc; c += NW) {
    const int x = c * WAVE + lane;
    bool f = false;
    if (x < RN) {
      int s, own;
      side_own(x, &s, &own);
      const int k = x - own;
      if (k < (s ? cntA : cntB)) {
        const int h = posl[(s ? 0 : cntA) + k];
        const uint2 me = sym_cls(x), hd = sym_cls(h);
        f = me.x == hd.x && me.y != hd.y;
      }
    }
    const u64 b = __ballot(f);
    if (lane == 0) cb[c] = b;
  }
  if (t == 0) {
    // boundary renames: those after the other branch's last rename of the window
    u32 bnd = 0;
    if (RN) {
      int s, own;
      side_own(RN - 1, &s, &own);
      const int cnt_o = s ? cntA : cntB;
      const u32 bx = cnt_o ? (u32)posl[(s ? 0 : cntA) + cnt_o - 1] + 1u : 0u;
      bnd = bx | ((u32)s << 31);
    }
    P.wbnd[w] = bnd;
  }
  __syncthreads();
  const u64 nall = (u64)(P.na + P.nb);
  for (int c = wv; c < nrc; c += NW) {
    const u64 b = cb[c];
    if (!b) continue;
    u32 before = lane < c ? (u32)__popcll(cb[lane]) : 0u;  // chunks before c
    if (NCHK > WAVE) before += WAVE + lane < c ? (u32)__popcll(cb[WAVE + lane]) : 0u;
    before = wave_incl_sum(before);
    before = __builtin_amdgcn_readlane(before, WAVE - 1);
    if ((b >> lane) & 1ull) {
      const u64 slot = Mbase + before + (u32)__popcll(b & lanemask_lt());
      if (slot < nall) P.cslot[slot] = (u32)(Mbase + (u64)(c * WAVE + lane));
    }
  }
  if (t == 0) {
    u32 tot = 0;
    for (int c = 0; c < nrc; ++c) tot += (u32)__popcll(cb[c]);
    P.wcand[w] = tot;
  }
}

// ---------------------------------------------------------------------------
// presorted windows (timestamps non-decreasing in each branch log)

#ifndef WF_NT
#define WF_NT 512
#endif
#ifndef WF_CAP
#define WF_CAP WIN_CAP              // max ops per presorted window
#endif
#ifndef WF_WIDE_CAP
#define WF_WIDE_CAP 8192  // the wide presorted window (run_presorted(wide)): one per CU
#endif
#define WF_WIDE_NT 1024
#define WF_NCH (WF_CAP / WAVE)
#define WF_WAVES (WF_NT / WAVE)
#define WF_ITEMS (WF_CAP / WF_NT)
#define WF_KP ((2 * CH + WF_NT - 1) / WF_NT)  // partial-chunk kinds per lane

// LDS 40,640 B (buffers are reused across steps; four workgroups fit a CU up to 40,960 B
// each, and the bucket counters take a word each: DESIGN.md §5) so 4 workgroups fit a CU: while
// some workgroups run their LDS steps, others stream their windows from HBM.
// DBG: step timestamps of every window (diagnostics, tools/window_phases.py):
// lane 0 of wave 0 stores s_memtime at the start (i = 0) and after step i = 1 .. 14 into
// P.dbg[w * WF_NSTAMP + i].
#define WF_NSTAMP 16
// Diagnostic builds: SMX_ABLATE = 100 + N leaves the kernel after step N = 2 .. 13 (timing
// of the steps by difference, tools/window_ablate.py); results invalid.  The bit-tested
// ablations (WF_ABL: 4 = stop before the payload, 16 = load only) are values below 100.
#define WF_EXIT(N)                                                         \
  do {                                                                     \
    if (SMX_DIAG && P.ablate == 100 + (N)) {                               \
      if (t == 0 && sord[0] == 0xfffeu && rown[1] == 0xfffeu) P.meta->dup_key = 1; \
      return;                                                              \
    }                                                                      \
  } while (0)
#define WF_ABL(bit) (SMX_DIAG && P.ablate < 100 && (P.ablate & (bit)))
#define WSTAMP(i)                                                                  \
  do {                                                                             \
    if (DBG && t == 0) P.dbg[w * WF_NSTAMP + (i)] = __builtin_amdgcn_s_memtime(); \
  } while (0)

// MAP: the sample-sorted shard's source map (P.src_map) is read; a separate instance so
// that the plain path's store loop has no load whose wait would also drain its stores
#ifndef WF_MINB
#define WF_MINB 8
#endif
template <int CAP, int NT, bool DBG, bool MAP>
__global__ void __launch_bounds__(NT, CAP > WF_CAP ? 4 : WF_MINB) k_window_f(WinArgs P) {
  // CAP ops per window on NT threads: (2048, 512) four windows per CU; (8192, 1024) one
  // window per CU for logs whose equal-timestamp groups need it (config 5)
  constexpr int ITEMS = CAP / NT, NCH = CAP / WAVE, WAVES = NT / WAVE, KP = (2 * CH + NT - 1) / NT;
  static_assert(CAP % NT == 0 && NCH <= 2 * WAVE && CAP <= 65536, "window geometry");
  constexpr int OW = CAP / 32;     // occupancy words over S positions
  // sts: the timestamps by element (steps 1-2); the group counters, then starts (gcnt, steps
  // 3-6); the members in bucket order (mkey, mel, steps 8-9); the payload by final slot
  // (st_a, st_b, steps 11-14)
  __shared__ __attribute__((aligned(16))) u64 sts[CAP];
  __shared__ __attribute__((aligned(16))) u16 sord[CAP];  // final slot -> element (step 9 on)
  __shared__ __attribute__((aligned(16))) u32 bcnt[CAP];  // bucket counters, then starts, one per word (steps 1-9); then rown
  __shared__ u16 sp[CAP];         // head element -> S position of its run (steps 2-4); later posl
  __shared__ __attribute__((aligned(16))) u8 skS[CAP];  // kinds by final slot (step 9 on)
  __shared__ u16 inv[CAP];        // element -> final slot
  __shared__ u64 tbase[SMX_N_KINDS]; // T of a kind's slot x = tbase[kind] + x
  __shared__ u64 gbits[NCH];       // run-head ballots per 64-op chunk (steps 2-4), later candidate ballots
  __shared__ u32 occ[OW];          // bit s: a run starts at S position s (steps 1-4)
  __shared__ u16 rc[NCH][2];      // per 64 renames: those of A, of B; then their exclusive prefixes
  __shared__ u32 kbase[SMX_N_KINDS + 1];  // first final slot of each kind
  __shared__ u32 wck[SMX_N_KINDS];        // the window's ops of each kind
  __shared__ u64 base[SMX_N_KINDS + 1];
  __shared__ u32 woffk[SMX_N_KINDS + 2];  // this window's offsets: kinds, renames of A, of B
  __shared__ u32 wtot[2];                 // the window's renames of A, of B
  __shared__ u32 vbw[WAVES][3];        // per wave: value widths (addr, file, name); later the block scans' scratch
  u16* rown = reinterpret_cast<u16*>(bcnt);  // rename rank within its branch (step 10 on)

  const int t = threadIdx.x;
  const int lane = t & (WAVE - 1);
  const int wv = t / WAVE;
  const i64 w = blockIdx.x;  // (XCD-ordered presorted windows measured slower: 1.241 -> 1.269 ms, profiles/r03_p)
  // the plan already failed (k_khist saw a timestamp group no window holds, or an
  // earlier window overflowed): leave before any load; a scalar read, in flight with
  // the window bounds' (a stale 0 only defers the exit to the check after the loads)
  if (P.meta->f_fail) return;
  const i64 a0 = P.bnd[2 * w], b0 = P.bnd[2 * w + 1];
  const int na = (int)(P.bnd[2 * w + 2] - a0);
  const int nb = (int)(P.bnd[2 * w + 3] - b0);
  const int sz = na + nb;
  if (na < 0 || nb < 0 || sz > CAP) {  // the presorted plan does not hold
    // bit 0: branch logs not timestamp-ordered; bit 1: window too large for LDS;
    // bit 2: ... and it holds one timestamp only, so smaller windows cannot help
    if (threadIdx.x == 0) {
      u64 f = 1;
      if (na >= 0 && nb >= 0) {
        const u64* A = P.kts + a0;
        const u64* B = P.kts + P.na + P.bgap + b0;
        const u64 v = na ? A[0] : B[0];
        const bool one = (!na || (A[0] == v && A[na - 1] == v)) && (!nb || (B[0] == v && B[nb - 1] == v));
        f = one ? 6 : 2;
      }
      atomicOr((unsigned long long*)&P.meta->f_fail, (unsigned long long)f);
    }
    return;
  }
  const i64 bpos = P.na + b0 - na;  // op index of B element e is bpos + e
  const i64 bld = bpos + P.bgap;    // ... stored at field index bld + e
  WSTAMP(0);

  // 1. load the sort keys (kind, timestamp, top of the id) and the payload
  u32 hi_r[ITEMS];  // the top 32 bits of oid_hi: the rank key (only they are loaded)
  u32 sym_r[ITEMS];
  i32 v0_r[ITEMS], v1_r[ITEMS];
  u32 k_r[ITEMS];
  bool bad = false;
  // every global read of the window is issued here, before any loaded value is used:
  // the load phase is one round trip to memory, and the later phases find their
  // operands in registers (no dependent global reads between barriers).  The few side
  // reads go first, so that their address arithmetic never waits on the bulk loads.
  // kinds of the <= 255 ops between each branch's chunk start and the window start
  // (window offsets below); entries 0..255 branch A, 256..511 branch B
  u32 kpart[KP];
#pragma unroll
  for (int u = 0; u < KP; ++u) {
    const int x = t + NT * u;
    const int pa = (int)(a0 % CH), pb = (int)(b0 % CH);
    const int side = x >= CH;
    const int q = x - side * CH;
    kpart[u] = 0xffffffffu;
    if (x < 2 * CH && q < (side ? pb : pa)) kpart[u] = P.kind[side ? (P.na + P.bgap + b0 - pb + q) : (a0 - pa + q)];
  }
  // timestamps just before the window on each branch
  u64 prev_a = 0, prev_b = 0;
  if (t == 0 && a0 > 0) prev_a = P.kts[a0 - 1];
  if (t == 0 && b0 > 0) prev_b = P.kts[P.na + P.bgap + b0 - 1];
  // T-order segment starts; window offsets = chunk prefix at the window start + kinds
  // of the <= 255 ops between that chunk start and the window start (per branch)
  const u64 base_v = t <= SMX_N_KINDS ? P.meta->base[t] : 0ull;
  const u32 kmask_r = P.meta->kmask[0] | P.meta->kmask[1];
  // a window that already failed the plan (dense groups: every window does) makes the
  // rest of the launch pointless: checked after the load phase, no extra round trip
  const u64 failed = t == 0 ? P.meta->f_fail : 0ull;
  u32 woff_x = 0, woff_y = 0;  // (added where stored: an add here would wait for every load)
  // (32-bit chunk indices: 2 * kinds * CM < 2^32 for any n < 2^31, the i32 output limit)
  if (t < SMX_N_KINDS) {
    woff_x = P.cpre[(u32)t * (u32)P.CM + (u32)(a0 / CH)];
    woff_y = P.cpre[(u32)(SMX_N_KINDS + t) * (u32)P.CM + (u32)(b0 / CH)];
  } else if (t < SMX_N_KINDS + 2) {
    const int sd = t - SMX_N_KINDS;
    woff_x = P.cpre[(u32)(sd * SMX_N_KINDS + KREN) * (u32)P.CM + (u32)((sd ? b0 : a0) / CH)];
  }
  // value widths published so far (a stale read only costs a redundant atomicOr)
  u32 vcur[3] = {0u, 0u, 0u};
  if (t == 0) {
#pragma unroll
    for (int q = 0; q < 3; ++q) vcur[q] = __hip_atomic_load(&P.meta->vbits[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  // all loads are issued unconditionally (clamped to a valid op) so that the
  // loads of a lane are in flight together; the guards apply to the LDS stores only
  u64 ts_r[ITEMS];
  auto op_index = [&](int e) -> i64 {  // (an empty window still writes its exports)
    const int ec = e < sz ? e : 0;
    return sz == 0 ? 0 : (ec < na ? a0 + ec : bld + ec);
  };
#pragma unroll
  for (int i = 0; i < ITEMS; ++i) {
    const i64 j = op_index(t + NT * i);
    k_r[i] = P.kind[j];
    ts_r[i] = P.kts[j];
    hi_r[i] = reinterpret_cast<const u32*>(P.khi)[2 * j + 1];
    sym_r[i] = P.sym[j];
    v0_r[i] = P.v0[j];
    v1_r[i] = P.v1[j];
  }
  u32 none_mv = 0;  // moves with a None value (prefix fix-up)
  u32 vb_a = 0, vb_f = 0, vb_c = 0;  // OR of (value + 1): widths of the packed final-state table
  // branch-free: the LDS slots past sz take harmless values (every later phase reads
  // slots < sz only), the rest is selects -- no exec-mask bookkeeping per item
  static_assert(NT * ITEMS <= CAP, "item slots inside the LDS arrays");
#pragma unroll
  for (int i = 0; i < ITEMS; ++i) {
    const int e = t + NT * i;
    const bool ok = e < sz;
    const u32 kr = k_r[i];
    bad |= ok & ((kr >= SMX_N_KINDS) | (sym_r[i] >= (u64)P.n_sym));
    const u32 k = kr < SMX_N_KINDS ? kr : SMX_N_KINDS - 1;
    sts[e] = ts_r[i];
    const bool mv = ok & (k == KMOVE), rn = ok & (k == KREN);
    const bool ha = v0_r[i] >= 0, hf = v1_r[i] >= 0;
    sym_r[i] = (sym_r[i] & SYM_MASK) | ((mv & ha) ? MS_HAS_A : 0u) | ((mv & hf) ? MS_HAS_F : 0u);
    none_mv += (mv & !(ha & hf)) ? 1u : 0u;
    vb_a |= mv ? (u32)(v0_r[i] + 1) : 0u;
    vb_f |= mv ? (u32)(v1_r[i] + 1) : 0u;
    vb_c |= rn ? (u32)(v1_r[i] + 1) : 0u;
  }
  vb_a = wave_or_to_last(vb_a);
  vb_f = wave_or_to_last(vb_f);
  vb_c = wave_or_to_last(vb_c);
  if (lane == WAVE - 1) {
    vbw[wv][0] = vb_a;
    vbw[wv][1] = vb_f;
    vbw[wv][2] = vb_c;
  }
  if (bad) P.meta->bad_sym = 1;
  static_assert(OW <= NT, "one occupancy word per thread");
  if (t < OW) occ[t] = 0u;
  {
    typedef u32 __attribute__((ext_vector_type(4))) z4;
    for (int i = t; i < CAP / 4; i += NT) reinterpret_cast<z4*>(bcnt)[i] = z4{0u, 0u, 0u, 0u};
  }
  if (t <= SMX_N_KINDS) base[t] = base_v;
  if (t < SMX_N_KINDS + 2) woffk[t] = woff_x + woff_y;
  if (t == 0) wtot[0] = failed != 0;
  __syncthreads();
  if (wtot[0]) return;  // (wtot is written again in step 10)
  WSTAMP(1);
  if (WF_ABL(16)) {  // diagnostics: load only (keeps every load live)
    u32 x = 0;
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) x += sym_r[i] + (u32)v0_r[i] + (u32)v1_r[i] + (u32)hi_r[i];
    if (x == 0x9e3779b9u) P.meta->dup_key = 1;
    return;
  }
  // window offsets: the partial-chunk kinds
#pragma unroll
  for (int u = 0; u < KP; ++u) {
    if (kpart[u] != 0xffffffffu) {
      const u32 k = kpart[u] < SMX_N_KINDS ? kpart[u] : SMX_N_KINDS - 1;
      atomicAdd(&woffk[k], 1u);
      if (k == KREN) atomicAdd(&woffk[SMX_N_KINDS + (t + NT * u >= CH)], 1u);
    }
  }

  const int nch = (sz + WAVE - 1) / WAVE;
  // steps 2-9: the window's order (the module comment); their LDS views and registers
  // end with the scope
  {
    constexpr int GMAX = 4 * CAP;    // group counters (u16, in sts once the timestamps are dead)
    __shared__ u16 occpre[OW];       // set bits before each occupancy word
    __shared__ u16 lasth[NCH];       // last head at or before the end of each 64-op chunk
    __shared__ u32 rinfo[2];         // groups fit, R
    u32* gcnt = reinterpret_cast<u32*>(sts);             // group counters, two u16 per word
    static_assert(GMAX / 2 * sizeof(u32) <= sizeof(sts), "group counters inside sts");
    u32* mkey = reinterpret_cast<u32*>(sts);             // bucket order: 32-bit keys (after the group starts are dead)
    u16* mel = reinterpret_cast<u16*>(reinterpret_cast<u32*>(sts) + CAP);  // ... and elements
    // 2. run heads, the order check, each head's run position
    bool dec = false;
    if (t == 0) {
      dec = (a0 > 0 && na > 0 && prev_a > sts[0]) || (b0 > 0 && nb > 0 && prev_b > sts[na]);
      win_publish_widths(P.meta, &vbw[0][0], WAVES, vcur);
    }
    u64 hbr[ITEMS];
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
      const int e = t + NT * i;
      const bool valid = e < sz;
      const bool first = e == 0 || e == na;
      const u64 pv = sts[valid && !first ? e - 1 : 0];
      const bool head = valid && (first || pv != ts_r[i]);
      dec |= valid && !first && pv > ts_r[i];
      hbr[i] = __ballot(head);
      // this item's 64-op chunk: wave-uniform, and said so (t / WAVE is a lane value to the
      // compiler, which would then run the head searches below as lane-divergent loops)
      const int c = __builtin_amdgcn_readfirstlane((NT * i) / WAVE + wv);
      if (lane == 0 && c < NCH) gbits[c] = hbr[i];
      // the heads of this chunk, one at a time with the whole wave: a 64-way search of
      // the other part for #{ops < v} (two or three rounds of one LDS read per lane)
      u64 hb = hbr[i];
      while (hb) {
        const int hl = __ffsll((unsigned long long)hb) - 1;
        hb &= hb - 1;
        const int eh = c * WAVE + hl;
        const u64 v = ((u64)(u32)__builtin_amdgcn_readlane((int)(u32)(ts_r[i] >> 32), hl) << 32) |
                      (u64)(u32)__builtin_amdgcn_readlane((int)(u32)ts_r[i], hl);
        const bool sa = eh < na;
        const int o0 = sa ? na : 0, no = sa ? nb : na;
        int lo = 0, len = no;  // answer in [lo, lo + len]; everything before lo is < v
        while (len > 0) {
          const int S = (len + WAVE - 1) / WAVE;
          const int q = lane * S;
          const bool pr = q < len && sts[o0 + lo + (q < len ? q : 0)] < v;
          const int cnt = __popcll(__ballot(pr));
          if (cnt == 0) break;
          const int qp = lo + (cnt - 1) * S;  // the last sample below v
          const int hi = min(qp + S, lo + len);
          lo = qp + 1;
          len = hi - lo;
        }
        const int spos = (sa ? eh : eh - na) + lo;
        if (lane == 0) {
          sp[eh] = (u16)spos;
          atomicOr(&occ[spos >> 5], 1u << (spos & 31));
        }
      }
    }
    if (__syncthreads_or(dec)) {
      if (t == 0) atomicOr((unsigned long long*)&P.meta->f_fail, 1ull);
      return;
    }
    WSTAMP(2);
    WF_EXIT(2);
    // 3. (wave 0) the last head of each chunk, the runs' dense index, the group count
    const u32 kpres = __builtin_amdgcn_readfirstlane(kmask_r);
    const int KD = __popc(kpres);
    const int kbits_r = 32 - __clz((int)(max(KD, 1) - 1));  // bits of a dense kind
    if (wv == 0) {
      static_assert(NCH <= 2 * WAVE && OW <= 4 * WAVE, "one wave covers the chunks and occupancy words");
      u32 carry = 0;  // (last head + 1; 0 = none yet)
#pragma unroll
      for (int c0 = 0; c0 < NCH; c0 += WAVE) {
        const int c = c0 + lane;
        const u64 hw = c < nch ? gbits[c] : 0ull;
        u32 lh = hw ? (u32)(c * WAVE + 63 - __clzll(hw)) + 1u : 0u;
        lh = max(wave_incl_max_u32(lh), carry);
        if (c < NCH) lasth[c] = (u16)(lh ? lh - 1u : 0u);
        carry = (u32)__builtin_amdgcn_readlane((int)lh, WAVE - 1);
      }
      u32 rsum = 0;
#pragma unroll
      for (int w0 = 0; w0 < OW; w0 += WAVE) {
        const int x = w0 + lane;
        const u32 o = x < OW ? occ[x] : 0u;
        const u32 pc = (u32)__popc(o), inc = wave_incl_sum_u32(pc);
        if (x < OW) occpre[x] = (u16)(rsum + inc - pc);
        rsum += (u32)__builtin_amdgcn_readlane((int)inc, WAVE - 1);
      }
      if (lane == 0) {
        rinfo[0] = (u32)KD * rsum <= (u32)GMAX && !(SMX_DIAG && P.ablate == 200);
        rinfo[1] = rsum;
      }
    }
    {  // the group counters (the timestamps are dead: every head has searched)
      typedef u32 __attribute__((ext_vector_type(4))) z4;
      for (int i = t; i < GMAX / 8; i += NT) reinterpret_cast<z4*>(gcnt)[i] = z4{0u, 0u, 0u, 0u};
    }
    __syncthreads();
    if (!rinfo[0]) {  // more (kind, run) groups than counters: smaller windows (f_fail 2)
      if (t == 0) atomicOr((unsigned long long*)&P.meta->f_fail, 2ull);
      return;
    }
    WSTAMP(3);
    WF_EXIT(3);
    {
      const u32 R = rinfo[1];
      // 4. each op's run (its head: in its chunk, else the last head of the earlier
      //    chunks), group g = dense kind * R + run, counted
      const u64 lem = lanemask_lt() | (1ull << lane);
      u32 g_r[ITEMS];
#pragma unroll
      for (int i = 0; i < ITEMS; ++i) {
        const int e = t + NT * i;
        const int c = __builtin_amdgcn_readfirstlane((NT * i) / WAVE + wv);
        const u64 m = hbr[i] & lem;
        const int h = m ? c * WAVE + 63 - __clzll(m) : (int)lasth[c > 0 ? c - 1 : 0];
        const u32 k = k_r[i] < SMX_N_KINDS ? k_r[i] : SMX_N_KINDS - 1;
        g_r[i] = 0xffffffffu;
        u32 r = 0, dk = 0;
        if (e < sz) {
          const u32 s = sp[h];
          r = occpre[s >> 5] + (u32)__popc(occ[s >> 5] & ((1u << (s & 31)) - 1u));
          dk = (u32)__popc(kpres & ((1u << k) - 1u));
          g_r[i] = dk * R + r;
        }
        // the wide windows: a wave inside one run (config 5: one run per window) has at
        // most KD distinct groups, counted per group by its lowest lane (a per-lane LDS
        // atomic on a handful of words serialises: wide window 0.422 -> 0.406 ms on config 5);
        // otherwise, and in the normal windows (many runs, where the test costs more than it
        // saves), one atomic per op
        bool agg = false;
        u32 r0 = 0;
        if constexpr (CAP > WF_CAP) {
          const u64 vm = __ballot(e < sz);
          r0 = (u32)__builtin_amdgcn_readfirstlane((int)r);
          agg = vm && __ballot(e < sz && r - r0 > 0u) == 0;
        }
        if (agg) {
          const u64 peers = wave_peers_n(dk, e < sz, kbits_r);
          if (e < sz && (peers & lanemask_lt()) == 0)
            atomicAdd(&gcnt[g_r[i] >> 1], (u32)__popcll(peers) << (16 * (g_r[i] & 1)));
        } else if (e < sz) {
          atomicAdd(&gcnt[g_r[i] >> 1], 1u << (16 * (g_r[i] & 1)));
        }
      }
      __syncthreads();
      WSTAMP(4);
      WF_EXIT(4);
      // 5. group starts: exclusive scan of the KD * R counters (kind-major = T order), in
      //    passes of 4 * NT counters (one pass on config 3's windows: 6 kinds x 14 runs)
      const int GS = KD * (int)R;
      {
        u32 carry = 0;
        for (int g0 = 0; g0 < GS; g0 += 4 * NT) {  // (block-uniform)
          const int x = g0 / 2 + 2 * t;  // words x, x + 1: counters 2x .. 2x + 3
          const u32 w0 = 2 * x < GS ? gcnt[x] : 0u, w1 = 2 * x + 2 < GS ? gcnt[x + 1] : 0u;
          const u32 c0 = w0 & 0xffffu, c1 = w0 >> 16, c2 = w1 & 0xffffu, c3 = w1 >> 16;
          u32 tot;
          const u32 run = carry + block_excl_scan<OpSum, u32, WAVES>(c0 + c1 + c2 + c3, &vbw[0][0], &tot);
          if (2 * x < GS) gcnt[x] = run | ((run + c0) << 16);
          if (2 * x + 2 < GS) gcnt[x + 1] = (run + c0 + c1) | ((run + c0 + c1 + c2) << 16);
          carry += tot;
        }
      }
      __syncthreads();
      auto gstart = [&](int g) -> u32 {
        return g < GS ? (gcnt[g >> 1] >> (16 * (g & 1))) & 0xffffu : (u32)sz;
      };
      // kinds: window-local start and count (kind k's groups are d(k) * R .. + R)
      if (t <= SMX_N_KINDS) {
        u32 s = (u32)sz, e = (u32)sz;
        if (t < SMX_N_KINDS) {
          const int d = __popc(kpres & ((1u << t) - 1u));
          s = R ? gstart(d * (int)R) : 0u;
          e = ((kpres >> t) & 1u) && R ? gstart((d + 1) * (int)R) : s;
          wck[t] = e - s;
        }
        kbase[t] = s;
      }
      WSTAMP(5);
      WF_EXIT(5);
      // 6. interpolation bucket inside the group: b = gs + (ge - gs) * key / 2^32
      u32 b_r[ITEMS], ar_r[ITEMS];
#pragma unroll
      for (int i = 0; i < ITEMS; ++i) {
        b_r[i] = 0xffffffffu;
        ar_r[i] = 0u;
        if (g_r[i] == 0xffffffffu) continue;
        const u32 gs = gstart((int)g_r[i]), ge = gstart((int)g_r[i] + 1);
        const u32 b = gs + (u32)(((u64)(ge - gs) * hi_r[i]) >> 32);
        b_r[i] = b;
        ar_r[i] = atomicAdd(&bcnt[b], 1u);
      }
      __syncthreads();
      WSTAMP(6);
      WF_EXIT(6);
      // 7. bucket starts
      {
        constexpr int WPT = CAP / NT;
        u32 cw[WPT], sum = 0;
#pragma unroll
        for (int i = 0; i < WPT; ++i) {
          cw[i] = bcnt[WPT * t + i];
          sum += cw[i];
        }
        u32 tot;
        u32 run = block_excl_scan<OpSum, u32, WAVES>(sum, &vbw[0][0], &tot);
#pragma unroll
        for (int i = 0; i < WPT; ++i) {
          bcnt[WPT * t + i] = run;
          run += cw[i];
        }
      }
      __syncthreads();
      auto bstart = [&](u32 b) -> u32 { return b < (u32)CAP ? bcnt[b] : (u32)sz; };
      WSTAMP(7);
      WF_EXIT(7);
      // 8. members in bucket order: key and element
      u32 slot_r[ITEMS];
#pragma unroll
      for (int i = 0; i < ITEMS; ++i) {
        slot_r[i] = 0u;
        if (b_r[i] == 0xffffffffu) continue;
        const u32 s = bstart(b_r[i]) + ar_r[i];
        slot_r[i] = s;
        mkey[s] = hi_r[i];
        mel[s] = (u16)(t + NT * i);
      }
      __syncthreads();
      WSTAMP(8);
      WF_EXIT(8);
      // 9. rank inside the bucket on (key, full id, side, index); the final order
      //    (per-lane loops: one op per bucket on average; a wave-uniform loop over the
      //    ITEMS buckets together spilled registers)
#pragma unroll
      for (int i = 0; i < ITEMS; ++i) {
        const u32 b = b_r[i];
        if (b == 0xffffffffu) continue;
        const int e = t + NT * i;
        const u32 b1 = b + 1 < (u32)CAP ? b + 1 : (u32)CAP - 1;  // (branch-free bucket bounds)
        const u32 lo = slot_r[i] - ar_r[i];  // (the bucket's start: this op's slot less its arrival rank)
        const u32 hw = bcnt[b1];
        const u32 hi = b + 1 < (u32)CAP ? hw : (u32)sz, kp = hi_r[i];
        u32 c = 0;
        bool tie = false;
#pragma unroll 1
        for (u32 q = lo; q < hi; ++q) {  // (own slot: x == kp, not a tie)
          const u32 x = mkey[q];
          c += x < kp;
          tie |= (x == kp) & (q != slot_r[i]);
        }
        if (tie) {  // equal top 32 bits (rare): the full ids, then element order = (side, index)
          c = 0;
          const i64 jm = e < na ? a0 + e : bld + e;
          const u64 hm = P.khi[jm], lm = P.klo[jm];
#pragma unroll 1
          for (u32 q = lo; q < hi; ++q) {
            const u32 x = mkey[q];
            if (x != kp || q == slot_r[i]) {
              c += x < kp;
              continue;
            }
            const int eo = mel[q];
            const i64 jo = eo < na ? a0 + eo : bld + eo;
            const u64 ho = P.khi[jo], lo2 = P.klo[jo];
            c += ho < hm || (ho == hm && (lo2 < lm || (lo2 == lm && eo < e)));
          }
        }
        const u32 f = lo + c;
        sord[f] = (u16)e;
        inv[e] = (u16)f;
        skS[f] = (u8)(k_r[i] < SMX_N_KINDS ? k_r[i] : SMX_N_KINDS - 1);
      }
      __syncthreads();
      WSTAMP(9);
      WF_EXIT(9);
    }
  }
  // 10. renames: rank among the window's renames of the same branch (final order), the
  //     renames per branch of each 64 (rc) and, on wave 0, rc's exclusive scan.  (rown
  //     takes the bucket counters' place: step 9 read them last, before its barrier.)
  const int R0 = kbase[KREN], RN = wck[KREN];
  const int nrc = (RN + WAVE - 1) / WAVE;
  for (int c = wv; c < nrc; c += WAVES) {
    const int x = c * WAVE + lane;
    const bool valid = x < RN;
    const int e = valid ? sord[R0 + x] : 0;
    const bool sb = valid && e >= na;
    const u64 bm = __ballot(sb), vm = __ballot(valid);
    const u64 lt = lanemask_lt();
    if (valid) rown[x] = (u16)(sb ? __popcll(bm & lt) : __popcll(vm & ~bm & lt));
    if (lane == 0) {
      rc[c][0] = (u16)__popcll(vm & ~bm);
      rc[c][1] = (u16)__popcll(bm);
    }
  }
  __syncthreads();
  if (wv == 0) {
    u32 c0s = 0, c1s = 0;  // carries over 64-chunk passes
#pragma unroll
    for (int cb0 = 0; cb0 < NCH; cb0 += WAVE) {
      const int c = cb0 + lane;
      const u32 x0 = c < nrc ? rc[c][0] : 0u;
      const u32 x1 = c < nrc ? rc[c][1] : 0u;
      const u32 i0 = wave_incl_sum(x0), i1 = wave_incl_sum(x1);
      if (c < nrc) {
        rc[c][0] = (u16)(c0s + i0 - x0);
        rc[c][1] = (u16)(c1s + i1 - x1);
      }
      c0s += (u32)__builtin_amdgcn_readlane((int)i0, WAVE - 1);
      c1s += (u32)__builtin_amdgcn_readlane((int)i1, WAVE - 1);
    }
    if (lane == WAVE - 1) {
      wtot[0] = c0s;
      wtot[1] = c1s;
    }
  }
  if (none_mv) atomicAdd((unsigned long long*)&P.meta->n_move_none, (unsigned long long)none_mv);
  __syncthreads();
  WSTAMP(10);
  WF_EXIT(10);

  // 11. payload by element, round 1: sym (| the move's has-value bits) and v0; the
  //     position of each rename in its branch's list (posl)
  if (WF_ABL(4)) return;
  u32* st_a = (u32*)sts;             // [CAP] sym | flags
  i32* st_b = (i32*)sts + CAP;   // [CAP] v0, then v1
  u16* posl = sp;                    // (the run positions are dead since step 4)
  // by final slot: each element's owner stores its payload at inv[element]
  int xi[ITEMS];
#pragma unroll
  for (int i = 0; i < ITEMS; ++i) {
    const int e = t + NT * i;
    xi[i] = e < sz ? inv[e] : CAP;
    if (e < sz) {
      st_a[xi[i]] = sym_r[i];
      if (k_r[i] <= KREN) st_b[xi[i]] = v0_r[i];  // (moves and renames only: the other kinds output neither v0 nor v1)
    }
  }
  if (t < SMX_N_KINDS) tbase[t] = base[t] + woffk[t] - kbase[t];
  const int cntA = wtot[0], cntB = wtot[1];
  for (int x = t; x < RN; x += NT) {
    const int e = sord[R0 + x];
    const int s = e >= na;
    posl[(s ? cntA : 0) + rc[x >> 6][s] + rown[x]] = (u16)x;
  }
  if (t == 0) {
    P.wren[2 * w] = woffk[KREN];
    P.wren[2 * w + 1] = woffk[CNT_REN_A];
  }
  __syncthreads();
  WSTAMP(11);
  WF_EXIT(11);
  // 12. natural-head DivergentRename flags -> candidate slots; window exports
  win_rename_flags<NT, NCH>(
      P, w, woffk[KREN], RN, cntA, cntB, posl, gbits,
      [&](int x, int* s, int* own) {
        const int e = sord[R0 + x];
        *s = e >= na;
        *own = rc[x >> 6][*s] + rown[x];
      },
      [&](int x) -> uint2 {
        return make_uint2(st_a[R0 + x] & SYM_MASK, (u32)st_b[R0 + x]);
      });
  WSTAMP(12);
  WF_EXIT(12);

  // 13. T-ordered records in final order (consecutive lanes -> consecutive T inside
  //     each kind: coalesced)
  const u64 nall = (u64)(P.na + P.nb);
  const u64 nmv = base[KREN];
  // four consecutive slots per thread (CAP = 4 * NT): one LDS read of each array,
  // and when the four share a kind (kinds are contiguous slot ranges) one 16-byte
  // store per output array
  // (CAP = 4 * NT * OP: OP passes of four slots per thread)
  constexpr int OP = CAP / (4 * NT);
  static_assert(CAP == 4 * NT * OP, "four slots per thread and pass");
  auto gsrc = [&](i32 j) -> i32 {
    return MAP ? P.src_map[j] : (j < P.na ? (i32)(P.src_a + j) : (i32)(P.src_b + (j - P.na)));
  };
  u32 k4[OP][4];
  u64 T4[OP][4];
  bool uni[OP];
#pragma unroll
  for (int ps = 0; ps < OP; ++ps) {
    const int x0 = 4 * (t + NT * ps);
    const int m4 = sz - x0 < 4 ? sz - x0 : 4;
    uni[ps] = false;
    if (m4 <= 0) continue;
    const uint2 ew = *reinterpret_cast<const uint2*>(&sord[x0]);
    const u32 kw = *reinterpret_cast<const u32*>(&skS[x0]);
    const uint4 av = *reinterpret_cast<const uint4*>(&st_a[x0]);
    const uint4 bv = *reinterpret_cast<const uint4*>(&st_b[x0]);
    const u32 ee[4] = {ew.x & 0xffffu, ew.x >> 16, ew.y & 0xffffu, ew.y >> 16};
    const u32 aa[4] = {av.x, av.y, av.z, av.w};
    const i32 bb[4] = {(i32)bv.x, (i32)bv.y, (i32)bv.z, (i32)bv.w};
    i32 j4[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      u32 k = (kw >> (8 * u)) & 0xffu;
      k = k < SMX_N_KINDS ? k : 0u;  // (slots past sz)
      k4[ps][u] = k;
      T4[ps][u] = tbase[k] + (u64)(x0 + u);
      j4[u] = (i32)(ee[u] < (u32)na ? a0 + ee[u] : bpos + ee[u]);
    }
    uni[ps] = m4 == 4 && k4[ps][3] == k4[ps][0] && T4[ps][0] + 3 < nall;
    if (uni[ps]) {
      const u64 T = T4[ps][0];
      if (k4[ps][0] == KMOVE) {
        st4(P.out_order + T, gsrc(j4[0]), gsrc(j4[1]), gsrc(j4[2]), gsrc(j4[3]));
        st4(P.out_addr + T, bb[0], bb[1], bb[2], bb[3]);
        st4(P.out_ctx + T, -1, -1, -1, -1);
        st4((i32*)P.msym + T, (i32)aa[0], (i32)aa[1], (i32)aa[2], (i32)aa[3]);
      } else {
        st4(P.tsrc + (T - nmv), j4[0], j4[1], j4[2], j4[3]);
        st4((i32*)P.tsym + (T - nmv), (i32)(aa[0] & SYM_MASK), (i32)(aa[1] & SYM_MASK), (i32)(aa[2] & SYM_MASK),
            (i32)(aa[3] & SYM_MASK));
      }
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const u64 T = T4[ps][u];
        if (u >= m4 || T >= nall) continue;  // (T >= nall: only a failed, discarded plan)
        if (k4[ps][u] == KMOVE) {
          P.out_order[T] = gsrc(j4[u]);
          P.out_addr[T] = bb[u];
          P.out_ctx[T] = -1;
          P.msym[T] = aa[u];
        } else {
          P.tsrc[T - nmv] = j4[u];
          P.tsym[T - nmv] = aa[u] & SYM_MASK;
        }
      }
    }
  }
  __syncthreads();
  WSTAMP(13);
  WF_EXIT(13);
  // 14. round 2: v1 -> the move's newFile, the rename's chain value
#pragma unroll
  for (int i = 0; i < ITEMS; ++i)
    if (xi[i] < CAP && k_r[i] <= KREN) st_b[xi[i]] = v1_r[i];
  __syncthreads();
#pragma unroll
  for (int ps = 0; ps < OP; ++ps) {
    const int x0 = 4 * (t + NT * ps);
    const int m4 = sz - x0 < 4 ? sz - x0 : 4;
    if (m4 <= 0 || (k4[ps][0] > KREN && k4[ps][m4 - 1] > KREN)) continue;
    const uint4 bv = *reinterpret_cast<const uint4*>(&st_b[x0]);
    const i32 bb[4] = {(i32)bv.x, (i32)bv.y, (i32)bv.z, (i32)bv.w};
    if (uni[ps]) {
      const u64 T = T4[ps][0];
      st4(k4[ps][0] == KMOVE ? P.out_file + T : P.Rstr + (T - nmv), bb[0], bb[1], bb[2], bb[3]);
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const u64 T = T4[ps][u];
        if (u >= m4 || T >= nall || k4[ps][u] > KREN) continue;
        if (k4[ps][u] == KMOVE) P.out_file[T] = bb[u];
        else P.Rstr[T - nmv] = bb[u];
      }
    }
  }
  if (DBG) {
    __syncthreads();
    WSTAMP(14);
  }
}

// ---------------------------------------------------------------------------
// generic windows: branch logs pre-sorted by (timestamp, oid); fixed diagonals

__device__ __forceinline__ bool key_le(u64 ta, u64 ha, u64 la, u64 tb, u64 hb, u64 lb) {
  if (ta != tb) return ta < tb;
  if (ha != hb) return ha < hb;
  return la <= lb;
}

// 1024-op windows on 512 threads: 38 KB of LDS, four windows per CU (2048-op windows
// took 75 KB, two per CU; config 5 window stage 0.80 -> 0.61 ms, profiles/r02_i)
#ifndef WG_CAP
#define WG_CAP 1024                 // ops per generic window (fixed diagonals, k_gpart)
#endif
#ifndef WG_NT
#define WG_NT 512
#endif
#define WG_ITEMS (WG_CAP / WG_NT)
#define WG_NCH (WG_CAP / WAVE)

__global__ void __launch_bounds__(WG_NT) k_window_g(WinArgs P) {
  __shared__ u64 sts[WG_CAP];
  __shared__ u64 shi[WG_CAP];
  __shared__ u64 slo[WG_CAP];
  __shared__ u32 ssrc[WG_CAP];
  __shared__ u16 sord[WG_CAP];       // merge order, later posl
  __shared__ u16 fin[WG_CAP];
  __shared__ u16 rown[WG_CAP];
  __shared__ u8 skind[WG_CAP];
  __shared__ u8 srank[WG_CAP];
  __shared__ u16 ccnt[WG_NCH][SMX_N_KINDS];
  __shared__ u16 rc[WG_NCH][2];
  __shared__ u32 kbase[SMX_N_KINDS + 1];
  __shared__ u32 wck[SMX_N_KINDS];
  __shared__ u64 base[SMX_N_KINDS + 1];
  __shared__ u64 cb[WG_NCH];
  __shared__ u32 wtot[2];
  __shared__ u32 vbw[WG_NT / WAVE][3];
  __shared__ u32 woffk[NCNT];
  // after the merge the id words are dead: the payload by element takes their place
  u32* st_sym = reinterpret_cast<u32*>(shi);
  i32* st_v0 = reinterpret_cast<i32*>(shi) + WG_CAP;
  i32* st_v1 = reinterpret_cast<i32*>(slo);

  const int t = threadIdx.x;
  const int lane = t & (WAVE - 1);
  const int wv = t / WAVE;
  // consecutive windows on one XCD: a timestamp group spans several windows, whose
  // gathers through the permutation then hit the same L2
  const i64 w = xcd_item(blockIdx.x, P.W);
  if (P.meta->f_fail) return;  // the segmented sort failed: no permutation to gather through
  const i64 a0 = P.bnd[2 * w], b0 = P.bnd[2 * w + 1];
  const int na = (int)(P.bnd[2 * w + 2] - a0);
  const int nb = (int)(P.bnd[2 * w + 3] - b0);
  const int sz = na + nb;

  // loads: the sorted keys and the permutation, then the op fields through it (two
  // round trips, every item's loads in flight together; the payload stays in registers
  // until the merge is done)
  bool bad = false;
  u32 vb_a = 0, vb_f = 0, vb_c = 0;
  u32 src_r[WG_ITEMS], k_r[WG_ITEMS], sym_r[WG_ITEMS];
  i32 v0_r[WG_ITEMS], v1_r[WG_ITEMS];
  u64 kt_r[WG_ITEMS], kh_r[WG_ITEMS], kl_r[WG_ITEMS];
#pragma unroll
  for (int i = 0; i < WG_ITEMS; ++i) {
    const int e = t + WG_NT * i;
    const int ec = e < sz ? e : 0;
    const i64 j = sz == 0 ? 0 : (ec < na ? a0 + ec : P.na + b0 + (ec - na));
    src_r[i] = P.perm[j];
    kt_r[i] = P.kts[j];
    kh_r[i] = P.khi[j];
    kl_r[i] = P.klo[j];
  }
  if (t < NCNT) woffk[t] = P.woff[(i64)t * P.W + w];
#pragma unroll
  for (int i = 0; i < WG_ITEMS; ++i) {
    const u32 src = src_r[i];
    k_r[i] = P.kind[src];
    sym_r[i] = P.sym[src];
    v0_r[i] = P.v0[src];
    v1_r[i] = P.v1[src];
  }
#pragma unroll
  for (int i = 0; i < WG_ITEMS; ++i) {
    const int e = t + WG_NT * i;
    if (e >= sz) continue;
    sts[e] = kt_r[i];
    shi[e] = kh_r[i];
    slo[e] = kl_r[i];
    ssrc[e] = src_r[i];
    const u32 k = k_r[i];
    bad |= (k >= SMX_N_KINDS) || (sym_r[i] >= (u64)P.n_sym);
    skind[e] = (u8)(k < SMX_N_KINDS ? k : SMX_N_KINDS - 1);
    if (k == KMOVE) {
      vb_a |= (u32)(v0_r[i] + 1);
      vb_f |= (u32)(v1_r[i] + 1);
    } else if (k == KREN) {
      vb_c |= (u32)(v1_r[i] + 1);
    }
  }
  vb_a = wave_or_to_last(vb_a);
  vb_f = wave_or_to_last(vb_f);
  vb_c = wave_or_to_last(vb_c);
  if (lane == WAVE - 1) {
    vbw[wv][0] = vb_a;
    vbw[wv][1] = vb_f;
    vbw[wv][2] = vb_c;
  }
  if (bad) P.meta->bad_sym = 1;
  for (int i = t; i < WG_NCH * SMX_N_KINDS; i += WG_NT) (&ccnt[0][0])[i] = 0;
  if (t <= SMX_N_KINDS) base[t] = P.meta->base[t];
  __syncthreads();

  if (t == 0) win_publish_widths(P.meta, &vbw[0][0], WG_NT / WAVE);
  if (sz > 0) {
    const int d0 = t * WG_ITEMS < sz ? t * WG_ITEMS : sz;
    const int d1 = d0 + WG_ITEMS < sz ? d0 + WG_ITEMS : sz;
    int lo = d0 - nb > 0 ? d0 - nb : 0, hi = d0 < na ? d0 : na;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      const int j = na + d0 - 1 - mid;
      if (key_le(sts[mid], shi[mid], slo[mid], sts[j], shi[j], slo[j])) lo = mid + 1;
      else hi = mid;
    }
    int ia = lo, ib = d0 - lo;
    for (int d = d0; d < d1; ++d) {
      bool take_a;
      if (ia >= na) take_a = false;
      else if (ib >= nb) take_a = true;
      else {
        const int j = na + ib;
        take_a = key_le(sts[ia], shi[ia], slo[ia], sts[j], shi[j], slo[j]);
      }
      sord[d] = (u16)(take_a ? ia++ : na + ib++);
    }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < WG_ITEMS; ++i) {  // (visible after the multisplit's barriers)
    const int e = t + WG_NT * i;
    if (e < sz) {
      st_sym[e] = sym_r[i];
      st_v0[e] = v0_r[i];
      st_v1[e] = v1_r[i];
    }
  }

  const int nch = (sz + WAVE - 1) / WAVE;
  for (int c = wv; c < nch; c += WG_NT / WAVE) {
    const int m = c * WAVE + lane;
    const bool valid = m < sz;
    const int e = valid ? sord[m] : 0;
    const u32 k = valid ? skind[e] : 0u;
    const u64 peers = wave_peers<5>(k, valid);
    const u32 r = __popcll(peers & lanemask_lt());
    if (valid) {
      srank[m] = (u8)r;
      if (r == 0) ccnt[c][k] = (u16)__popcll(peers);
    }
  }
  __syncthreads();
  for (int k = wv; k < SMX_N_KINDS; k += WG_NT / WAVE) {
    const u32 x = lane < nch ? ccnt[lane][k] : 0u;
    const u32 inc = wave_incl_sum(x);
    if (lane < nch) ccnt[lane][k] = (u16)(inc - x);
    if (lane == WAVE - 1) wck[k] = inc;
  }
  __syncthreads();
  if (wv == 0) {
    const u32 x = lane < SMX_N_KINDS ? wck[lane] : 0u;
    const u32 inc = wave_incl_sum(x);
    if (lane < SMX_N_KINDS) kbase[lane] = inc - x;
    if (lane == SMX_N_KINDS - 1) kbase[SMX_N_KINDS] = inc;
  }
  __syncthreads();
  for (int m = t; m < sz; m += WG_NT) {
    const int e = sord[m];
    const u32 k = skind[e];
    fin[kbase[k] + ccnt[m / WAVE][k] + srank[m]] = (u16)e;
  }
  __syncthreads();

  const int R0 = kbase[KREN], RN = wck[KREN];
  const int nrc = (RN + WAVE - 1) / WAVE;
  for (int c = wv; c < nrc; c += WG_NT / WAVE) {
    const int x = c * WAVE + lane;
    const bool valid = x < RN;
    const int e = valid ? fin[R0 + x] : 0;
    const bool sb = valid && e >= na;
    const u64 bm = __ballot(sb), vm = __ballot(valid);
    const u64 lt = lanemask_lt();
    if (valid) rown[x] = (u16)(sb ? __popcll(bm & lt) : __popcll(vm & ~bm & lt));
    if (lane == 0) {
      rc[c][0] = (u16)__popcll(vm & ~bm);
      rc[c][1] = (u16)__popcll(bm);
    }
  }
  __syncthreads();
  if (wv == 0) {
    const u32 x0 = lane < nrc ? rc[lane][0] : 0u;
    const u32 x1 = lane < nrc ? rc[lane][1] : 0u;
    const u32 i0 = wave_incl_sum(x0), i1 = wave_incl_sum(x1);
    if (lane < nrc) {
      rc[lane][0] = (u16)(i0 - x0);
      rc[lane][1] = (u16)(i1 - x1);
    }
    if (lane == WAVE - 1) {
      wtot[0] = i0;
      wtot[1] = i1;
    }
  }
  __syncthreads();
  const int cntA = wtot[0], cntB = wtot[1];
  u16* posl = sord;
  for (int x = t; x < RN; x += WG_NT) {
    const int e = fin[R0 + x];
    const int s = e >= na;
    posl[(s ? cntA : 0) + rc[x >> 6][s] + rown[x]] = (u16)x;
  }
  if (t == 0) {
    P.wren[2 * w] = woffk[KREN];
    P.wren[2 * w + 1] = woffk[CNT_REN_A];
  }
  __syncthreads();
  win_rename_flags<WG_NT, WG_NCH>(
      P, w, woffk[KREN], RN, cntA, cntB, posl, cb,
      [&](int x, int* s, int* own) {
        const int e = fin[R0 + x];
        *s = e >= na;
        *own = rc[x >> 6][*s] + rown[x];
      },
      [&](int x) -> uint2 {
        const int e = fin[R0 + x];
        return make_uint2(st_sym[e], (u32)st_v0[e]);
      });

  const u64 nall = (u64)(P.na + P.nb);
  const u64 nmv = base[KREN];
  for (int x = t; x < sz; x += WG_NT) {
    const int e = fin[x];
    const u32 k = skind[e];
    const u32 src = ssrc[e];
    const u64 T = base[k] + woffk[k] + (u32)(x - kbase[k]);
    if (T >= nall) continue;
    const u32 s = st_sym[e];
    if (k == KMOVE) {
      const i32 a = st_v0[e], f = st_v1[e];
      P.out_order[T] = win_gsrc(P, src);
      P.out_addr[T] = a;
      P.out_file[T] = f;
      P.out_ctx[T] = -1;
      P.msym[T] = (s & SYM_MASK) | (a >= 0 ? MS_HAS_A : 0u) | (f >= 0 ? MS_HAS_F : 0u);
    } else {
      P.tsrc[T - nmv] = (i32)src;
      P.tsym[T - nmv] = s;
      if (k == KREN) P.Rstr[T - nmv] = st_v1[e];
    }
  }
}
