// smx_emit.h -- the output kernels of a merge: k_emit / k_emit4 write every op after the
// move block, k_mv_init / k_mv_fix the None-value moves' prefix.
// Part of the smx_compose.hip unit: included once, there.
#pragma once

struct EmitArgs {
  const i32* tsrc;     // P = T - nMv: local source op (renames first, then the rest)
  const u32* tsym;
  const u64* skipbits; // renames skipped by the walk
  const u32* skiplist; // ... as a sorted list
  const int4* fin;
  const ComposeMeta* meta;
  u64 n;
  u32 smax;
  int allow_pack;  // the final-state table came from k_tb_reduce (packs when widths fit)
  u64 na_loc;      // local op j -> global j < na_loc ? src_a + j : src_b + j - na_loc
  i64 src_a, src_b;
  const i32* src_map;  // or, for a sample-sorted shard, src_map[j]
  i32* out_order;
  i32* out_addr;
  i32* out_file;
  i32* out_ctx;
  i64* counts;
  int status_none;  // report pending None-value moves (single merge) in counts[0]
  u64* hrec;        // or null: the synchronous call's verdict word (EarlyVerdict)
  u64 hseq;
};

// Streams read once and outputs written once: non-temporal, so that they do not evict
// the gathered final-state table from L2 (k_emit4's aligned 16-byte stores; plain ones
// measured emit 0.753 -> 0.821 ms on config 3, profiles/r06/ab_c3_emit_stores.txt).  A
// wave's outputs are an aligned range, so no line is shared between waves; the partial
// stores at the range's ends are plain (round 2 measured non-temporal partial-line
// stores 1.4-1.8x slower than plain ones, when ranges were not aligned).
#define NTLD(p) __builtin_nontemporal_load(p)
#define NTST(v, p) __builtin_nontemporal_store((v), (p))
#ifndef EMIT_WT
#define EMIT_WT 1024  // positions per wave (2048: emit 0.753 -> 0.749 ms, within noise, profiles/r06/ab_c3_emit_stores.txt)
#endif
#ifndef EMIT_B
#define EMIT_B 8      // wave steps whose loads are issued together
#endif
static_assert(EMIT_WT % (WAVE * EMIT_B) == 0, "a wave's output range is whole batches of steps");

// Every op after the move block (the moves' records came from the window
// kernel).  Each wave owns EMIT_WT consecutive OUTPUT indices (aligned: no output
// line is shared between waves); output o holds the op at position
//   renames  P = o' + #{skips j : S[j] - j <= o'}   (o' = o - nMv, S = sorted skip list)
//   others   P = o' + nskip                          (every skip is a rename)
// found by one binary search per wave and a scalar walk over the (few) skips of
// each 64-output step.  Renames see their symbol's final move state, the rest
// also its last rename (compose.py:30-49).  Block 0 writes the call's counts.
__global__ void __launch_bounds__(BLOCK) k_emit(EmitArgs E) {
  const ComposeMeta* M = E.meta;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    // -1 invalid input (sym >= n_sym or kind >= 18); -2 the plan failed, -3 moves
    // with a None value still need their prefix fix-up (smx_compose_finish)
    const bool bad = M->bad_sym != 0;
    E.counts[0] = bad ? -1 : M->f_fail ? -2 : (M->n_move_none && E.status_none) ? -3 : (i64)(E.n - M->n_skip);
    E.counts[1] = bad ? -1 : (i64)M->n_conf;
    // seq << 1 | 1: smx_compose_finish has work left (or an error) and reads the meta
    if (E.hrec) *E.hrec = E.hseq << 1 | ((bad || M->f_fail || (M->n_move_none && M->kcnt[KMOVE])) ? 1u : 0u);
  }
  if (M->f_fail | M->bad_sym) return;
  const u64 nskip = M->n_skip;
  const u64 nmv = min(M->kcnt[KMOVE], E.n);
  const u64 nP = E.n - nmv;
  const u64 nR = min(M->kcnt[KREN], nP);
  const u64 nout = E.n - nskip, nRk = nR - nskip;
  auto gsrc = [&](i32 j) -> i32 {
    if (E.src_map) return E.src_map[j];
    return (u64)j < E.na_loc ? (i32)(E.src_a + j) : (i32)(E.src_b + ((i64)j - (i64)E.na_loc));
  };
  const FinPack FP = fin_pack_of(M->vbits, E.allow_pack != 0);
  const int lane = threadIdx.x & (WAVE - 1);
  const u64 w0 = (((u64)blockIdx.x * BLOCK + threadIdx.x) / WAVE) * EMIT_WT;  // output index
  if (w0 + EMIT_WT <= nmv || w0 >= nout || nP == 0) return;
  u64 kk = 0;  // skips with S[j] - j below the next step's first rename output
  {
    const u64 o0 = w0 > nmv ? w0 - nmv : 0;
    if (o0 < nRk) {
      u64 lo = 0, hi = nskip;
      while (lo < hi) {
        const u64 mid = (lo + hi) >> 1;
        if ((u64)E.skiplist[mid] - mid < o0) lo = mid + 1;
        else hi = mid;
      }
      kk = lo;
    }
  }
  for (int bt = 0; bt < EMIT_WT / (WAVE * EMIT_B); ++bt) {
    const u64 ob = w0 + (u64)bt * WAVE * EMIT_B;
    if (ob >= nout) break;
    u64 pp[EMIT_B];
#pragma unroll
    for (int j = 0; j < EMIT_B; ++j) {
      const u64 b = ob + (u64)j * WAVE;  // the step's first output (wave-uniform)
      const u64 o = b + lane;
      const u64 op = o >= nmv ? o - nmv : 0;
      const u64 k0 = kk;
      u64 add = 0;
      if (b + WAVE > nmv && (b > nmv ? b - nmv : 0) < nRk) {
        // rename outputs in this step (o' up to b + 63 - nMv): the skips at or below o'
        const u64 ohi = b + WAVE - 1 - nmv;
        while (kk < nskip) {
          const u64 sj = (u64)(u32)__builtin_amdgcn_readfirstlane((int)E.skiplist[kk]) - kk;
          if (sj > ohi) break;
          add += op >= sj;
          ++kk;
        }
      }
      const bool ok = o >= nmv && o < nout;
      pp[j] = !ok ? 0 : (op < nRk ? op + k0 + add : op + nskip);
    }
    i32 src[EMIT_B];
    u32 sy[EMIT_B];
#pragma unroll
    for (int j = 0; j < EMIT_B; ++j) {
      src[j] = NTLD(&E.tsrc[pp[j]]);
      sy[j] = min(NTLD(&E.tsym[pp[j]]), E.smax);
    }
    int4 F[EMIT_B];
    if (FP.packed) {
      u64 x[EMIT_B];
#pragma unroll
      for (int j = 0; j < EMIT_B; ++j) x[j] = fin_word(FP, E.fin, sy[j]);
#pragma unroll
      for (int j = 0; j < EMIT_B; ++j) F[j] = fin_decode(FP, x[j]);
    } else {
#pragma unroll
      for (int j = 0; j < EMIT_B; ++j) F[j] = E.fin[sy[j]];
    }
#pragma unroll
    for (int j = 0; j < EMIT_B; ++j) {
      const u64 o = ob + (u64)j * WAVE + lane;
      if (o >= nmv && o < nout) {
        const bool ren = o - nmv < nRk;
        NTST(gsrc(src[j]), &E.out_order[o]);
        NTST(F[j].x, &E.out_addr[o]);
        NTST(F[j].y, &E.out_file[o]);
        NTST(ren ? -1 : F[j].z, &E.out_ctx[o]);
      }
    }
  }
}

// k_emit with four consecutive outputs per lane: the streams move 16 bytes per lane
// and instruction (the per-lane address work of the texture path is what bounds this
// kernel: a fully divergent 64-lane table gather costs the CU ~150 cycles, a coalesced
// 4-byte stream instruction about as many per byte as a 16-byte one per four).  Each
// wave owns EMIT_WT consecutive output indices; a step is 256 outputs.  Four outputs
// of a lane read four consecutive positions P unless a skipped rename falls between
// them (rare): then each is read on its own.
#define EMIT4_STEPS (EMIT_WT / (4 * WAVE))
typedef u32 ev4u __attribute__((ext_vector_type(4)));
typedef i32 ev4i __attribute__((ext_vector_type(4)));
typedef ev4u __attribute__((aligned(4))) ev4u_a4;
__global__ void __launch_bounds__(BLOCK) k_emit4(EmitArgs E) {
  const ComposeMeta* M = E.meta;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const bool bad = M->bad_sym != 0;
    E.counts[0] = bad ? -1 : M->f_fail ? -2 : (M->n_move_none && E.status_none) ? -3 : (i64)(E.n - M->n_skip);
    E.counts[1] = bad ? -1 : (i64)M->n_conf;
    // seq << 1 | 1: smx_compose_finish has work left (or an error) and reads the meta
    if (E.hrec) *E.hrec = E.hseq << 1 | ((bad || M->f_fail || (M->n_move_none && M->kcnt[KMOVE])) ? 1u : 0u);
  }
  if (M->f_fail | M->bad_sym) return;
  const u64 nskip = M->n_skip;
  const u64 nmv = min(M->kcnt[KMOVE], E.n);
  const u64 nP = E.n - nmv;
  const u64 nR = min(M->kcnt[KREN], nP);
  const u64 nout = E.n - nskip, nRk = nR - nskip;
  auto gsrc = [&](i32 j) -> i32 {
    if (E.src_map) return E.src_map[j];
    return (u64)j < E.na_loc ? (i32)(E.src_a + j) : (i32)(E.src_b + ((i64)j - (i64)E.na_loc));
  };
  const FinPack FP = fin_pack_of(M->vbits, E.allow_pack != 0);
  const int lane = threadIdx.x & (WAVE - 1);
  const u64 w0 = (((u64)blockIdx.x * BLOCK + threadIdx.x) / WAVE) * EMIT_WT;  // output index
  if (w0 + EMIT_WT <= nmv || w0 >= nout || nP == 0) return;
  u64 kk = 0;  // skips with S[j] - j below the next step's first rename output
  {
    const u64 o0 = w0 > nmv ? w0 - nmv : 0;
    if (o0 < nRk) {
      u64 lo = 0, hi = nskip;
      while (lo < hi) {
        const u64 mid = (lo + hi) >> 1;
        if ((u64)E.skiplist[mid] - mid < o0) lo = mid + 1;
        else hi = mid;
      }
      kk = lo;
    }
  }
  u64 pp[EMIT4_STEPS][4];
  bool vec[EMIT4_STEPS];
#pragma unroll
  for (int j = 0; j < EMIT4_STEPS; ++j) {
    const u64 b = w0 + (u64)j * 4 * WAVE;  // the step's first output (wave-uniform)
    const u64 o = b + 4 * (u64)lane;
    u64 add[4] = {0, 0, 0, 0};
    const u64 k0 = kk;
    if (b + 4 * WAVE > nmv && (b > nmv ? b - nmv : 0) < nRk) {
      const u64 ohi = b + 4 * WAVE - 1 - nmv;
      while (kk < nskip) {
        const u64 sj = (u64)(u32)__builtin_amdgcn_readfirstlane((int)E.skiplist[kk]) - kk;
        if (sj > ohi) break;
#pragma unroll
        for (int u = 0; u < 4; ++u) add[u] += (o + u >= nmv ? o + u - nmv : 0) >= sj;
        ++kk;
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const u64 ou = o + u;
      const u64 op = ou >= nmv ? ou - nmv : 0;
      const bool ok = ou >= nmv && ou < nout;
      pp[j][u] = !ok ? 0 : (op < nRk ? op + k0 + add[u] : op + nskip);
    }
    vec[j] = o >= nmv && o + 3 < nout && pp[j][3] == pp[j][0] + 3;
  }
  i32 src[EMIT4_STEPS][4];
  u32 sy[EMIT4_STEPS][4];
#pragma unroll
  for (int j = 0; j < EMIT4_STEPS; ++j) {
    if (vec[j]) {
      const ev4u s4 = __builtin_nontemporal_load(reinterpret_cast<const ev4u_a4*>(&E.tsrc[pp[j][0]]));
      const ev4u y4 = __builtin_nontemporal_load(reinterpret_cast<const ev4u_a4*>(&E.tsym[pp[j][0]]));
      src[j][0] = (i32)s4.x, src[j][1] = (i32)s4.y, src[j][2] = (i32)s4.z, src[j][3] = (i32)s4.w;
      sy[j][0] = y4.x, sy[j][1] = y4.y, sy[j][2] = y4.z, sy[j][3] = y4.w;
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        src[j][u] = NTLD(&E.tsrc[pp[j][u]]);
        sy[j][u] = NTLD(&E.tsym[pp[j][u]]);
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) sy[j][u] = min(sy[j][u], E.smax);
  }
#pragma unroll
  for (int j = 0; j < EMIT4_STEPS; ++j) {
    int4 F[4];
    if (FP.packed) {
      u64 x[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) x[u] = fin_word(FP, E.fin, sy[j][u]);
#pragma unroll
      for (int u = 0; u < 4; ++u) F[u] = fin_decode(FP, x[u]);
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u) F[u] = E.fin[sy[j][u]];
    }
    const u64 o = w0 + (u64)j * 4 * WAVE + 4 * (u64)lane;
    i32 vo[4], va[4], vf[4], vc[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const bool ren = o + u >= nmv && o + u - nmv < nRk;
      vo[u] = gsrc(src[j][u]);
      va[u] = F[u].x;
      vf[u] = F[u].y;
      vc[u] = ren ? -1 : F[u].z;
    }
    if (o >= nmv && o + 3 < nout) {  // o is a multiple of 4: 16-byte aligned stores
      NTST((ev4i{vo[0], vo[1], vo[2], vo[3]}), reinterpret_cast<ev4i*>(&E.out_order[o]));
      NTST((ev4i{va[0], va[1], va[2], va[3]}), reinterpret_cast<ev4i*>(&E.out_addr[o]));
      NTST((ev4i{vf[0], vf[1], vf[2], vf[3]}), reinterpret_cast<ev4i*>(&E.out_file[o]));
      NTST((ev4i{vc[0], vc[1], vc[2], vc[3]}), reinterpret_cast<ev4i*>(&E.out_ctx[o]));
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (o + u >= nmv && o + u < nout) {
          E.out_order[o + u] = vo[u];
          E.out_addr[o + u] = va[u];
          E.out_file[o + u] = vf[u];
          E.out_ctx[o + u] = vc[u];
        }
      }
    }
  }
}

// Moves whose newAddress or newFile is None see the symbol's inclusive prefix
// (compose.py:73-82 + 37-41): moves grouped by symbol in T order, last-non-None
// scan over the moves' own values (out_addr / out_file with msym's has-value bits);
// the composed output index of move T is T.
// Sharded merge: mvpre[2][n_sym] = the symbol's last non-None (addr, file) on the
// lower shards, as (shard + 1) << 32 | (value + 1), 0 = none.
__global__ void k_mv_init(const u32* __restrict__ msym, u64 nMv, u64* __restrict__ keys, u32* __restrict__ vals) {
  for (u64 j = (u64)blockIdx.x * BLOCK + threadIdx.x; j < nMv; j += (u64)gridDim.x * BLOCK) {
    keys[j] = msym[j] & SYM_MASK;
    vals[j] = (u32)j;
  }
}

__global__ void k_mv_fix(const u64* __restrict__ keys, const u32* __restrict__ vals, u64 nMv,
                         const u32* __restrict__ msym, const u64* __restrict__ mvpre, u64 n_sym,
                         i32* __restrict__ out_addr, i32* __restrict__ out_file) {
  for (u64 j = (u64)blockIdx.x * BLOCK + threadIdx.x; j < nMv; j += (u64)gridDim.x * BLOCK) {
    if (j != 0 && keys[j - 1] == keys[j]) continue;
    i32 ra = -1, rf = -1;
    if (mvpre && keys[j] < n_sym) {
      const u64 pa = mvpre[keys[j]], pf = mvpre[n_sym + keys[j]];
      if (pa) ra = (i32)(u32)pa - 1;
      if (pf) rf = (i32)(u32)pf - 1;
    }
    for (u64 i = j; i < nMv && keys[i] == keys[j]; ++i) {
      const u32 T = vals[i];
      const u32 f = msym[T];
      if (f & MS_HAS_A) ra = out_addr[T];
      else out_addr[T] = ra;
      if (f & MS_HAS_F) rf = out_file[T];
      else out_file[T] = rf;
    }
  }
}
