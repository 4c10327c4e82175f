// smx_rga_part.h -- the RGA event record, the stable radix partition of the records by list id
// and the list starts.  Part of the smx_rga.hip unit: included once, there.
#pragma once

// Event record, 2 u64 words, grouped by list by the partition below:
//   w0 = anchor << 32 | t' >> 32   (t' = t with the sign bit flipped: order-preserving)
//   w1 = value << 32 | op << 30 | event index   (index = creation order)
// (anchor, t, author, opid, index) is the crdt.py:48-57 key order; w0 decides it
// unless two events share anchor and the top half of t, and only then are t, author
// and opid read from the input columns by event index (rga_key_lt).
#define RGA_REC 2
struct __attribute__((aligned(16))) R16 {  // one record (16-byte loads / stores)
  u64 a, b;
};
#define RGA_WV 1  // the value / op / index word
#define RGA_IDX_MASK 0x3fffffffu
#define RGA_TOMB_BIT 0x80000000u  // tmp_s: the element is tombstoned (list mode, smx_rga_out.out_tomb)

// Grouping the events by list: a stable radix partition of whole records on the list id,
// 8 bits per pass (one pass up to 256 lists; up to 65536 the high byte here and the low
// byte per bucket in k_rrec_local; beyond, LSD passes of this kernel).  The first
// pass reads the input columns and packs the records; each pass stages a tile in LDS
// in digit order and writes each digit's run of records contiguously, so every byte
// moves in full cache lines.  Stable: each list's events stay in stream order.
#ifndef RR_NT
#define RR_NT 512                         // scatter workgroup (persistent, one per CU)
#endif
#define RR_NW (RR_NT / WAVE)
#ifndef RR_PER_CU
#define RR_PER_CU 2  // persistent scatter workgroups per CU (LDS ~74 KB each)
#endif
#ifndef RREC_ITEMS
#define RREC_ITEMS 6
#endif
#define RREC_TILE (RR_NT * RREC_ITEMS)    // 3072 records (120 KB) per block and pass
#define RREC_SEG (RREC_TILE / RR_NW)      // contiguous records per wave
#define RGA_NDIG 256                      // digits per pass
static_assert(RREC_TILE % BLOCK == 0 && RREC_TILE <= 65535, "tile: k_rrec_hist blocks, u16 slots");

template <bool FIRST>
__global__ void __launch_bounds__(BLOCK) k_rrec_hist(smx_rga_ops o, const u32* __restrict__ keys, int shift,
                                                     u32* __restrict__ hist, i32* __restrict__ err) {
  __shared__ u32 h[RGA_NDIG];
  h[threadIdx.x] = 0;
  __syncthreads();
  const i64 base = (i64)blockIdx.x * RREC_TILE;
  constexpr int IT = RREC_TILE / BLOCK;
  u32 key[IT], bad = 0;  // all loads first: a conditional error store between them would
                         // order each iteration's loads after the previous check
#pragma unroll
  for (int it = 0; it < IT; ++it) {
    const i64 i = base + it * BLOCK + threadIdx.x;
    key[it] = 0;
    if (i < o.n_ops) {
      if constexpr (FIRST) {
        const u32 l = o.list[i];
        // a list id out of range counts as list 0, where k_rrec_scatter places it (an op
        // > 2 fails the call there; its record still goes to its list)
        const bool b = l >= (u64)o.n_lists;
        key[it] = b ? 0u : l;
        bad |= (u32)b;
      } else {
        key[it] = keys[i];
      }
    }
  }
#pragma unroll
  for (int it = 0; it < IT; ++it) {
    const i64 i = base + it * BLOCK + threadIdx.x;
    if (i < o.n_ops) atomicAdd(&h[(key[it] >> shift) & 255u], 1u);
  }
  if (bad) *err = 1;
  __syncthreads();
  hist[(i64)blockIdx.x * RGA_NDIG + threadIdx.x] = h[threadIdx.x];
}

// This thread's share of one tile, loaded into registers: pass 1 the input columns of
// its RREC_ITEMS events, pass 2+ their list ids and RREC_ITEMS * 5 consecutive record
// words of the previous pass (consecutive lanes, consecutive words).
template <bool FIRST>
struct RTile;
template <>
struct RTile<true> {
  u32 list[RREC_ITEMS], value[RREC_ITEMS], anchor[RREC_ITEMS], op[RREC_ITEMS];
  i64 t[RREC_ITEMS];
};
#define RREC_V4 ((RREC_TILE * RGA_REC * 8 / 16 + RR_NT - 1) / RR_NT)  // 16-byte loads per thread
typedef u32 v4u32 __attribute__((ext_vector_type(4)));
template <>
struct RTile<false> {
  u32 key[RREC_ITEMS];
  v4u32 w[RREC_V4];
};

__device__ __forceinline__ i64 rrec_event(i64 base, u32 w, int it, u32 lane) {
  return base + (i64)w * RREC_SEG + it * WAVE + lane;
}

template <bool FIRST>
__device__ __forceinline__ void rrec_load(RTile<FIRST>& T, const smx_rga_ops& o, const u32* __restrict__ kin,
                                          const u64* __restrict__ rin, i64 base, u32 t, u32 w, u32 lane) {
  const i64 n = o.n_ops;
  if constexpr (FIRST) {
#pragma unroll
    for (int it = 0; it < RREC_ITEMS; ++it) {
      const i64 i = rrec_event(base, w, it, lane);
      const bool v = i < n;
      T.list[it] = v ? o.list[i] : 0u;
      T.op[it] = v ? o.op[i] : 0u;
      T.value[it] = v ? o.value[i] : 0u;
      T.anchor[it] = v ? o.anchor[i] : 0u;
      T.t[it] = v ? o.t[i] : 0;
    }
  } else {
#pragma unroll
    for (int it = 0; it < RREC_ITEMS; ++it) {
      const i64 i = rrec_event(base, w, it, lane);
      T.key[it] = i < n ? kin[i] : 0u;
    }
    // 16-byte chunks of the tile's words; an odd last word of the whole stream reads
    // 8 bytes of the buffer's (256-byte) padding with it
    const i64 cnt = n - base < RREC_TILE ? n - base : RREC_TILE;
    const i64 nv = (cnt * RGA_REC + 1) / 2;
    const v4u32* q = reinterpret_cast<const v4u32*>(rin + (u64)base * RGA_REC);
#pragma unroll
    for (int i = 0; i < RREC_V4; ++i) {
      const i64 x = (i64)t + (i64)i * RR_NT;
      T.w[i] = x < nv ? __builtin_nontemporal_load(&q[x]) : v4u32{0, 0, 0, 0};
    }
  }
}

// A persistent workgroup per CU walks the tiles; per tile: wave multisplit of the
// records by digit (ranks and per-wave digit counts), block scan of the digit totals,
// records staged in LDS in digit order, then every digit's run written contiguously
// (RREC_TILE / 256 records per run on average: whole cache lines).  The next tile's
// loads are issued before the current tile's runs are written, so the two overlap.
template <bool FIRST, typename KO = u32>
__global__ void __launch_bounds__(RR_NT) k_rrec_scatter(smx_rga_ops o, const u32* __restrict__ kin,
                                                        const u64* __restrict__ rin, KO* __restrict__ kout,
                                                        u64* __restrict__ rout, int shift,
                                                        const u32* __restrict__ offs, i32* __restrict__ err,
                                                        u32 ntiles) {
  __shared__ __attribute__((aligned(16))) u64 srec[RREC_TILE * RGA_REC];  // 48 KB
  __shared__ u32 skey[RREC_TILE];
  __shared__ u16 spos[RREC_TILE];            // tile record -> staged slot (pass 2+)
  __shared__ u16 wc[RR_NW][RGA_NDIG];        // per-wave digit counts, then offsets
  __shared__ u32 lstart[RGA_NDIG];
  __shared__ u32 gofs[RGA_NDIG];
  const u32 t = threadIdx.x, lane = t & (WAVE - 1), w = t / WAVE;
  const i64 n = o.n_ops;
  const u64 lt = lanemask_lt();
  RTile<FIRST> T;
  u32 tile = blockIdx.x;
  if (tile < ntiles) rrec_load<FIRST>(T, o, kin, rin, (i64)tile * RREC_TILE, t, w, lane);
  for (; tile < ntiles; tile += gridDim.x) {
    const i64 base = (i64)tile * RREC_TILE;
    const u32 cnt = (u32)(n - base < RREC_TILE ? n - base : RREC_TILE);
    for (int x = t; x < RR_NW * RGA_NDIG; x += RR_NT) (&wc[0][0])[x] = 0;
    if (t < RGA_NDIG) gofs[t] = offs[(i64)tile * RGA_NDIG + t];
    __syncthreads();
    u32 key[RREC_ITEMS], dr[RREC_ITEMS];
#pragma unroll
    for (int it = 0; it < RREC_ITEMS; ++it) {
      const bool valid = rrec_event(base, w, it, lane) < n;
      if constexpr (FIRST) {
        key[it] = T.list[it];
        const bool badl = key[it] >= (u64)o.n_lists, bado = T.op[it] > 2;
        if (valid && (badl || bado)) {
          *err = 1;
          if (badl) key[it] = 0;
        }
      } else {
        key[it] = T.key[it];
      }
      const u32 d = (key[it] >> shift) & 255u;
      const u64 peers = wave_peers<8>(d, valid);
      const u32 before = wc[w][d];
      dr[it] = d | ((before + (u32)__popcll(peers & lt)) << 8);
      if (valid && (peers >> lane) == 1ull) wc[w][d] = (u16)(before + (u32)__popcll(peers));
    }
    __syncthreads();
    if (t < RGA_NDIG) {
      u32 tot = 0;
#pragma unroll
      for (int q = 0; q < RR_NW; ++q) tot += wc[q][t];
      lstart[t] = tot;
    }
    __syncthreads();
    if (t < WAVE) {  // exclusive scan of the 256 digit totals, 4 per lane
      u32 x[4], sum = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        x[j] = lstart[4 * t + j];
        sum += x[j];
      }
      u32 run = wave_incl_sum(sum) - sum;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        lstart[4 * t + j] = run;
        run += x[j];
      }
    }
    __syncthreads();
    if (t < RGA_NDIG) {
      u32 acc = lstart[t];
#pragma unroll
      for (int q = 0; q < RR_NW; ++q) {
        const u32 c = wc[q][t];
        wc[q][t] = (u16)acc;
        acc += c;
      }
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < RREC_ITEMS; ++it) {
      const u32 li = (u32)(w * RREC_SEG + it * WAVE + lane);
      const i64 i = base + li;
      if (i >= n) continue;
      const u32 d = dr[it] & 255u, p = wc[w][d] + (dr[it] >> 8);
      skey[p] = key[it];
      if constexpr (FIRST) {
        u64* r = &srec[p * RGA_REC];
        const u64 tt = (u64)T.t[it] ^ 0x8000000000000000ull;
        r[0] = ((u64)T.anchor[it] << 32) | (tt >> 32);
        const u32 op = T.op[it] > 2 ? 0u : T.op[it];
        r[RGA_WV] = ((u64)T.value[it] << 32) | (op << 30) | (u32)i;
      } else {
        spos[li] = (u16)p;
      }
    }
    if constexpr (!FIRST) {
      __syncthreads();
#pragma unroll
      for (int i = 0; i < RREC_V4; ++i) {
        const u32 c = t + (u32)i * RR_NT;  // words 2c, 2c + 1
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const u32 x = 2 * c + h;
          if (x < cnt * RGA_REC) {
            const u32 r = x / RGA_REC, k = x - r * RGA_REC;
            srec[spos[r] * RGA_REC + k] = h ? ((u64)T.w[i].w << 32 | T.w[i].z) : ((u64)T.w[i].y << 32 | T.w[i].x);
          }
        }
      }
    }
    __syncthreads();
    // the next tile's loads fly while this tile's runs are written
    if (tile + gridDim.x < ntiles) rrec_load<FIRST>(T, o, kin, rin, (i64)(tile + gridDim.x) * RREC_TILE, t, w, lane);
#pragma unroll 1
    for (u32 p = t; p < cnt; p += RR_NT) {  // record-wise: consecutive lanes, consecutive 16-byte records
      const u32 key = skey[p];
      const u32 d = (key >> shift) & 255u;
      const u32 dst = gofs[d] + p - lstart[d];
      kout[dst] = (KO)key;  // (u8: the low byte, for k_rrec_local)
      *reinterpret_cast<R16*>(rout + (u64)dst * RGA_REC) = reinterpret_cast<const R16*>(srec)[p];
    }
    __syncthreads();  // LDS is rewritten by the next tile
  }
}

// lstart[l] = first sorted position of list l (an empty list starts where the next
// one does); one pass over the sorted list ids.
// Also zeroes the survivor sums of 256-list chunks (csum, RGA_CS_MAX words), which the
// list kernels fill and k_rga_out reads.
#define RGA_CS_LISTS 256                   // lists per survivor-sum chunk
#define RGA_CS_MAX 256                     // chunks (k_rga_out: one uint4 per lane)
#define RGA_FUSED_MAX (RGA_CS_LISTS * RGA_CS_MAX)  // lists up to which k_rga_out finds its own offsets
// err word bits: RGA_E_INPUT a list id >= n_lists or an op > 2 (the call fails);
// RGA_E_UNGROUPED a call that said its events come grouped by list (SMX_RGA_GROUPED) has a
// list id that decreases: every list kernel leaves at once and the call is redone with
// the partition
#define RGA_E_INPUT 1
#define RGA_E_UNGROUPED 2

// The list starts that event i of the list-ordered stream decides: lists lo..hi (one past
// the previous event's list .. this event's) start at i, so an empty list starts where the
// next one does; behind the last event the lists past hi start at n.  I: the caller's list-id
// type (u32 in k_rga_gbounds, which clamps hi to nl - 1; i64 in k_rga_bounds).
template <typename I>
__device__ __forceinline__ void rga_fill_starts(u32* lstart, I lo, I hi, i64 i, i64 n, i64 nl) {
  for (I L = lo; L <= hi; ++L) lstart[L] = (u32)i;
  if (i == n - 1)
    for (i64 L = (i64)hi + 1; L < nl; ++L) lstart[L] = (u32)n;
}

// Events already grouped by list (non-decreasing list ids: what crdt.replay and RGA
// hand over, stream after stream) are read in place by the list kernels (ColSrc), so no
// partition runs: only the list starts, which come from the steps of the list id, and
// the input checks, reading the list ids and ops.  Also zeroes the survivor chunk sums
// (k_rga_bounds' duty).
__global__ void __launch_bounds__(BLOCK) k_rga_gbounds(smx_rga_ops o, u32* __restrict__ lstart,
                                                       u32* __restrict__ csum, i32* __restrict__ err) {
  const i64 n = o.n_ops, nl = o.n_lists;
  if (blockIdx.x == 0 && threadIdx.x < RGA_CS_MAX) csum[threadIdx.x] = 0u;
  u32 bad = 0;
  // four consecutive events per thread: one 16-byte list-id load and one 4-byte op load
  // when aligned (the columns are the caller's: checked, else event by event)
  const bool vec = ((reinterpret_cast<uintptr_t>(o.list) | reinterpret_cast<uintptr_t>(o.op)) & 3) == 0 &&
                   (reinterpret_cast<uintptr_t>(o.list) & 15) == 0;
  for (i64 i0 = ((i64)blockIdx.x * BLOCK + threadIdx.x) * 4; i0 < n; i0 += (i64)gridDim.x * BLOCK * 4) {
    u32 l4[4], op4[4];
    if (vec && i0 + 4 <= n) {
      const uint4 v = *reinterpret_cast<const uint4*>(o.list + i0);
      const u32 ob = *reinterpret_cast<const u32*>(o.op + i0);
      l4[0] = v.x, l4[1] = v.y, l4[2] = v.z, l4[3] = v.w;
#pragma unroll
      for (int u = 0; u < 4; ++u) op4[u] = (ob >> (8 * u)) & 0xffu;
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        l4[u] = i0 + u < n ? (u32)o.list[i0 + u] : 0u;
        op4[u] = i0 + u < n ? (u32)o.op[i0 + u] : 0u;
      }
    }
    u32 prev = i0 > 0 ? (u32)o.list[i0 - 1] : 0u;  // (the neighbour lane's line: an L1 hit)
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const i64 i = i0 + u;
      if (i >= n) break;
      const u32 l = l4[u], op = op4[u];
      bad |= (l >= (u64)nl || op > 2) ? (u32)(RGA_E_INPUT | RGA_E_UNGROUPED) : 0u;
      bad |= i > 0 && l < prev ? (u32)RGA_E_UNGROUPED : 0u;
      const u32 lo = i == 0 ? 0u : prev + 1u, hi = l < (u64)nl ? l : (u32)(nl - 1);
      rga_fill_starts(lstart, lo, hi, i, n, nl);
      prev = l;
    }
  }
  if (bad) atomicOr(err, (i32)bad);
}

__global__ void k_rga_bounds(const u32* __restrict__ keys, i64 n, i64 nl, u32* __restrict__ lstart,
                             u32* __restrict__ csum) {
  if (blockIdx.x == 0 && threadIdx.x < RGA_CS_MAX) csum[threadIdx.x] = 0u;
  for (i64 j = (i64)blockIdx.x * BLOCK + threadIdx.x; j < n; j += (i64)gridDim.x * BLOCK) {
    const i64 l = keys[j];
    rga_fill_starts<i64>(lstart, (j ? (i64)keys[j - 1] : -1) + 1, l, j, n, nl);
  }
}

// Two-byte list ids (257..65536 lists): the first pass partitions by the HIGH byte
// (k_rrec_hist / k_rrec_scatter, stable), then one workgroup per high-byte bucket orders
// its records by the low byte on its own (k_rrec_local): a count, a scan in LDS and a
// stable scatter of tiles in stream order -- no global histogram, scan or bounds pass
// (the bucket's list starts come from its scan), and no list ids written (the list
// kernels read only the starts).  Bucket d is [dstart[d], dstart[d + 1]).
#define RL_NT 1024
#define RL_NW (RL_NT / WAVE)
#ifndef RL_ITEMS
#define RL_ITEMS 4
#endif
#define RL_TILE (RL_NT * RL_ITEMS)
#define RL_SEG (RL_TILE / RL_NW)  // contiguous records per wave and tile
#define RL_CU 8                   // count phase: keys in flight per lane
#ifndef RL_S
#define RL_S 2  // workgroups per bucket
#endif
__global__ void __launch_bounds__(RL_NT) k_rrec_local(const u8* __restrict__ kin, const u64* __restrict__ rin,
                                                      u64* __restrict__ rout,
                                                      const u32* __restrict__ dstart, i64 nl,
                                                      u32* __restrict__ lstart, u32* __restrict__ csum) {
  __shared__ u32 cnt[RGA_NDIG];
  __shared__ u32 run[RGA_NDIG];
  __shared__ u16 wc[RL_NW][RGA_NDIG];
  __shared__ u32 tstart[RGA_NDIG], wsum[RGA_NDIG / WAVE];
  const u32 t = threadIdx.x, lane = t & (WAVE - 1), w = t / WAVE;
  // RL_S workgroups per bucket (two fit a CU): workgroup h scatters the h-th part of the
  // bucket, after counting the whole bucket and the parts before its own
  const u32 d = blockIdx.x / RL_S, h = blockIdx.x - d * RL_S;
  if (blockIdx.x == 0 && t < RGA_CS_MAX) csum[t] = 0u;  // (k_rga_bounds' other duty)
  const u32 b0 = dstart[d], b1 = dstart[d + 1];
  const u32 seg = (b1 - b0 + RL_S - 1) / RL_S;
  const u32 sa = min(b0 + h * seg, b1), sb = min(sa + seg, b1);
  u32 kd[RL_ITEMS], dr[RL_ITEMS];
  R16 rv[RL_ITEMS];
  auto load_tile = [&](u32 base) {
#pragma unroll
    for (int it = 0; it < RL_ITEMS; ++it) {
      const u32 i = base + w * RL_SEG + it * WAVE + lane;
      const bool valid = i < sb;
      kd[it] = valid ? kin[i] : 0u;
      rv[it].a = valid ? rin[(u64)i * RGA_REC] : 0ull;
      rv[it].b = valid ? rin[(u64)i * RGA_REC + 1] : 0ull;
    }
  };
  if (t < RGA_NDIG) {
    cnt[t] = 0;
    tstart[t] = 0;  // (first: the counts of the parts before this workgroup's)
  }
  __syncthreads();
  {  // 4 low bytes per load (aligned words over [b0, b1); the buffer has room past n)
    const u32* kw = reinterpret_cast<const u32*>(kin);
    const u32 w0 = b0 >> 2, w1 = (b1 + 3) >> 2;
    for (u32 x0 = w0 + t; x0 < w1; x0 += RL_NT * RL_CU) {  // RL_CU loads in flight per lane
      u32 k[RL_CU];
#pragma unroll
      for (int j = 0; j < RL_CU; ++j) {
        const u32 x = x0 + j * RL_NT;
        k[j] = x < w1 ? kw[x] : 0u;
      }
#pragma unroll
      for (int j = 0; j < RL_CU; ++j) {
        const u32 x = x0 + j * RL_NT;
        if (x >= w1) continue;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const u32 i = 4 * x + q;
          if (i >= b0 && i < b1) {
            const u32 dd = (k[j] >> (8 * q)) & 255u;
            atomicAdd(&cnt[dd], 1u);
            if (i < sa) atomicAdd(&tstart[dd], 1u);
          }
        }
      }
    }
  }
  __syncthreads();
  if (t < WAVE) {  // exclusive scan of the 256 low-byte counts, 4 per lane
    u32 x[4], sum = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      x[j] = cnt[4 * t + j];
      sum += x[j];
    }
    u32 r = wave_incl_sum(sum) - sum;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      run[4 * t + j] = b0 + r;
      r += x[j];
    }
  }
  __syncthreads();
  if (t < RGA_NDIG) {  // list starts (an empty list starts where the next one does)
    const i64 l = (i64)d * RGA_NDIG + t;
    if (h == 0 && l < nl) lstart[l] = run[t];
    run[t] += tstart[t];
  }
  __syncthreads();
  const u64 lt = lanemask_lt();
  // the tile's records staged in LDS in (low byte, stream) order, then written run by
  // run: consecutive lanes store consecutive 16-byte records of one list
  __shared__ R16 stg[RL_TILE];
  __shared__ u8 sdig[RL_TILE];
  for (u32 base = sa; base < sb; base += RL_TILE) {
    load_tile(base);
    for (u32 x = t; x < RL_NW * RGA_NDIG; x += RL_NT) (&wc[0][0])[x] = 0;
    __syncthreads();
#pragma unroll
    for (int it = 0; it < RL_ITEMS; ++it) {
      const u32 i = base + w * RL_SEG + it * WAVE + lane;
      const bool valid = i < sb;
      const u32 dd = kd[it] & 255u;
      const u64 peers = wave_peers<8>(dd, valid);
      const u32 before = wc[w][dd];
      dr[it] = dd | ((before + (u32)__popcll(peers & lt)) << 8);
      if (valid && (peers >> lane) == 1ull) wc[w][dd] = (u16)(before + (u32)__popcll(peers));
    }
    __syncthreads();
    u32 tc = 0, inc = 0;
    if (t < RGA_NDIG) {  // per-wave offsets inside the digit's share of the tile
#pragma unroll
      for (int q = 0; q < RL_NW; ++q) {
        const u32 c = wc[q][t];
        wc[q][t] = (u16)tc;
        tc += c;
      }
      inc = wave_incl_sum(tc);
      if (lane == WAVE - 1) wsum[w] = inc;
    }
    __syncthreads();
    if (t < RGA_NDIG) {
      u32 ex = inc - tc;
      for (u32 q = 0; q < w; ++q) ex += wsum[q];
      tstart[t] = ex;
      cnt[t] = tc;
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < RL_ITEMS; ++it) {
      const u32 i = base + w * RL_SEG + it * WAVE + lane;
      if (i >= sb) continue;
      const u32 dd = dr[it] & 255u;
      const u32 slot = tstart[dd] + wc[w][dd] + (dr[it] >> 8);
      stg[slot] = rv[it];
      sdig[slot] = (u8)dd;
    }
    __syncthreads();
    const u32 nv = min((u32)RL_TILE, sb - base);
    for (u32 j = t; j < nv; j += RL_NT) {
      const u32 dd = sdig[j];
      const u32 pos = run[dd] + (j - tstart[dd]);
      *(R16*)(rout + (u64)pos * RGA_REC) = stg[j];
    }
    __syncthreads();
    if (t < RGA_NDIG) run[t] += cnt[t];
  }
}
