// smx_segsort.h -- the generic plan's segmented sort (k_segsort) and the radix plan's
// duplicate-key check (k_dupcheck).  Part of the smx_compose.hip unit: included once, there.
#pragma once

// Generic plan: each branch sorted by (ts, oid_hi, oid_lo, index), then fixed windows
// over the sorted logs (k_window_g).  Used when the presorted plan fails.  Two ways to
// sort a branch:
//  * segmented (GEN_SEG): the branch's timestamps never decrease but its equal-timestamp
//    groups are too long for a presorted window (config 5) -- only each group needs
//    sorting, by oid.  Nominal tiles of SEG_H ops snap back to a group start, so each
//    tile holds whole groups (fewer than SEG_H + the longest group ops); a block sorts
//    its tile with a bitonic network on (group, top 38 bits of oid_hi, tile index), and
//    runs of equal (group, hi38) (rare; every duplicate id) are re-sorted exactly on
//    (oid_hi, oid_lo, index).  A group longer than SEG_CAP - SEG_H ops or a timestamp that decreases sets
//    meta->seg_over and the radix sort runs instead.
//  * radix (GEN_RADIX / GEN_RADIX_LO): stable LSD radix sort on (ts, oid_hi), checked
//    afterwards for adjacent (ts, oid_hi) duplicates, which rerun it with oid_lo.
#define SEG_CAP 8192
#define SEG_H 4096
#define SEG_NT 1024
enum { GEN_SEG, GEN_RADIX, GEN_RADIX_LO };

__global__ void k_dupcheck(const u64* __restrict__ sts, const u64* __restrict__ shi, i64 na, i64 n,
                           ComposeMeta* meta) {
  for (i64 i = (i64)blockIdx.x * BLOCK + threadIdx.x + 1; i < n; i += (i64)gridDim.x * BLOCK)
    if (i != na && sts[i] == sts[i - 1] && shi[i] == shi[i - 1]) meta->dup_key = 1;
}

// One pass of the bitonic network over 8 keys per thread: the thread holds keys
// base | m << b (m = 0..7) and runs the stages whose partner bit is b + 2, b + 1, b
// (the top `nbits` of them), ascending where bit k of the index is clear.
__device__ __forceinline__ void seg_pass(u64 (&v)[8], u32 base, u32 b, u32 k, int top, int nbits) {
#pragma unroll
  for (int bit = 2; bit >= 0; --bit) {
    if (bit > top || bit <= top - nbits) continue;
#pragma unroll
    for (int m = 0; m < 8; ++m) {
      if ((m >> bit) & 1) continue;
      const int m2 = m | (1 << bit);
      const bool asc = ((base | ((u32)m << b)) & k) == 0;
      const u64 x = v[m], y = v[m2];
      const bool sw = asc ? y < x : x < y;
      v[m] = sw ? y : x;
      v[m2] = sw ? x : y;
    }
  }
}

// Interpolation buckets (the default): element x of group [gs, ge) goes to bucket
// (gs + (ge - gs) * hi32 / 2^32) / 2, i.e. two elements per bucket on random ids;
// buckets are ordered like (group, hi), a counting sort places them and each element
// ranks itself on the full key inside its bucket.  A bucket above SEG_BKMAX (ids that
// cluster) sends the tile to the bitonic network.  The key array is unpadded so that two
// blocks (64 KB keys + 8 KB of 16-bit bucket counters each) fit a CU.
#define SEGPAD(i) (i)
#define SEG_NBK (SEG_CAP / 2)
#define SEG_BKMAX 32

// One tile of one branch (ts, hi, lo: the branch's columns; outputs at the branch's
// offset; off: the branch's first op index in A||B).  Sort key, one u64 per element:
// group (13 bits) | top 38 bits of oid_hi | tile index (13 bits) -- unique, so the
// bitonic network needs no payload; equal (group, hi38) pairs (rare on random ids,
// every duplicate id) are re-sorted exactly afterwards.  Each thread holds 8 keys whose
// indices differ in three consecutive bits b .. b+2, so three stages of the network run
// in registers per LDS round trip (33 round trips for 8192 keys instead of 91 stages).
// The segmented sort cannot order this log: seg_over for the host, and f_fail bit 3 so
// that every kernel queued behind the sort (k_gpart, k_wcount, k_window_g, the tail)
// leaves at once -- the host learns it from the merge's one meta read and runs the
// radix plan then (no host round trip between the sort and the windows).
// seg_over bit 0: a timestamp group longer than a tile holds (the branch is ordered: the
// radix plan orders it); bit 1 (SEG_DECREASE): a timestamp decreases (a sharded range
// slice must then fail, not be radix-sorted locally: smx_shard_step ORDER_FIX).
__device__ __forceinline__ void seg_fail(ComposeMeta* meta, bool decrease) {
  atomicOr((unsigned long long*)&meta->seg_over, decrease ? (unsigned long long)SEG_DECREASE : 1ull);
  atomicOr((unsigned long long*)&meta->f_fail, (unsigned long long)SEG_FAIL_BIT);
}

// One launch per branch (both in one grid measured slower: segsort 0.52 -> 0.60 ms on
// config 5, profiles/r03_v).
__global__ void __launch_bounds__(SEG_NT) k_segsort(const u64* __restrict__ ts, const u64* __restrict__ hi,
                                                    const u64* __restrict__ lo, i64 cnt, u32 off,
                                                    u64* __restrict__ sts, u64* __restrict__ shi,
                                                    u64* __restrict__ slo, u32* __restrict__ perm,
                                                    ComposeMeta* meta) {
  constexpr int PER = SEG_CAP / SEG_NT;  // 8 keys per thread
  static_assert(PER == 8, "the register passes assume 8 keys per thread");
  __shared__ u64 key[SEGPAD(SEG_CAP)];
  __shared__ u32 wsum[SEG_NT / WAVE + 1];
  __shared__ i64 se[2];
  __shared__ u32 bcnt[SEG_NBK / 2];  // two 16-bit bucket counters per word
  const int t = threadIdx.x, lane = t & (WAVE - 1), wv = t / WAVE;
  const i64 p0 = (i64)blockIdx.x * SEG_H;
  // Layout: every adjacent pair of the nominal range (the nominal ranges cover the
  // branch).  Tile bounds: the group of p0 (and of p0 + SEG_H) starts within the
  // SEG_CAP - SEG_H ops before it, where the ops below its timestamp are counted.
  constexpr int W = SEG_CAP - SEG_H;
  const u64 v0 = ts[p0];
  const bool has_end = p0 + SEG_H < cnt;
  const u64 v1 = has_end ? ts[p0 + SEG_H] : 0;
  bool dec = false, bad = false;
  u32 c0 = 0, c1 = 0;
#pragma unroll
  for (int r = 0; r < SEG_H / SEG_NT; ++r) {
    const i64 i = p0 + r * SEG_NT + t;
    if (i + 1 < cnt) dec |= ts[i + 1] < ts[i];
  }
#pragma unroll
  for (int r = 0; r < W / SEG_NT; ++r) {
    const i64 i0 = p0 - W + r * SEG_NT + t, i1 = p0 + SEG_H - W + r * SEG_NT + t;
    if (i0 >= 0) c0 += ts[i0] < v0;
    if (has_end) c1 += ts[i1] < v1;
  }
  if (t < 2) se[t] = 0;
  __syncthreads();
  c0 = wave_incl_sum(c0);
  c1 = wave_incl_sum(c1);
  if (lane == WAVE - 1) {
    atomicAdd((unsigned long long*)&se[0], (unsigned long long)c0);
    atomicAdd((unsigned long long*)&se[1], (unsigned long long)c1);
  }
  const i64 a0 = p0 - W > 0 ? p0 - W : 0, a1 = p0 + SEG_H - W;
  // a group reaching below its window: longer than the tile scheme allows
  if (t == 0 && p0 - W > 0 && ts[p0 - W - 1] == v0) bad = true;
  if (t == 1 && has_end && a1 > 0 && ts[a1 - 1] == v1) bad = true;
  const bool any_dec = __syncthreads_or(dec);
  if (any_dec | __syncthreads_or(bad)) {
    if (t == 0) seg_fail(meta, any_dec);
    return;
  }
  const i64 s = a0 + se[0], size = (has_end ? a1 + se[1] : cnt) - s;
  if (size <= 0) return;
  if (size > SEG_CAP) {
    if (t == 0) seg_fail(meta, false);
    return;
  }
  u32 P = 8, lgP = 3;
  while (P < (u32)size) P <<= 1, ++lgP;
  const bool own = (u32)t * PER < P;  // this thread holds 8 keys of the network
  // group index of each element: inclusive count of group starts after the first
  u32 f[PER], run = 0;
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const i64 x = (i64)t * PER + k;
    f[k] = x > 0 && x < size && ts[s + x] != ts[s + x - 1];
    run += f[k];
  }
  const u32 inc = wave_incl_sum(run);
  if (lane == WAVE - 1) wsum[wv] = inc;
  __syncthreads();
  u32 g = inc - run;
  for (int q = 0; q < wv; ++q) g += wsum[q];
  u64 v[PER];
  u32 gk[PER];
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const u32 x = t * PER + k;
    g += f[k];
    gk[k] = g;
    v[k] = x < (u32)size ? ((u64)g << 51) | ((hi[s + x] >> 26) << 13) | x : ~0ull;  // padding sorts last
  }
  bool bitonic = false;
  {
    u32 ng = 1;  // groups in the tile
    for (int q = 0; q < SEG_NT / WAVE; ++q) ng += wsum[q];
    u16* gst = reinterpret_cast<u16*>(key);  // group starts (the key array is free until the scatter)
    for (int i = t; i < SEG_NBK / 2; i += SEG_NT) bcnt[i] = 0u;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const u32 x = t * PER + k;
      if (x < (u32)size && (x == 0 || f[k])) gst[gk[k]] = (u16)x;
    }
    __syncthreads();
    u32 bk[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const u32 x = t * PER + k;
      bk[k] = 0;
      if (x < (u32)size) {
        const u32 gs = gst[gk[k]], ge = gk[k] + 1 < ng ? (u32)gst[gk[k] + 1] : (u32)size;
        const u32 h32 = (u32)(v[k] >> 19);  // the top 32 of the 38 id bits
        bk[k] = (gs + (u32)(((u64)(ge - gs) * h32) >> 32)) >> 1;
        atomicAdd(&bcnt[bk[k] >> 1], 1u << (16 * (bk[k] & 1)));
      }
    }
    __syncthreads();
    // exclusive scan of the counters (4 per thread), largest bucket -> fallback
    const u32 nbw = ((u32)size + 3) / 4;  // counter words in use: 2 words per thread
    u32 w0 = 2 * t < nbw ? bcnt[2 * t] : 0u, w1 = 2 * t + 1 < nbw ? bcnt[2 * t + 1] : 0u;
    const u32 c0 = w0 & 0xffffu, c1 = w0 >> 16, c2 = w1 & 0xffffu, c3 = w1 >> 16;
    const u32 mx = max(max(c0, c1), max(c2, c3));
    u32 tot;
    const u32 e0 = block_excl_scan<OpSum, u32, SEG_NT / WAVE>(c0 + c1 + c2 + c3, wsum, &tot);
    const u32 e1 = e0 + c0, e2 = e1 + c1, e3 = e2 + c2;
    if (2 * t < nbw) bcnt[2 * t] = e0 | (e1 << 16);
    if (2 * t + 1 < nbw) bcnt[2 * t + 1] = e2 | (e3 << 16);
    bitonic = __syncthreads_or(mx > SEG_BKMAX);
    if (!bitonic) {
      // scatter: the counters become bucket ends
#pragma unroll
      for (int k = 0; k < PER; ++k) {
        const u32 x = t * PER + k;
        if (x < (u32)size) {
          const u32 sh = 16 * (bk[k] & 1);
          const u32 old = atomicAdd(&bcnt[bk[k] >> 1], 1u << sh);
          key[(old >> sh) & 0xffffu] = v[k];
        }
      }
      __syncthreads();
      u32 fp[PER];
#pragma unroll
      for (int k = 0; k < PER; ++k) {
        const u32 x = t * PER + k;
        fp[k] = 0;
        if (x < (u32)size) {
          const u32 b = bk[k];
          const u32 e = (bcnt[b >> 1] >> (16 * (b & 1))) & 0xffffu;
          const u32 lo = b ? (bcnt[(b - 1) >> 1] >> (16 * ((b - 1) & 1))) & 0xffffu : 0u;
          u32 c = 0;
          for (u32 q = lo; q < e; ++q) c += key[q] < v[k];
          fp[k] = lo + c;
        }
      }
      __syncthreads();
#pragma unroll
      for (int k = 0; k < PER; ++k)
        if (t * PER + k < (u32)size) key[fp[k]] = v[k];
      __syncthreads();
    }
  }
  if (bitonic) {
    // merge levels k = 2, 4, 8: keys 8t .. 8t+7 (b = 0)
    seg_pass(v, (u32)t * 8, 0, 2, 0, 1);
    seg_pass(v, (u32)t * 8, 0, 4, 1, 2);
    seg_pass(v, (u32)t * 8, 0, 8, 2, 3);
    // later levels: a pass per window b of three partner bits; the keys move between
    // layouts through LDS (write in the old layout, read in the new one)
    u32 cur = 0;  // layout of v
    auto base_of = [&](u32 b) { return ((u32)t >> b << (b + 3)) | ((u32)t & ((1u << b) - 1)); };
    for (u32 lk = 4; lk <= lgP; ++lk) {
      const u32 k = 1u << lk;
      for (int jb = (int)lk - 1; jb >= 0;) {
        const u32 b = jb >= 2 ? (u32)jb - 2 : 0u;
        if (b != cur) {
          __syncthreads();  // the previous layout's reads are done
          if (own) {
            const u32 bo = base_of(cur);
#pragma unroll
            for (int m = 0; m < PER; ++m) key[SEGPAD(bo | ((u32)m << cur))] = v[m];
          }
          __syncthreads();
          if (own) {
            const u32 bn = base_of(b);
#pragma unroll
            for (int m = 0; m < PER; ++m) v[m] = key[SEGPAD(bn | ((u32)m << b))];
          }
          cur = b;
        }
        if (own) seg_pass(v, base_of(b), b, k, jb - (int)b, jb - (int)b + 1);
        jb = (int)b - 1;
      }
    }
    __syncthreads();
    if (own) {
      const u32 bo = base_of(cur);
#pragma unroll
      for (int m = 0; m < PER; ++m) key[SEGPAD(bo | ((u32)m << cur))] = v[m];
    }
    __syncthreads();
  }
  // runs of equal (group, hi38): exact order on (oid_hi, oid_lo, index)
  for (u32 x = t; x + 1 < (u32)size; x += SEG_NT) {
    const u64 kx = key[SEGPAD(x)] >> 13;
    if ((key[SEGPAD(x + 1)] >> 13) != kx || (x > 0 && (key[SEGPAD(x - 1)] >> 13) == kx)) continue;
    u32 e = x + 2;
    while (e < (u32)size && (key[SEGPAD(e)] >> 13) == kx) ++e;
    for (u32 y = x + 1; y < e; ++y) {
      const u64 ky = key[SEGPAD(y)];
      const u32 vi = (u32)ky & 0x1fffu;
      const u64 vh = hi[s + vi], vl = lo[s + vi];
      u32 z = y;
      while (z > x) {
        const u64 kw = key[SEGPAD(z - 1)];
        const u32 wi = (u32)kw & 0x1fffu;
        const u64 wh = hi[s + wi], wl = lo[s + wi];
        if (!(vh < wh || (vh == wh && (vl < wl || (vl == wl && vi < wi))))) break;
        key[SEGPAD(z)] = kw;
        --z;
      }
      key[SEGPAD(z)] = ky;
    }
  }
  __syncthreads();
  for (u32 x = t; x < (u32)size; x += SEG_NT) {
    const i64 src = s + (key[SEGPAD(x)] & 0x1fffu);
    sts[s + x] = ts[src];
    shi[s + x] = hi[src];
    slo[s + x] = lo[src];
    perm[s + x] = off + (u32)src;
  }
}
