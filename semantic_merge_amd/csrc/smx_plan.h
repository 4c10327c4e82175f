// smx_plan.h -- the planning kernels of a merge: the presorted plan's chunk histogram,
// window boundaries and column scans (k_khist, k_fpart, k_cscan_*), the generic plan's
// boundaries, counts and bases (k_gpart, k_wcount, k_wscan, k_bases) and its gathers.
// Part of the smx_compose.hip unit: included once, there.
#pragma once

// Per-branch OR / AND of the key words (generic path: skip constant radix digits).
__global__ void __launch_bounds__(BLOCK) k_keymask(const u64* __restrict__ ts, const u64* __restrict__ hi,
                                                   const u64* __restrict__ lo, i64 na, i64 n,
                                                   ComposeMeta* meta) {
  u64 ro[2][3] = {{0, 0, 0}, {0, 0, 0}};
  u64 ra[2][3] = {{~0ull, ~0ull, ~0ull}, {~0ull, ~0ull, ~0ull}};
  for (i64 i = (i64)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (i64)gridDim.x * BLOCK) {
    const u64 v[3] = {ts[i], hi[i], lo[i]};
    const int s = i >= na;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      ro[s][q] |= v[q];
      ra[s][q] &= v[q];
    }
  }
  // wave OR of the 12 words (AND = NOT OR NOT) on DPP, then LDS, then one device
  // atomic per word and block (a device atomic per thread serialised on 12 words)
  __shared__ u32 sm[24];
  if (threadIdx.x < 24) sm[threadIdx.x] = 0;
  __syncthreads();
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const u64 w[2] = {ro[s][q], ~ra[s][q]};
#pragma unroll
      for (int x = 0; x < 2; ++x) {
        const u32 lo32 = wave_or_to_last((u32)w[x]), hi32 = wave_or_to_last((u32)(w[x] >> 32));
        if ((threadIdx.x & (WAVE - 1)) == WAVE - 1) {
          atomicOr(&sm[(s * 3 + q) * 4 + 2 * x], lo32);
          atomicOr(&sm[(s * 3 + q) * 4 + 2 * x + 1], hi32);
        }
      }
    }
  __syncthreads();
  if (threadIdx.x < 6) {
    const int s = threadIdx.x / 3, q = threadIdx.x % 3;
    const u32* v = &sm[threadIdx.x * 4];
    atomicOr((unsigned long long*)&meta->key_or[s][q], ((unsigned long long)v[1] << 32) | v[0]);
    atomicAnd((unsigned long long*)&meta->key_and[s][q], ~(((unsigned long long)v[3] << 32) | v[2]));
  }
}

// Zero fill as a kernel: the asynchronous part of a merge, which is captured into a
// HIP graph, holds kernel nodes only.
__global__ void k_zero(u32* __restrict__ p, u64 nw) {
  for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < nw; i += (u64)gridDim.x * blockDim.x) p[i] = 0u;
}
static int zero_async(void* p, size_t bytes, hipStream_t st) {
  if (bytes % 4) return set_err(SMX_E_ARG, "zero_async: size not a multiple of 4");
  const u64 nw = bytes / 4;
  if (nw == 0) return SMX_OK;
  u64 g = SMX_CEIL_DIV(nw, (u64)BLOCK * 4);
  if (g > 4096) g = 4096;
  hipLaunchKernelGGL(k_zero, dim3((u32)g), dim3(BLOCK), 0, st, (u32*)p, nw);
  HIP_TRY(hipGetLastError());
  return SMX_OK;
}

__global__ void k_meta_init(ComposeMeta* meta) {
  for (int s = 0; s < 2; ++s)
    for (int q = 0; q < 3; ++q) meta->key_and[s][q] = ~0ull;
}

// Presorted windows: boundary k sits at the merge-path split of diagonal k*tgt
// (timestamps, A first on ties), snapped down to the first op of that timestamp on
// both branches, so every (timestamp) group lands whole in one window.
// tgt is a multiple of CH, so at split candidates m = CH*i the merge-path test
// A[m] <= B[d-1-m] reads only chunk samples (sA[i] = A[CH*i], sB[j] =
// B[CH*j + CH-1]; 1/256 of the keys, cache-resident): the first level of the
// search runs on them, the second inside one chunk.  The snap gallops back over
// the (short) run of equal timestamps.
// LongW (the synchronous merge's early verdict): k_khist made the long-group test; on its
// F_LONG these are the wide plan's boundaries (tgt_w, W_w windows of D_w chunks, its own
// long test flagging F_WLONG) and k_cscan_mid then clears F_LONG, so no normal window, no
// re-arm and no second k_fpart run (config 5's doomed attempt).
struct LongW {
  i64 tgt_w = 0, W_w = 0, D_w = 0;  // tgt_w 0: off
};
__device__ __forceinline__ void fpart_body(const u64* __restrict__ ts, const u64* __restrict__ tsB,
                                           const u64* __restrict__ sA, const u64* __restrict__ sB, i64 na, i64 nb,
                                           i64 W, i64 tgt, i64 D, i64* __restrict__ bnd, ComposeMeta* meta,
                                           u32* long_host, i64 blk, i64 nblk, LongW lw = LongW{}) {
  const i64 k = blk * BLOCK + threadIdx.x;
  bool chk = true;  // flag timestamp groups longer than a window (from k_khist's samples)
  u64 fl = F_LONG;
  if (lw.tgt_w) {
    if ((__hip_atomic_load(&meta->f_fail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & F_LONG) == F_LONG) {
      W = lw.W_w, tgt = lw.tgt_w, D = lw.D_w;  // the wide plan, tested at its own capacity
      fl = F_WLONG;
      long_host = nullptr;
    } else {
      chk = false;  // (k_khist tested the normal capacity)
    }
  }
  if (chk) {
    // A chunk sample equal to the sample D chunks (one window capacity) later (A: first
    // ops of chunks c and c + D; B: last ops of full chunks): that timestamp group alone
    // overflows a window, so the presorted plan cannot hold.  Flagged before the windows
    // run: k_window_f then leaves before its loads (6: a window too large, and smaller
    // windows cannot help).  Grid-stride over the samples, off the search's path.
    const i64 nt = nblk * BLOCK, ca = SMX_CEIL_DIV(na, (i64)CH), cb = nb / CH;
    bool lg = false;
    for (i64 c = k; c + D < ca; c += nt) lg |= sA[c] == sA[c + D];
    for (i64 c = k; c + D < cb; c += nt) lg |= sB[c] == sB[c + D];
    const u64 lgw = __ballot(lg);
    if (lgw && (threadIdx.x & (WAVE - 1)) == 0 &&
        (__hip_atomic_load(&meta->f_fail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & fl) != fl) {
      atomicOr((unsigned long long*)&meta->f_fail, fl);
      // ... and, on the synchronous path, to the host (pinned, coherent), which then
      // launches no tail behind this failed plan
      if (long_host) __hip_atomic_store(long_host, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    // a wave that saw the plan fail leaves its boundaries unsearched, as 0 (k_window_f
    // leaves before its loads on F_LONG, and a zero boundary only ever gives an empty or
    // an oversized window; the wide plan redoes them) -- on config 5 the snap's gallops
    // over 4096-op timestamp runs were most of this kernel
    if (lgw) {
      if (k <= W) bnd[2 * k] = bnd[2 * k + 1] = 0;
      return;
    }
  }
  if (k > W) return;
  const i64 n = na + nb;
  const u64* A = ts;
  const u64* B = tsB;
  const i64 d = k * tgt;
  if (k == 0 || d >= n || k == W) {
    bnd[2 * k] = k == 0 ? 0 : na;
    bnd[2 * k + 1] = k == 0 ? 0 : nb;
    return;
  }
  const i64 lo0 = d - nb > 0 ? d - nb : 0, hi0 = d < na ? d : na;
  i64 lo = lo0, hi = hi0;
  if (lo < hi) {
    const i64 ilo = SMX_CEIL_DIV(lo, (i64)CH), ihi = (hi - 1) / CH;  // samples inside [lo, hi)
    if (ilo <= ihi) {
      const i64 dj = d / CH - 1;
      i64 l = ilo, h = ihi + 1;
      while (l < h) {
        const i64 mid = (l + h) >> 1;
        if (sA[mid] <= sB[dj - mid]) l = mid + 1;
        else h = mid;
      }
      // test true at CH*(l-1) (if l > ilo), false at CH*l (if l <= ihi)
      if (l > ilo) lo = CH * (l - 1) + 1;
      if (l <= ihi) hi = CH * l;
    }
    while (lo < hi) {
      const i64 mid = (lo + hi) >> 1;
      if (A[mid] <= B[d - 1 - mid]) lo = mid + 1;
      else hi = mid;
    }
  }
  const i64 a = lo, b = d - lo;
  const u64 tau = (a < na && (b >= nb || A[a] <= B[b])) ? A[a] : B[b];
  // first index of each branch with ts >= tau: at or before the split
  i64 r[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const u64* X = s ? B : A;
    i64 h = s ? b : a;  // X[h] >= tau, or h == branch length
    i64 step = 1, l = 0;
    while (h > 0) {
      const i64 cand = h - step > 0 ? h - step : 0;
      if (X[cand] < tau) {
        l = cand + 1;
        break;
      }
      h = cand;
      step *= 2;
    }
    while (l < h) {
      const i64 mid = (l + h) >> 1;
      if (X[mid] < tau) l = mid + 1;
      else h = mid;
    }
    r[s] = l;
  }
  bnd[2 * k] = r[0];
  bnd[2 * k + 1] = r[1];
}
__global__ void k_fpart(const u64* __restrict__ ts, const u64* __restrict__ tsB, const u64* __restrict__ sA,
                        const u64* __restrict__ sB, i64 na, i64 nb, i64 W, i64 tgt, i64 D, i64* __restrict__ bnd,
                        ComposeMeta* meta, u32* long_host, LongW lw) {
  fpart_body(ts, tsB, sA, sB, na, nb, W, tgt, D, bnd, meta, long_host, blockIdx.x, gridDim.x, lw);
}

// Generic windows over branch logs sorted by (ts, oid): fixed diagonals of WIN_CAP.
__global__ void k_gpart(const u64* __restrict__ sts, const u64* __restrict__ shi,
                        const u64* __restrict__ slo, i64 na, i64 nb, i64 W, i64* __restrict__ bnd,
                        const ComposeMeta* meta) {
  const i64 k = (i64)blockIdx.x * BLOCK + threadIdx.x;
  if (k > W || meta->f_fail) return;  // (the segmented sort failed: nothing to cut)
  const i64 n = na + nb;
  const i64 d = k * WG_CAP;
  if (k == 0) { bnd[0] = 0; bnd[1] = 0; return; }
  if (d >= n || k == W) { bnd[2 * k] = na; bnd[2 * k + 1] = nb; return; }
  i64 lo = d - nb > 0 ? d - nb : 0, hi = d < na ? d : na;
  while (lo < hi) {
    i64 mid = (lo + hi) >> 1;
    const i64 j = na + d - 1 - mid;
    if (key_le(sts[mid], shi[mid], slo[mid], sts[j], shi[j], slo[j])) lo = mid + 1;
    else hi = mid;
  }
  bnd[2 * k] = lo;
  bnd[2 * k + 1] = d - lo;
}

// Presorted plan, counting: kind histogram of fixed 256-op chunks of each branch
// (cnt[side][kind][chunk]), then an exclusive scan over chunks per (side, kind).
// A window derives its T offsets from the chunk prefixes at its start plus the
// kinds of at most 255 ops before it.  Coalesced: iteration j of a block reads
// chunk j, lane t its byte t.
#ifndef KH_NT
#define KH_NT 512                  // 32 chunks per block: a column's counts fill a 128-byte line
#endif
#define CH_PER_BLOCK (KH_NT / 16)   // 16 lanes x 16 kind bytes per 256-op chunk
#ifndef KH_R
#define KH_R 1                     // chunk rounds per block (4 measured slower: profiles/r02_k/khist_rounds_ab.txt)
#endif

// Block b counts global chunks [b*CH_PER_BLOCK, ...) (A chunks, then B chunks):
// lane t reads bytes [16*(t%16), +16) of chunk t/16 (one 16-byte load when
// aligned), so a chunk is one 16-lane DPP row.  No atomics: each lane counts its 16
// kinds in packed 5-bit fields (6 kinds per word), widens them to 10-bit fields and
// the row adds them up with DPP shifts; the row's last lane holds the chunk's counts.
// Dl > 0 (the synchronous merge's early verdict): k_fpart's long-group test is made here,
// on the input itself (the timestamp Dl chunks later, one more load per chunk), so that
// the host learns it right behind this kernel and launches the windows that hold the
// groups (smx_compose.hip enqueue_async); f_fail = F_LONG and long_host[0] = 1.
__global__ void __launch_bounds__(KH_NT) k_khist(const u8* __restrict__ kind, const u64* __restrict__ ts,
                                                 i64 na, i64 nb, i64 bgap, i64 CM, u32* __restrict__ cnt,
                                                 u64* __restrict__ sA, u64* __restrict__ sB, ComposeMeta* meta,
                                                 u32* long_host, i64 Dl) {
  __shared__ u32 c[CH_PER_BLOCK * KH_R][SMX_N_KINDS];
  __shared__ u32 km[2];
  __shared__ u32 lgb;  // the block saw a group longer than a window (Dl)
  const i64 CA = SMX_CEIL_DIV(na, (i64)CH), CB = SMX_CEIL_DIV(nb, (i64)CH);
  const int j = threadIdx.x / 16, q = threadIdx.x % 16;
  if (threadIdx.x < 2) km[threadIdx.x] = 0;
  if (threadIdx.x == 0) lgb = 0;
  // KH_R rounds of CH_PER_BLOCK chunks per block; every round's loads are issued first
  u32 w[KH_R][4];
  int nvr[KH_R];
  // timestamp samples for k_fpart: first op of each A chunk, last op of each full B chunk
  // (stored after the counting: their loads then wait beside the kind bytes', not ahead of
  // them; separate registers for A and B, or the second load waits on the first)
  u64 smpA[KH_R], smpB[KH_R], farA[KH_R], farB[KH_R];  // (far: the sample Dl chunks later)
  u64* atA[KH_R];
  u64* atB[KH_R];
  bool chkA[KH_R], chkB[KH_R];
#pragma unroll
  for (int rd = 0; rd < KH_R; ++rd) {
    const i64 g = ((i64)blockIdx.x * KH_R + rd) * CH_PER_BLOCK + j;
    const int side = g >= CA;
    const i64 cc = side ? g - CA : g;
    const i64 len = side ? nb : na;
    const i64 r0 = cc * CH + q * 16;  // branch position of this lane's first byte
    const int nv = g < CA + CB ? (int)(len - r0 < 0 ? 0 : (len - r0 < 16 ? len - r0 : 16)) : 0;
    nvr[rd] = nv;
    const u8* src = kind + (side ? na + bgap : 0) + r0;
    w[rd][0] = w[rd][1] = w[rd][2] = w[rd][3] = 0u;
    if (nv == 16 && (reinterpret_cast<uintptr_t>(src) & 15) == 0) {
      const uint4 v = *reinterpret_cast<const uint4*>(src);
      w[rd][0] = v.x; w[rd][1] = v.y; w[rd][2] = v.z; w[rd][3] = v.w;
    } else {
#pragma unroll
      for (int y = 0; y < 16; ++y)
        if (y < nv) w[rd][y >> 2] |= (u32)src[y] << (8 * (y & 3));
    }
    atA[rd] = atB[rd] = nullptr;
    smpA[rd] = smpB[rd] = farA[rd] = farB[rd] = 0;
    chkA[rd] = chkB[rd] = false;
    if (g < CA + CB) {
      if (!side && q == 0) {
        atA[rd] = sA + cc;
        smpA[rd] = ts[cc * CH];
        if (Dl > 0 && cc + Dl < CA) {
          chkA[rd] = true;
          farA[rd] = ts[(cc + Dl) * CH];
        }
      }
      if (side && q == 15 && nv == 16) {
        atB[rd] = sB + cc;
        smpB[rd] = ts[na + bgap + cc * CH + CH - 1];
        if (Dl > 0 && cc + Dl < nb / CH) {  // (B samples: last ops of full chunks)
          chkB[rd] = true;
          farB[rd] = ts[na + bgap + (cc + Dl) * CH + CH - 1];
        }
      }
    }
  }
  bool bad = false;
#pragma unroll
  for (int rd = 0; rd < KH_R; ++rd) {
    const int nv = nvr[rd];
    u32 pk[3] = {0u, 0u, 0u};  // kind k: bits 5 * (k % 6) of word k / 6
#pragma unroll
    for (int y = 0; y < 16; ++y) {
      if (y >= nv) break;
      u32 k = (w[rd][y >> 2] >> (8 * (y & 3))) & 0xffu;
      bad |= k >= SMX_N_KINDS;
      k = k < SMX_N_KINDS ? k : SMX_N_KINDS - 1;
      const u32 wd = (k * 43u) >> 8;  // k / 6 for k < 18
      const u32 inc = 1u << (5u * (k - 6u * wd));
      pk[0] += wd == 0 ? inc : 0u;
      pk[1] += wd == 1 ? inc : 0u;
      pk[2] += wd == 2 ? inc : 0u;
    }
    // 10-bit fields (a chunk count is at most 256), three kinds per word; row sums
    u32 f[6];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      f[2 * i] = (pk[i] & 31u) | ((pk[i] >> 5) & 31u) << 10 | ((pk[i] >> 10) & 31u) << 20;
      f[2 * i + 1] = ((pk[i] >> 15) & 31u) | ((pk[i] >> 20) & 31u) << 10 | ((pk[i] >> 25) & 31u) << 20;
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      u32 v = f[i];
      v += dpp_u32<0x111, 0xf>(v);  // row_shr:1
      v += dpp_u32<0x112, 0xf>(v);  // row_shr:2
      v += dpp_u32<0x114, 0xf>(v);  // row_shr:4
      v += dpp_u32<0x118, 0xf>(v);  // row_shr:8
      f[i] = v;
    }
    if (q == 15) {
#pragma unroll
      for (int k = 0; k < SMX_N_KINDS; ++k) c[rd * CH_PER_BLOCK + j][k] = (f[k / 3] >> (10 * (k % 3))) & 1023u;
    }
  }
  bool lg = false;
#pragma unroll
  for (int rd = 0; rd < KH_R; ++rd) {
    if (atA[rd]) *atA[rd] = smpA[rd];
    if (atB[rd]) *atB[rd] = smpB[rd];
    lg |= (chkA[rd] && farA[rd] == smpA[rd]) || (chkB[rd] && farB[rd] == smpB[rd]);
  }
  // a sample equal to the one Dl chunks (one window capacity) later: that timestamp group
  // alone overflows a window (k_fpart's test); published below, once per
  // block, and to the host by the one block whose atomic set it (thousands of waves
  // storing to the pinned flag over the bus slowed this kernel and its completion)
  if (__ballot(lg) && (threadIdx.x & (WAVE - 1)) == 0) atomicOr(&lgb, 1u);
  if (__ballot(bad) && (threadIdx.x & (WAVE - 1)) == 0) {
    meta->bad_sym = 1;
    if (long_host) __hip_atomic_store(long_host + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  __syncthreads();
  if (threadIdx.x == 0 && lgb &&
      (__hip_atomic_load(&meta->f_fail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & F_LONG) != F_LONG) {
    const u64 was = atomicOr((unsigned long long*)&meta->f_fail, F_LONG);
    if ((was & F_LONG) != F_LONG && long_host)
      __hip_atomic_store(long_host, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  // column-major output: consecutive threads write consecutive chunks of one column;
  // the kinds present per branch (the scans skip the all-zero columns)
  u32 m0 = 0, m1 = 0;
  for (int i = threadIdx.x; i < CH_PER_BLOCK * KH_R * SMX_N_KINDS; i += KH_NT) {
    const int jj = i % (CH_PER_BLOCK * KH_R), k = i / (CH_PER_BLOCK * KH_R);
    const i64 gg = (i64)blockIdx.x * CH_PER_BLOCK * KH_R + jj;
    if (gg >= CA + CB) continue;
    const int sd = gg >= CA;
    const u32 v = c[jj][k];
    cnt[((i64)sd * SMX_N_KINDS + k) * CM + (sd ? gg - CA : gg)] = v;
    if (v) (sd ? m1 : m0) |= 1u << k;
  }
  m0 = wave_or_to_last(m0);
  m1 = wave_or_to_last(m1);
  if ((threadIdx.x & (WAVE - 1)) == WAVE - 1) {
    if (m0) atomicOr(&km[0], m0);
    if (m1) atomicOr(&km[1], m1);
  }
  __syncthreads();
  // published only when it adds bits (a stale read costs a redundant atomic): the
  // blocks would otherwise serialise on two words
  if (threadIdx.x < 2 && km[threadIdx.x]) {
    const u32 cur = __hip_atomic_load(&meta->kmask[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if ((cur | km[threadIdx.x]) != cur) atomicOr(&meta->kmask[threadIdx.x], km[threadIdx.x]);
  }
}

__device__ __forceinline__ bool cs_present(const ComposeMeta* meta, int col) {
  return (meta->kmask[col >= SMX_N_KINDS] >> (col % SMX_N_KINDS)) & 1u;
}

// Exclusive scan of each (side, kind) column of chunk counts in three fully
// parallel phases over tiles of CS_TILE chunks: tile sums; scan of the tile sums
// (+ column totals into meta); tile scans.
#define CS_TILE (BLOCK * 8)

__global__ void __launch_bounds__(BLOCK) k_cscan_up(const u32* __restrict__ cnt, i64 na, i64 nb, i64 CM,
                                                    i64 NT, u32* __restrict__ tsum, const ComposeMeta* meta) {
  __shared__ u32 s[NWAVES + 1];
  const int col = blockIdx.y;
  if (!cs_present(meta, col)) return;  // all-zero column: its prefixes are its counts
  const i64 C = SMX_CEIL_DIV(col >= SMX_N_KINDS ? nb : na, (i64)CH);
  const i64 t0 = (i64)blockIdx.x * CS_TILE;
  if (t0 >= C) return;
  const u32* colp = cnt + (i64)col * CM;
  const i64 b = t0 + (i64)threadIdx.x * 8;
  u32 acc = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) acc += b + j < C ? colp[b + j] : 0u;
  u32 tot;
  block_excl_scan<OpSum, u32>(acc, s, &tot);
  if (threadIdx.x == 0) tsum[(i64)col * NT + blockIdx.x] = tot;
}

// The window count the plan's windows read (meta->n_win): nwin, or after an early
// F_LONG (k_khist) with the wide boundaries in place (nwin_long > 0, k_fpart's LongW) the
// wide plan's -- and F_LONG is cleared so the wide windows and the tail run.
__device__ __forceinline__ void set_n_win(ComposeMeta* meta, u64 nwin, u64 nwin_long) {
  if (nwin_long && meta->f_fail == F_LONG) {
    meta->f_fail = 0;
    nwin = nwin_long;
  }
  meta->n_win = nwin;
}

__global__ void __launch_bounds__(BLOCK) k_cscan_mid(u32* __restrict__ tsum, i64 na, i64 nb, i64 CM, i64 NT,
                                                     u32* __restrict__ cnt, ComposeMeta* meta, u64 nwin,
                                                     u64 nwin_long) {
  __shared__ u32 s[NWAVES + 1];
  const int col = blockIdx.x;
  const int side = col / SMX_N_KINDS, k = col % SMX_N_KINDS;
  const i64 C = SMX_CEIL_DIV(side ? nb : na, (i64)CH);
  const i64 nt = cs_present(meta, col) ? SMX_CEIL_DIV(C, (i64)CS_TILE) : 0;  // (absent: total 0)
  u32 carry = 0;
  for (i64 r0 = 0; r0 < nt; r0 += BLOCK) {
    const i64 r = r0 + threadIdx.x;
    const u32 v = r < nt ? tsum[(i64)col * NT + r] : 0u;
    u32 tot;
    const u32 ex = block_excl_scan<OpSum, u32>(v, s, &tot);
    if (r < nt) tsum[(i64)col * NT + r] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0) {
    cnt[(i64)col * CM + C] = carry;  // prefix at the end of the branch (a window may start there)
    atomicAdd((unsigned long long*)&meta->kcnt[k], (unsigned long long)carry);
    if (k == KREN) meta->n_ren_side[side] = carry;
    // the last column's block: the T-order segment starts (k_bases), from every total
    __threadfence();
    if (atomicAdd((unsigned long long*)&meta->cs_done, 1ull) == (unsigned long long)gridDim.x - 1) {
      __threadfence();
      set_n_win(meta, nwin, nwin_long);
      u64 acc = 0;
      for (int kk = 0; kk < SMX_N_KINDS; ++kk) {
        meta->base[kk] = acc;
        acc += __hip_atomic_load(&meta->kcnt[kk], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      meta->base[SMX_N_KINDS] = acc;
    }
  }
}

__global__ void __launch_bounds__(BLOCK) k_cscan_down(u32* __restrict__ cnt, i64 na, i64 nb, i64 CM, i64 NT,
                                                      const u32* __restrict__ tsum, const ComposeMeta* meta) {
  __shared__ u32 s[NWAVES + 1];
  const int col = blockIdx.y;
  if (!cs_present(meta, col)) return;
  const i64 C = SMX_CEIL_DIV(col >= SMX_N_KINDS ? nb : na, (i64)CH);
  const i64 t0 = (i64)blockIdx.x * CS_TILE;
  if (t0 >= C) return;
  u32* colp = cnt + (i64)col * CM;
  const i64 b = t0 + (i64)threadIdx.x * 8;
  u32 v[8];
  u32 acc = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    v[j] = b + j < C ? colp[b + j] : 0u;
    acc += v[j];
  }
  u32 tot;
  u32 run = tsum[(i64)col * NT + blockIdx.x] + block_excl_scan<OpSum, u32>(acc, s, &tot);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    if (b + j < C) colp[b + j] = run;
    run += v[j];
  }
}

// Small merges (CM <= CS_SMALL_CM chunks per branch): each (side, kind) column scanned by
// one block in one launch (k_cscan_up / mid / down are three launch latencies); the
// totals and, in the last column's block, the T-order segment starts as in k_cscan_mid.
#ifndef CS_SMALL_CM
#define CS_SMALL_CM 16384
#endif
__device__ __forceinline__ void cscan_small_body(u32* __restrict__ cnt, i64 na, i64 nb, i64 CM, ComposeMeta* meta,
                                                 u64 nwin, int col, u32* s, u64 nwin_long = 0) {
  const int side = col / SMX_N_KINDS, k = col % SMX_N_KINDS;
  const i64 C = SMX_CEIL_DIV(side ? nb : na, (i64)CH);
  u32* colp = cnt + (i64)col * CM;
  u32 carry = 0;
  if (cs_present(meta, col)) {  // (an absent column's prefixes are its zero counts)
    for (i64 t0 = 0; t0 < C; t0 += CS_TILE) {
      const i64 b = t0 + (i64)threadIdx.x * 8;
      u32 v[8];
      u32 acc = 0;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        v[j] = b + j < C ? colp[b + j] : 0u;
        acc += v[j];
      }
      u32 tot;
      u32 run = carry + block_excl_scan<OpSum, u32>(acc, s, &tot);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (b + j < C) colp[b + j] = run;
        run += v[j];
      }
      carry += tot;
    }
  }
  if (threadIdx.x == 0) {
    colp[C] = carry;  // prefix at the end of the branch (a window may start there)
    atomicAdd((unsigned long long*)&meta->kcnt[k], (unsigned long long)carry);
    if (k == KREN) meta->n_ren_side[side] = carry;
    __threadfence();
    if (atomicAdd((unsigned long long*)&meta->cs_done, 1ull) == (unsigned long long)(2 * SMX_N_KINDS - 1)) {
      __threadfence();
      set_n_win(meta, nwin, nwin_long);
      u64 acc = 0;
      for (int kk = 0; kk < SMX_N_KINDS; ++kk) {
        meta->base[kk] = acc;
        acc += __hip_atomic_load(&meta->kcnt[kk], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      meta->base[SMX_N_KINDS] = acc;
    }
  }
}
__global__ void __launch_bounds__(BLOCK) k_cscan_small(u32* __restrict__ cnt, i64 na, i64 nb, i64 CM,
                                                       ComposeMeta* meta, u64 nwin, u64 nwin_long) {
  __shared__ u32 s[NWAVES + 1];
  cscan_small_body(cnt, na, nb, CM, meta, nwin, blockIdx.x, s, nwin_long);
}
// Small merges (launch-bound): k_fpart and k_cscan_small are independent (both read
// only k_khist's outputs), so one launch runs both: the first nfp blocks are k_fpart's,
// the last 2 * SMX_N_KINDS k_cscan_small's columns.
__global__ void __launch_bounds__(BLOCK) k_fpart_cscan(const u64* __restrict__ ts, const u64* __restrict__ tsB,
                                                       const u64* __restrict__ sA, const u64* __restrict__ sB, i64 na,
                                                       i64 nb, i64 W, i64 tgt, i64 D, i64* __restrict__ bnd,
                                                       ComposeMeta* meta, u32* long_host, u32* __restrict__ cnt,
                                                       i64 CM, i64 nfp) {
  __shared__ u32 s[NWAVES + 1];
  if ((i64)blockIdx.x < nfp) fpart_body(ts, tsB, sA, sB, na, nb, W, tgt, D, bnd, meta, long_host, blockIdx.x, nfp);
  else cscan_small_body(cnt, na, nb, CM, meta, (u64)W, (int)(blockIdx.x - nfp), s);
}

// Per-window counts: each kind and renames per branch (+ moves with a None value
// in the generic layout).  Column-major [c][W].
//  * presorted layout (perm == nullptr): branch position j is op j; only the kind
//    bytes are read, 16 per lane (the layout itself is verified by k_window_f);
//  * generic layout: through the sort permutation, one op per lane.
__device__ __forceinline__ void wc_add_one(u32 k, u32 (&c)[SMX_N_KINDS], bool& bad) {
  bad |= k >= SMX_N_KINDS;
#pragma unroll
  for (int kk = 0; kk < SMX_N_KINDS; ++kk) c[kk] += (k == (u32)kk);
}

__device__ __forceinline__ void wc_add_bytes(u32 x, u32 (&c)[SMX_N_KINDS], bool& bad) {
#pragma unroll
  for (int q = 0; q < 4; ++q) wc_add_one((x >> (8 * q)) & 0xffu, c, bad);
}

#ifndef WC_NT
#define WC_NT BLOCK  // threads per generic window in k_wcount
#endif
__global__ void __launch_bounds__(WC_NT) k_wcount(const u8* __restrict__ kind, const i32* __restrict__ v0,
                                                  const i32* __restrict__ v1, const u32* __restrict__ perm,
                                                  const i64* __restrict__ bnd, i64 na, i64 W,
                                                  u32* __restrict__ wcnt, ComposeMeta* meta) {
  __shared__ u32 c[NCNT];
  if (perm != nullptr && meta->f_fail) return;  // the segmented sort failed: perm is not written
  const i64 w = xcd_item(blockIdx.x, W);  // (the window's gathers stay in one L2)
  if (threadIdx.x < NCNT) c[threadIdx.x] = 0;
  __syncthreads();
  const i64 a0 = bnd[2 * w], b0 = bnd[2 * w + 1], a1 = bnd[2 * w + 2], b1 = bnd[2 * w + 3];
  bool bad = false;
  if (perm == nullptr) {
    for (int side = 0; side < 2; ++side) {
      const i64 off = side ? na : 0;
      const i64 lo = off + (side ? b0 : a0), hi = off + (side ? b1 : a1);
      if (hi <= lo) continue;
      u32 cnt[SMX_N_KINDS];
#pragma unroll
      for (int kk = 0; kk < SMX_N_KINDS; ++kk) cnt[kk] = 0;
      const i64 alo = (lo + 15) & ~(i64)15, ahi = hi & ~(i64)15;
      if (alo >= ahi) {  // short range: bytes
        for (i64 j = lo + threadIdx.x; j < hi; j += WC_NT) wc_add_one(kind[j], cnt, bad);
      } else {
        for (i64 j = lo + threadIdx.x; j < alo; j += WC_NT) wc_add_one(kind[j], cnt, bad);
        for (i64 j = ahi + threadIdx.x; j < hi; j += WC_NT) wc_add_one(kind[j], cnt, bad);
        const uint4* v = (const uint4*)(kind + alo);
        for (i64 q = threadIdx.x; q < (ahi - alo) / 16; q += WC_NT) {
          const uint4 x = v[q];
          wc_add_bytes(x.x, cnt, bad);
          wc_add_bytes(x.y, cnt, bad);
          wc_add_bytes(x.z, cnt, bad);
          wc_add_bytes(x.w, cnt, bad);
        }
      }
#pragma unroll
      for (int kk = 0; kk < SMX_N_KINDS; ++kk) {
        const u32 tot = wave_incl_sum(cnt[kk]);
        if ((threadIdx.x & (WAVE - 1)) == WAVE - 1 && tot) {
          atomicAdd(&c[kk], tot);
          if (kk == KREN) atomicAdd(&c[CNT_REN_A + side], tot);
        }
      }
    }
  } else {
    // a window holds at most WG_CAP ops: WC_ITEMS per thread, every load issued before
    // any is used (the perm -> kind -> value chain is one round trip per level, not one
    // per item); the item count is fixed, so the ballots stay wave-uniform
    constexpr int WC_ITEMS = (WG_CAP + WC_NT - 1) / WC_NT;
    const u64 lt = lanemask_lt();
    const i64 nA = a1 - a0, nW = nA + (b1 - b0);
    u32 src[WC_ITEMS], kv[WC_ITEMS];
    i32 x0[WC_ITEMS], x1[WC_ITEMS];
    bool val[WC_ITEMS], sd[WC_ITEMS];
#pragma unroll
    for (int i = 0; i < WC_ITEMS; ++i) {
      const i64 e = (i64)i * WC_NT + threadIdx.x;
      val[i] = e < nW && e < WG_CAP;
      sd[i] = e >= nA;
      src[i] = val[i] ? perm[sd[i] ? na + b0 + (e - nA) : a0 + e] : 0u;
    }
#pragma unroll
    for (int i = 0; i < WC_ITEMS; ++i) kv[i] = kind[src[i]];
#pragma unroll
    for (int i = 0; i < WC_ITEMS; ++i) {  // the values of the moves only
      const bool mv = val[i] && kv[i] == KMOVE;
      x0[i] = mv ? v0[src[i]] : 0;
      x1[i] = mv ? v1[src[i]] : 0;
    }
#pragma unroll
    for (int i = 0; i < WC_ITEMS; ++i) {
      u32 k = 0;
      bool none_mv = false;
      if (val[i]) {
        bad |= kv[i] >= SMX_N_KINDS;
        k = kv[i] < SMX_N_KINDS ? kv[i] : SMX_N_KINDS - 1;
        none_mv = k == KMOVE && (x0[i] < 0 || x1[i] < 0);
      }
      const u64 peers = wave_peers<5>(k, val[i]);
      if (val[i] && (peers & lt) == 0) atomicAdd(&c[k], (u32)__popcll(peers));
      const u64 nm = __ballot(none_mv);
      if (nm && (threadIdx.x & (WAVE - 1)) == 0) atomicAdd(&c[CNT_NONE_MV], (u32)__popcll(nm));
      // renames per branch (a wave may straddle the A/B boundary: split the peers)
      if (val[i] && k == KREN) {
        const u64 sb = __ballot(sd[i]);
        const u64 mine = peers & (sd[i] ? sb : ~sb);
        if ((mine & lt) == 0) atomicAdd(&c[CNT_REN_A + (sd[i] ? 1 : 0)], (u32)__popcll(mine));
      }
    }
    if (nW > WG_CAP) bad = true;  // cannot happen: k_gpart cuts windows of at most WG_CAP ops
  }
  if (bad) meta->bad_sym = 1;
  __syncthreads();
  if (threadIdx.x < NCNT) wcnt[(i64)threadIdx.x * W + w] = c[threadIdx.x];
}

// Exclusive scan of each count column over windows; column totals into meta.
__global__ void __launch_bounds__(BLOCK) k_wscan(const u32* __restrict__ wcnt, u32* __restrict__ woff,
                                                 i64 W, ComposeMeta* meta) {
  __shared__ u32 s[NWAVES + 1];
  const int c = blockIdx.x;
  const u32* in = wcnt + (i64)c * W;
  u32* out = woff + (i64)c * W;
  u32 carry = 0;
  for (i64 r0 = 0; r0 < W; r0 += BLOCK * 8) {
    const i64 b = r0 + (i64)threadIdx.x * 8;
    u32 v[8];
    u32 acc = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      v[j] = b + j < W ? in[b + j] : 0u;
      acc += v[j];
    }
    u32 tot;
    u32 run = carry + block_excl_scan<OpSum, u32>(acc, s, &tot);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (b + j < W) out[b + j] = run;
      run += v[j];
    }
    carry += tot;
  }
  if (threadIdx.x == 0) {
    if (c < SMX_N_KINDS) meta->kcnt[c] = carry;
    else if (c == CNT_REN_A) meta->n_ren_side[0] = carry;
    else if (c == CNT_REN_B) meta->n_ren_side[1] = carry;
    else meta->n_move_none = carry;
  }
}

// T bases: exclusive prefix of the kind totals; the plan's window count.
__global__ void k_bases(ComposeMeta* meta, u64 nwin) {
  meta->n_win = nwin;
  u64 acc = 0;
  for (int k = 0; k < SMX_N_KINDS; ++k) {
    meta->base[k] = acc;
    acc += meta->kcnt[k];
  }
  meta->base[SMX_N_KINDS] = acc;
}

// ---------------------------------------------------------------------------
// kernels: generic path helpers

__global__ void k_gather_init(const u64* __restrict__ key, u64* __restrict__ kout, u32* __restrict__ vout,
                              i64 n) {
  for (i64 i = (i64)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (i64)gridDim.x * BLOCK) {
    kout[i] = key[i];
    vout[i] = (u32)i;
  }
}

__global__ void k_gather(const u64* __restrict__ key, const u32* __restrict__ idx, u64* __restrict__ kout,
                         i64 n) {
  for (i64 i = (i64)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (i64)gridDim.x * BLOCK)
    kout[i] = key[idx[i]];
}

// Two columns gathered through one read of the permutation.
__global__ void k_gather2(const u64* __restrict__ a, const u64* __restrict__ b, const u32* __restrict__ idx,
                          u64* __restrict__ aout, u64* __restrict__ bout, i64 n) {
  for (i64 i = (i64)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (i64)gridDim.x * BLOCK) {
    const u32 j = idx[i];
    aout[i] = a[j];
    bout[i] = b[j];
  }
}

__global__ void k_offset(u32* __restrict__ v, i64 n, u32 off) {
  for (i64 i = (i64)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (i64)gridDim.x * BLOCK) v[i] += off;
}
