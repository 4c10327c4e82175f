// smx_rga_list.h -- the replay of one list: a wave per list in LDS, a workgroup per list in
// global memory for the long ones.  Part of the smx_rga.hip unit: included once, there.
#pragma once

__device__ __forceinline__ u32 rga_lend(const u32* lstart, u32 l, i64 nl, i64 n) {
  return l + 1 < nl ? lstart[l + 1] : (u32)n;
}
// Where the list kernels' events come from.  RGA_SRC_LISTS: the lists of smx_rga_replay.
// RGA_SRC_ONTO (smx_rga_replay_onto) and RGA_SRC_CHAIN (smx_rga_replay_chain): a "list" is a
// job, lstart the jobs' slice starts, nl + 1 of them (smx_rga_onto.h, smx_rga_chain.h: the
// total is known on the device alone)
enum { RGA_SRC_LISTS = 0, RGA_SRC_ONTO = 1, RGA_SRC_CHAIN = 2 };
template <int SRC>
__device__ __forceinline__ u32 rga_lend_of(const u32* lstart, u32 l, i64 nl, i64 n) {
  if constexpr (SRC != RGA_SRC_LISTS) return lstart[l + 1];
  else return rga_lend(lstart, l, nl, n);
}

// A list's survivor count, and its share of its chunk's sum: the RGA_CS_MAX chunk
// sums sit just before scnt (rga_layout); k_rga_out adds them up to its list's offset.
__device__ __forceinline__ void rga_put_count(u32* scnt, u32 l, u32 m) {
  scnt[l] = m;
  if (l < RGA_FUSED_MAX) atomicAdd(scnt - RGA_CS_MAX + (l / RGA_CS_LISTS), m);  // (more lists: scan_excl)
}

// Events ia, ib (stream indices) whose record words 0 are equal: the rest of the
// crdt.py:48-57 key -- t (signed), author, opid -- then the creation index.
__device__ __forceinline__ bool rga_key_lt(const smx_rga_ops& o, u32 ia, u32 ib) {
  const i64 ta = o.t[ia], tb = o.t[ib];
  if (ta != tb) return ta < tb;
  const u32 aa = o.author[ia], ab = o.author[ib];
  if (aa != ab) return aa < ab;
  const u64 ha = (u64)o.opid_hi[ia], hb = (u64)o.opid_hi[ib];
  if (ha != hb) return ha < hb;
  const u64 la = (u64)o.opid_lo[ia], lb = (u64)o.opid_lo[ib];
  if (la != lb) return la < lb;
  return ia < ib;
}

// record a before record b in (key, creation index) order
__device__ __forceinline__ bool rec_lt(const u64* a, const u64* b, const smx_rga_ops& o) {
  if (a[0] != b[0]) return a[0] < b[0];
  return rga_key_lt(o, (u32)a[RGA_WV] & RGA_IDX_MASK, (u32)b[RGA_WV] & RGA_IDX_MASK);
}

// ---------------------------------------------------------------------------
// Lists of at most RW_CAP events: one wave per list, no block barriers.  Lane x owns
// the list's events x, x + 64, ... (K = ceil(cnt / 64) of them; the partition keeps
// each list's events in stream order, so event position = creation order).
//  1. value groups by an LDS hash table (CAS insert, a member chain per group);
//  2. the lane that inserted a group's value replays the group in stream order
//     (crdt.py:29-43);
//  3. the survivors, compacted, ordered by key word 0 with an in-register bitonic
//     network (DPP / swizzle lane exchanges); runs of equal word 0 are re-sorted on
//     the rest of the key and the index (crdt.py:45-57).
#define RW_CAP 256   // k_rga_wave; the deferred lists' kernel takes up to 2 * RW_CAP
#define RW_WAVES 2   // lists per block
#ifndef RW_PER_CU
#define RW_PER_CU 16  // k_rga_wave workgroups per CU (persistent; 0: one wave per list)
#endif
#define RW_EMPTY 0xffffffffu
#define RW_NIL 0xffffu
#define RW_DEAD 0x400u
#define RW_MOP 12       // member entries: event | op << RW_MOP
#define RW_MEV 0xfffu
#define RW_HT u16  // 16-bit group counts / bases (a list has at most 2 * RW_CAP events): less LDS per wave
#ifndef RW_OCC_W
#define RW_OCC_W 8  // k_rga_wave: registers for this many waves per SIMD (0: compiler's choice)
#endif
#if RW_OCC_W
#define RW_OCC __attribute__((amdgpu_waves_per_eu(RW_OCC_W, RW_OCC_W)))
#else
#define RW_OCC
#endif
#ifndef RW_PINS_K
#define RW_PINS_K 16  // lists of K >= this: a lane's K hash inserts probed together (off: for
                      // k_rga_wave's K = 4 0.563 -> 0.576 ms; k_rga_wave2's K = 8 26.9 us either way)
#endif
#ifndef RW_ABL
#define RW_ABL 0  // timing ablations (wrong results): bit0 no replay, bit1 no grouping / replay,
                  // bit2 no key order, bit3 load only
#endif

template <int CAP>
struct RwLds {
  static constexpr int cap = CAP;
  // hash slots: one per event for k_rga_wave's lists (7.4 KB of LDS per list, five
  // waves per SIMD; a full table still terminates, every value finds its slot), two
  // per event otherwise
  static constexpr int HT = CAP == RW_CAP ? CAP : 2 * CAP;
  u64 wv[CAP];          // value << 32 | op << 30 | index (record word RGA_WV)
  union {
    struct {
      u32 hkey[HT];     // the slot's value, RW_EMPTY
      RW_HT hcnt[HT];   // members of the slot's group
      RW_HT hbase[HT];  // first member position (exclusive scan of hcnt)
    } h;
    u64 gs[CAP];        // step 3: survivors' word 0, sorted
  };
  union {               // (mem is dead once the groups are replayed)
    u16 mem[CAP];       // group members, group by group, each in event order (| op << RW_MOP)
    u16 gp[CAP];        // step 3: survivors' events, sorted
  };
  u8 st[CAP];           // bit0 present, bit1 tombstoned
};

// Where a list kernel reads its events' record words (event e of the list at s0):
//  RecSrc  the partitioned 16-byte records
//  ColSrc  the input columns themselves (SMX_RGA_GROUPED: event s0 + e is the list's e-th
//          event, so word 0 = anchor << 32 | t' >> 32 and word 1 = value << 32 | op << 30 |
//          index are built at the load, no record pass)
//  OntoSrc the input columns, for a job of smx_rga_replay_onto: its first lb events are
//          its base's (columns b0 ...), the others its own (columns dq + lb ...); the words
//          as ColSrc builds them, the index being the column.  An op > 2 raises the error word.
//  ChainSrc the input columns, for a job of smx_rga_replay_chain: event e is column cm[e], cm
//          the job's part of the column map (k_rga_chain_map), one coalesced 4-byte load; the
//          words and the op check as OntoSrc's.
struct RecSrc {
  const u64* p;  // the list's first record
  __device__ __forceinline__ u64 w0(u32 e) const { return p[(u64)e * RGA_REC]; }
  __device__ __forceinline__ u64 w1(u32 e) const { return p[(u64)e * RGA_REC + RGA_WV]; }
};
struct ColSrc {
  const u32* anchor;
  const i64* t;
  const u32* value;
  const u8* op;
  u32 s0;
  __device__ __forceinline__ u64 w0(u32 e) const {
    const u32 j = s0 + e;
    return ((u64)anchor[j] << 32) | (((u64)t[j] ^ 0x8000000000000000ull) >> 32);
  }
  __device__ __forceinline__ u64 w1(u32 e) const {
    const u32 j = s0 + e, op3 = op[j];
    return ((u64)value[j] << 32) | ((op3 > 2 ? 0u : op3) << 30) | j;
  }
};

struct OntoSrc {
  const u32* anchor;
  const i64* t;
  const u32* value;
  const u8* op;
  i32* err;
  u32 b0, lb, dq;  // (dq = the first own column - lb, mod 2^32)
  __device__ __forceinline__ u32 col(u32 e) const { return e + (e < lb ? b0 : dq); }
  __device__ __forceinline__ u64 w0(u32 e) const {
    const u32 j = col(e);
    return ((u64)anchor[j] << 32) | (((u64)t[j] ^ 0x8000000000000000ull) >> 32);
  }
  __device__ __forceinline__ u64 w1(u32 e) const {
    const u32 j = col(e), op3 = op[j];
    if (op3 > 2) atomicOr(err, (i32)RGA_E_INPUT);
    return ((u64)value[j] << 32) | ((op3 > 2 ? 0u : op3) << 30) | j;
  }
};
// A job's source from its descriptor (k_rga_onto_jobs; kept where a batch keeps its list ids)
__device__ __forceinline__ OntoSrc rga_onto_src(const smx_rga_ops& o, u32 job, const i32* gate) {
  const uint4 d = reinterpret_cast<const uint4*>(o.list)[job];
  return OntoSrc{o.anchor, o.t, o.value, o.op, const_cast<i32*>(gate), d.x, d.y, d.z};
}

struct ChainSrc {
  const u32* anchor;
  const i64* t;
  const u32* value;
  const u8* op;
  i32* err;
  const u32* cm;  // the column of the job's event 0 (cmap + the job's slice start)
  __device__ __forceinline__ u32 col(u32 e) const { return cm[e]; }
  __device__ __forceinline__ u64 w0(u32 e) const {
    const u32 j = col(e);
    return ((u64)anchor[j] << 32) | (((u64)t[j] ^ 0x8000000000000000ull) >> 32);
  }
  __device__ __forceinline__ u64 w1(u32 e) const {
    const u32 j = col(e), op3 = op[j];
    if (op3 > 2) atomicOr(err, (i32)RGA_E_INPUT);
    return ((u64)value[j] << 32) | ((op3 > 2 ? 0u : op3) << 30) | j;
  }
};
// A job's source from the column map (kept where a batch keeps its list ids) and its slice start
__device__ __forceinline__ ChainSrc rga_chain_src(const smx_rga_ops& o, u32 s0, const i32* gate) {
  return ChainSrc{o.anchor, o.t, o.value, o.op, const_cast<i32*>(gate), o.list + s0};
}

// Event a before event b of one list in (key, index) order (crdt.py:48-57): word 0
// from LDS, the rest from the input columns by stream index (rare: equal word 0).
template <class LDS, class SRC>
__device__ __forceinline__ bool ev_lt(const LDS& S, const SRC& src, const smx_rga_ops& o, u32 a,
                                      u32 b) {
  const u64 wa = src.w0(a), wb = src.w0(b);  // (the list's records or columns, L2-resident)
  if (wa != wb) return wa < wb;
  return rga_key_lt(o, (u32)S.wv[a] & RGA_IDX_MASK, (u32)S.wv[b] & RGA_IDX_MASK);
}

// Step 3 over the survivors' (word 0, event) pairs held K2 per lane.
template <int K2, class LDS, class SRC>
__device__ __forceinline__ void rw_order(LDS& S, const SRC& src, const smx_rga_ops& o, u64 (&key)[8],
                                         u32 (&pay)[8], u32 m,
                                         u32 s0, u32 lane, u32* __restrict__ tmp_v, u32* __restrict__ tmp_s) {
  constexpr u32 N = 64u * K2;
  bool packed = false;
  {  // word 0 = anchor << 32 | t's top half.  When the survivors' anchor and t ranges fit
     // beside the event bits in 31 bits, sort (anchor - min, t - min, event) as one u32:
     // one lane exchange and a min / max per step instead of three exchanges and selects.
     // Equal packed fields <=> equal word 0, so the tie runs below are the same.
    constexpr u32 PB = LDS::cap <= 256 ? 8 : 9;  // event bits
    u32 amx = 0, anx = 0, tmx = 0, tnx = 0;
#pragma unroll
    for (int k = 0; k < K2; ++k)
      if ((u32)k * 64u + lane < m) {
        const u32 a = (u32)(key[k] >> 32), t = (u32)key[k];
        amx = max(amx, a);
        anx = max(anx, ~a);
        tmx = max(tmx, t);
        tnx = max(tnx, ~t);
      }
    amx = (u32)__builtin_amdgcn_readlane((int)wave_incl_max_u32(amx), WAVE - 1);
    anx = (u32)__builtin_amdgcn_readlane((int)wave_incl_max_u32(anx), WAVE - 1);
    tmx = (u32)__builtin_amdgcn_readlane((int)wave_incl_max_u32(tmx), WAVE - 1);
    tnx = (u32)__builtin_amdgcn_readlane((int)wave_incl_max_u32(tnx), WAVE - 1);
    const u32 amin = ~anx, tmin = ~tnx;
    const u32 ba = 32u - (u32)__clz((int)(amx - amin)), bt = 32u - (u32)__clz((int)(tmx - tmin));
    if (m > 0 && ba + bt + PB <= 31u) {
      packed = true;
      u32 pk[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) pk[k] = ~0u;
#pragma unroll
      for (int k = 0; k < K2; ++k)
        if ((u32)k * 64u + lane < m)
          pk[k] = (((u32)(key[k] >> 32) - amin) << (bt + PB)) | (((u32)key[k] - tmin) << PB) | pay[k];
      wave_bitonic32<K2>(pk, lane);
#pragma unroll
      for (int k = 0; k < K2; ++k) {
        const bool v = (u32)k * 64u + lane < m;
        key[k] = v ? (u64)(pk[k] >> PB) : ~0ull;
        pay[k] = v ? pk[k] & ((1u << PB) - 1u) : RW_DEAD;
      }
    }
  }
  if (!packed) wave_bitonic<K2>(key, pay, lane);
#pragma unroll
  for (int k = 0; k < K2; ++k) {
    const u32 q = (u32)k * 64u + lane;
    S.gs[q] = key[k];
    S.gp[q] = (u16)pay[k];
  }
  wave_lds_sync();
  auto tail_lt = [&](u32 b, u32 a) {  // events b, a with equal word 0; dead ones last
    if ((a | b) & RW_DEAD) return (a & RW_DEAD) && !(b & RW_DEAD);
    return ev_lt(S, src, o, b, a);
  };
#pragma unroll
  for (int k = 0; k < K2; ++k) {
    const u32 q = (u32)k * 64u + lane;
    if (q < m && q + 1 < N && S.gs[q + 1] == key[k] && (q == 0 || S.gs[q - 1] != key[k])) {
      u32 e = q + 2;  // the run [q, e) of equal word 0: insertion sort on the rest
      while (e < N && S.gs[e] == key[k]) ++e;
      for (u32 x = q + 1; x < e; ++x) {
        const u32 v = S.gp[x];
        u32 y = x;
        while (y > q && tail_lt(v, S.gp[y - 1])) {
          S.gp[y] = S.gp[y - 1];
          --y;
        }
        S.gp[y] = (u16)v;
      }
    }
  }
  wave_lds_sync();
  for (u32 q = lane; q < m; q += WAVE) {
    const u32 e = S.gp[q] & (RW_DEAD - 1);
    const u64 w = S.wv[e];
    tmp_v[s0 + q] = (u32)(w >> 32);
    tmp_s[s0 + q] = ((u32)w & RGA_IDX_MASK) | (S.st[e] & 2 ? RGA_TOMB_BIT : 0u);
  }
}

// tomb: list mode (crdt.py RGA.list) -- the tombstoned elements stay, flagged
// Returns the list's survivor count (wave-uniform); scnt[l] is the caller's to write.
template <int K, int CAP, class SRC>
__device__ __forceinline__ u32 rga_wave_list(const smx_rga_ops& o, const SRC src, u32 l, u32 s0, u32 cnt,
                                              RwLds<CAP>& S, u32 lane, bool tomb,
                                              u32* __restrict__ tmp_v, u32* __restrict__ tmp_s,
                                              u32* __restrict__ scnt) {
  u64 w0r[K];  // word 0 of this lane's events k * 64 + lane, kept for step 3
  {  // every load in flight at once; word 1 of each event to LDS
    u64 wvr[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const u32 e = (u32)k * 64u + lane;
      w0r[k] = e < cnt ? src.w0(e) : ~0ull;
      wvr[k] = e < cnt ? src.w1(e) : 0ull;
    }
    for (u32 t = lane; t < RwLds<CAP>::HT; t += WAVE) {
      S.h.hkey[t] = RW_EMPTY;
      S.h.hcnt[t] = 0;
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const u32 e = (u32)k * 64u + lane;
      if (e < cnt) S.wv[e] = wvr[k];
    }
  }
  wave_lds_sync();
  if (RW_ABL & 8) return (u32)__builtin_amdgcn_readfirstlane((int)((u32)S.wv[lane] & 1u));
  const u64 lt = lane ? ~0ull >> (WAVE - lane) : 0ull;  // (from `lane`: see k_rga_wave)
  constexpr int HB = RwLds<CAP>::HT == 256 ? 8 : RwLds<CAP>::HT == 512 ? 9 : 10;  // log2 of the hash slots
  static_assert(RwLds<CAP>::HT == 1 << HB, "hash slots");
  u32 slot[8], rk[8], opk[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) slot[k] = rk[k] = opk[k] = 0;
  if (RW_ABL & 2) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const u32 e = (u32)k * 64u + lane;
      S.st[e] = e < cnt && ((u32)(S.wv[e] >> 30) & 3u) != 2;
    }
  } else {
    // 1. value groups: each event's value into the hash table (CAS), its rank among
    //    the group's events (match within the wave, running counts across slots),
    //    then the groups laid out contiguously, each in event order
    if constexpr (K >= RW_PINS_K) {
    {  // all K of a lane's events probe together: one round of K CASes in flight per
       // step instead of K dependent probe chains (the slot a group lands in does not
       // matter; its members' order comes from the ranks below)
      u32 v[K], pend = 0;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const u32 e = (u32)k * 64u + lane;
        S.st[e] = 0;
        v[k] = 0;
        if (e < cnt) {
          const u64 wv = S.wv[e];
          v[k] = (u32)(wv >> 32);
          opk[k] = (u32)(wv >> 30) & 3u;
          slot[k] = (v[k] * 0x9E3779B1u) >> (32 - HB);
          pend |= 1u << k;
        }
      }
      while (__ballot(pend != 0)) {
        u32 old[K];
#pragma unroll
        for (int k = 0; k < K; ++k) old[k] = (pend >> k) & 1u ? atomicCAS(&S.h.hkey[slot[k]], RW_EMPTY, v[k]) : 0u;
#pragma unroll
        for (int k = 0; k < K; ++k)
          if ((pend >> k) & 1u) {
            if (old[k] == RW_EMPTY || old[k] == v[k])
              pend &= ~(1u << k);
            else
              slot[k] = (slot[k] + 1) & (RwLds<CAP>::HT - 1);
          }
      }
    }
    } else {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const u32 e = (u32)k * 64u + lane;
      S.st[e] = 0;
      if (e < cnt) {
        const u64 wv = S.wv[e];
        const u32 v = (u32)(wv >> 32);
        opk[k] = (u32)(wv >> 30) & 3u;
        u32 h = (v * 0x9E3779B1u) >> (32 - HB);
        for (;;) {
          const u32 old = atomicCAS(&S.h.hkey[h], RW_EMPTY, v);
          if (old == RW_EMPTY || old == v) break;
          h = (h + 1) & (RwLds<CAP>::HT - 1);
        }
        slot[k] = h;
      }
    }
    }
    wave_lds_sync();
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const u32 e = (u32)k * 64u + lane;
      const bool valid = e < cnt;
      const u64 peers = wave_peers<HB>(slot[k], valid);
      const u32 base = valid ? S.h.hcnt[slot[k]] : 0u;
      rk[k] = base + (u32)__popcll(peers & lt);
      wave_lds_sync();
      if (valid && (peers & lt) == 0) S.h.hcnt[slot[k]] = (RW_HT)(base + (u32)__popcll(peers));
      wave_lds_sync();
    }
    {  // exclusive scan of the group sizes, HT / 64 slots per lane
      constexpr int PL = RwLds<CAP>::HT / WAVE;
      u32 c[PL], tot = 0;
#pragma unroll
      for (int i = 0; i < PL; ++i) {
        c[i] = S.h.hcnt[lane * PL + i];
        tot += c[i];
      }
      u32 run = wave_incl_sum(tot) - tot;
#pragma unroll
      for (int i = 0; i < PL; ++i) {
        S.h.hbase[lane * PL + i] = (RW_HT)run;
        run += c[i];
      }
    }
    wave_lds_sync();
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const u32 e = (u32)k * 64u + lane;
      if (e < cnt) S.mem[S.h.hbase[slot[k]] + rk[k]] = (u16)(e | opk[k] << RW_MOP);  // event, op
    }
    wave_lds_sync();
    // 2. the group's first event's lane replays the group in event order (crdt.py:29-43)
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const u32 e = (u32)k * 64u + lane;
      if (e >= cnt || rk[k] != 0) continue;
      const u32 b = S.h.hbase[slot[k]], c = S.h.hcnt[slot[k]];
      if (c == 1 || (RW_ABL & 1)) {
        S.st[e] = opk[k] != 2;
        continue;
      }
      for (u32 i = 0; i < c; ++i) {
        const u32 xm = S.mem[b + i];
        const u32 x = xm & RW_MEV, op = xm >> RW_MOP;
        if (op == 2) {  // delete: every present element is tombstoned; creates nothing
          for (u32 j = 0; j < i; ++j) {
            const u32 y = S.mem[b + j] & RW_MEV;
            if (S.st[y] & 1) S.st[y] |= 2;
          }
          continue;
        }
        if (op == 1) {  // move: pops the live element first in list order
          u32 best = RW_NIL;
          u64 wb = 0;  // best's word 0: read when a second candidate shows up, then kept
          bool wbl = false;
          for (u32 j = 0; j < i; ++j) {
            const u32 y = S.mem[b + j] & RW_MEV;
            if (S.st[y] != 1) continue;
            if (best == RW_NIL) {
              best = y;
              continue;
            }
            if (!wbl) {
              wb = src.w0(best);
              wbl = true;
            }
            const u64 wy = src.w0(y);
            if (wy < wb ||
                (wy == wb && rga_key_lt(o, (u32)S.wv[y] & RGA_IDX_MASK, (u32)S.wv[best] & RGA_IDX_MASK))) {
              best = y;
              wb = wy;
            }
          }
          if (best != RW_NIL) S.st[best] = 0;
        }
        S.st[x] = 1;
      }
    }
  }
  wave_lds_sync();
  // 3. survivors (event order) -> K2 (word 0, event) pairs per lane, ordered by key
  u32 m = 0;
  u64 key[8];
  u32 pay[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    key[k] = ~0ull;
    pay[k] = RW_DEAD;
  }
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const u32 e = (u32)k * 64u + lane;
    const bool live = e < cnt && (tomb ? (S.st[e] & 1) != 0 : S.st[e] == 1);
    const u64 ball = __ballot(live);
    if (live) {
      const u32 q = m + (u32)__popcll(ball & lt);
      S.gp[q] = (u16)e;
      S.gs[q] = w0r[k];  // (the hash table under gs is dead after step 2)
    }
    m += (u32)__popcll(ball);
  }
  wave_lds_sync();
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const u32 a = (u32)k * 64u + lane;
    if (a < m) {
      pay[k] = S.gp[a];
      key[k] = S.gs[a];
    }
  }
  wave_lds_sync();  // gp / the hash table are rewritten below
  if (RW_ABL & 4) {
    for (u32 q = lane; q < m; q += WAVE) {
      const u64 w = S.wv[S.gp[q]];
      tmp_v[s0 + q] = (u32)(w >> 32);
      tmp_s[s0 + q] = (u32)w & RGA_IDX_MASK;
    }
  } else if (m <= 64) {
    rw_order<1>(S, src, o, key, pay, m, s0, lane, tmp_v, tmp_s);
  } else if (m <= 128) {
    rw_order<2>(S, src, o, key, pay, m, s0, lane, tmp_v, tmp_s);
  } else if (K <= 4 || m <= 256) {
    rw_order<(K <= 4 ? K : 4)>(S, src, o, key, pay, m, s0, lane, tmp_v, tmp_s);
  } else {
    rw_order<8>(S, src, o, key, pay, m, s0, lane, tmp_v, tmp_s);
  }
  return m;
}

template <bool DIRECT, int SRC = RGA_SRC_LISTS>
__global__ void __launch_bounds__(WAVE * RW_WAVES) RW_OCC k_rga_wave(smx_rga_ops o, const u64* __restrict__ R,
                                                             const u32* __restrict__ lstart,
                                                             i64 n, i64 nl, u32* __restrict__ tmp_v,
                                                             u32* __restrict__ tmp_s, u32* __restrict__ scnt,
                                                             int tomb, const i32* __restrict__ gate) {
  __shared__ RwLds<RW_CAP> lds[RW_WAVES];
  if (*gate & RGA_E_UNGROUPED) return;  // (a grouped call whose list ids decrease: redone partitioned)
  const u32 lane = threadIdx.x & (WAVE - 1);
  // the wave index as a scalar: the list index, its bounds and the slice base stay in
  // SGPRs (scalar loads of lstart; LDS member offsets fold into the instructions)
  const u32 w = (u32)__builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE));
  // persistent (RW_PER_CU workgroups per CU): each wave takes a contiguous range of
  // lists and adds its survivors into the 256-list chunk sums once per chunk (one device
  // atomic per list on a shared chunk word serialized the waves, and the next list's
  // loads waited for it)
  const u32 nw = gridDim.x * RW_WAVES, wid = blockIdx.x * RW_WAVES + w;
  const u32 per = (u32)((nl + nw - 1) / nw);
  const u32 L0 = min((u64)wid * per, (u64)nl), L1 = min((u64)L0 + per, (u64)nl);
  u32 acc = 0;
  for (u32 l = L0; l < L1; ++l) {
    const u32 s0 = lstart[l], cnt = rga_lend_of<SRC>(lstart, l, nl, n) - s0;
    if (cnt <= RW_CAP) {  // (longer lists: k_rga_wave2 / k_rga_big count themselves)
      // the lane id laundered per list: otherwise the compiler hoists every lane-derived
      // constant of the list code out of the loop and keeps it live
      u32 ln = lane;
      asm volatile("v_mov_b32 %0, %1" : "=v"(ln) : "v"(lane));
      u32 m;
      auto run = [&](auto src) {
        if (cnt <= 64) return rga_wave_list<1>(o, src, l, s0, cnt, lds[w], ln, tomb != 0, tmp_v, tmp_s, scnt);
        if (cnt <= 128) return rga_wave_list<2>(o, src, l, s0, cnt, lds[w], ln, tomb != 0, tmp_v, tmp_s, scnt);
        return rga_wave_list<4>(o, src, l, s0, cnt, lds[w], ln, tomb != 0, tmp_v, tmp_s, scnt);
      };
      if constexpr (SRC == RGA_SRC_ONTO) m = run(rga_onto_src(o, l, gate));
      else if constexpr (SRC == RGA_SRC_CHAIN) m = run(rga_chain_src(o, s0, gate));
      else if constexpr (DIRECT) m = run(ColSrc{o.anchor, o.t, o.value, o.op, s0});
      else m = run(RecSrc{R + (u64)s0 * RGA_REC});
      if (lane == 0) scnt[l] = m;
      acc += m;
      wave_lds_sync();  // the next list reuses the slice
    }
    if ((l + 1) % RGA_CS_LISTS == 0 || l + 1 == L1) {
      if (lane == 0 && acc && l < RGA_FUSED_MAX) atomicAdd(scnt - RGA_CS_MAX + l / RGA_CS_LISTS, acc);
      acc = 0;
    }
  }
}

// A wave writes the records of a list's cnt events, read through cs, to rw.
template <class CS>
__device__ __forceinline__ void rw_records(const CS cs, u64* rw, u32 cnt, u32 lane) {
  for (u32 e = lane; e < cnt; e += WAVE) {
    R16 r;
    r.a = cs.w0(e);
    r.b = cs.w1(e);
    *reinterpret_cast<R16*>(rw + (u64)e * RGA_REC) = r;
  }
  __threadfence_block();  // (this wave reads them back; k_rga_big after this kernel)
}

// Lists of RW_CAP + 1 .. 2 * RW_CAP events: the same wave per list with twice the
// slots; longer ones go on to k_rga_big.  Each wave sweeps 64 lists at a time for the
// long ones itself (k_rga_wave skips them; no hand-off list).
template <int SRC = RGA_SRC_LISTS>
__global__ void __launch_bounds__(WAVE * RW_WAVES) k_rga_wave2(smx_rga_ops o, const u64* __restrict__ R,
                                                              const u32* __restrict__ lstart,
                                                              i64 n, i64 nl, u32* __restrict__ defer,
                                                              u32* __restrict__ ndefer, u32* __restrict__ tmp_v,
                                                              u32* __restrict__ tmp_s, u32* __restrict__ scnt,
                                                              int tomb, const i32* __restrict__ gate, int direct) {
  __shared__ RwLds<2 * RW_CAP> lds[RW_WAVES];
  if (*gate & RGA_E_UNGROUPED) return;
  const u32 lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
  const u64 nw = (u64)gridDim.x * RW_WAVES;
  for (u64 l0 = ((u64)blockIdx.x * RW_WAVES + w) * WAVE; l0 < (u64)nl; l0 += nw * WAVE) {
    const u64 me = l0 + lane;
    const u32 c = me < (u64)nl ? rga_lend_of<SRC>(lstart, (u32)me, nl, n) - lstart[me] : 0u;
    u64 todo = __ballot(c > RW_CAP);
    while (todo) {
      const u32 l = (u32)(l0 + (u64)(__ffsll((unsigned long long)todo) - 1));
      todo &= todo - 1;
      const u32 s0 = lstart[l], cnt = rga_lend_of<SRC>(lstart, l, nl, n) - s0;
      // no partition: a long list's or job's records from the columns, into its slice
      u64* rw = const_cast<u64*>(R) + (u64)s0 * RGA_REC;
      if constexpr (SRC == RGA_SRC_CHAIN) rw_records(rga_chain_src(o, s0, gate), rw, cnt, lane);
      else if constexpr (SRC == RGA_SRC_ONTO) rw_records(rga_onto_src(o, l, gate), rw, cnt, lane);
      else if (direct) rw_records(ColSrc{o.anchor, o.t, o.value, o.op, s0}, rw, cnt, lane);  // (grouped events)
      if (cnt > 2 * RW_CAP) {
        if (lane == 0) defer[atomicAdd(ndefer, 1u)] = l;
        continue;
      }
      const u32 m = rga_wave_list<8>(o, RecSrc{R + (u64)s0 * RGA_REC}, l, s0, cnt, lds[w], lane, tomb != 0, tmp_v, tmp_s, scnt);
      if (lane == 0) rga_put_count(scnt, l, m);
      wave_lds_sync();  // the next list reuses the slice
    }
  }
}

// Block-wide sort of the record positions p[0..cnt) by `less`, in global memory:
// the bitonic network in its all-ascending form (first stage of each merge compares
// i with its mirror i ^ (k - 1)), so positions past cnt act as +infinity and are
// never touched.
template <typename Less>
__device__ void block_sort_positions(u32* p, u32 cnt, Less less) {
  u32 P = 1;
  while (P < cnt) P <<= 1;
  for (u32 k = 2; k <= P; k <<= 1) {
    for (u32 j = k >> 1; j > 0; j >>= 1) {
      const u32 mask = j == (k >> 1) ? k - 1 : j;
      for (u32 i = threadIdx.x; i < P; i += blockDim.x) {
        const u32 q = i ^ mask;
        if (q > i && q < cnt && less(p[q], p[i])) {
          const u32 x = p[i];
          p[i] = p[q];
          p[q] = x;
        }
      }
      __syncthreads();
    }
  }
}

// Lists longer than 2 * RW_CAP: the same replay from global memory, one block per list
// (such lists are rare — a whole file's history in one list).  Per list, in its
// record range: gp = positions sorted by (value, index), bst = state by that order;
// then the survivors' positions sorted by (key, index).
template <int SRC>
__device__ void rga_big_list(const smx_rga_ops& o, const u64* __restrict__ R, u32 l, const u32* __restrict__ lstart, i64 n, i64 nl,
                             u8* __restrict__ bst, u32* __restrict__ gp, u32* __restrict__ tmp_v,
                             u32* __restrict__ tmp_s, u32* __restrict__ scnt, bool tomb) {
  __shared__ u32 ns;
  const u32 t = threadIdx.x, NT = blockDim.x;
  const u32 s0 = lstart[l], cnt = rga_lend_of<SRC>(lstart, l, nl, n) - s0;
  const u64* L = R + (u64)s0 * RGA_REC;
  u8* S = bst + s0;
  u32* G = gp + s0;
  auto gkey = [&](u32 x) { const u64 w = L[x * RGA_REC + RGA_WV]; return ((w >> 32) << 30) | (w & RGA_IDX_MASK); };
  for (u32 x = t; x < cnt; x += NT) {
    G[x] = x;
    S[x] = 0;
  }
  __syncthreads();
  block_sort_positions(G, cnt, [&](u32 a, u32 b) { return gkey(a) < gkey(b); });
  for (u32 j = t; j < cnt; j += NT) {
    const u64 v = gkey(G[j]) >> 30;
    if (j != 0 && (gkey(G[j - 1]) >> 30) == v) continue;
    u32 end = j + 1;
    while (end < cnt && (gkey(G[end]) >> 30) == v) ++end;
    for (u32 x = j; x < end; ++x) {
      const u32 op = (u32)(L[G[x] * RGA_REC + RGA_WV] >> 30) & 3u;
      if (op == 2) {
        for (u32 y = j; y < x; ++y)
          if (S[y] & 1) S[y] |= 2;
        continue;
      }
      if (op == 1) {
        int best = -1;
        for (u32 y = j; y < x; ++y)
          if (S[y] == 1 && (best < 0 || rec_lt(&L[G[y] * RGA_REC], &L[G[best] * RGA_REC], o))) best = (int)y;
        if (best >= 0) S[best] = 0;
      }
      S[x] = 1;
    }
  }
  __syncthreads();
  // survivors' positions to the front of G (their order is fixed by the sort below);
  // the tombstone flag rides in bit 31 (positions < 2^30)
  if (t == 0) {
    u32 w = 0;
    for (u32 j = 0; j < cnt; ++j)
      if (tomb ? (S[j] & 1) : S[j] == 1) G[w++] = G[j] | (S[j] & 2 ? RGA_TOMB_BIT : 0u);
    ns = w;
  }
  __syncthreads();
  const u32 m = ns;
  block_sort_positions(G, m, [&](u32 a, u32 b) {
    return rec_lt(&L[(a & ~RGA_TOMB_BIT) * RGA_REC], &L[(b & ~RGA_TOMB_BIT) * RGA_REC], o);
  });
  for (u32 j = t; j < m; j += NT) {
    const u64 w = L[(G[j] & ~RGA_TOMB_BIT) * RGA_REC + RGA_WV];
    tmp_v[s0 + j] = (u32)(w >> 32);
    tmp_s[s0 + j] = ((u32)w & RGA_IDX_MASK) | (G[j] & RGA_TOMB_BIT);
  }
  if (t == 0) rga_put_count(scnt, l, m);
}

#ifndef RGA_BIG_GRID
#define RGA_BIG_GRID 32  // workgroups of k_rga_big (lists of > 2 RW_CAP events, one per workgroup at a time;
                         // 256 cost ~5 us of launch on every call, most of which have none)
#endif
template <int SRC = RGA_SRC_LISTS>
__global__ void __launch_bounds__(1024) k_rga_big(smx_rga_ops o, const u64* __restrict__ R,
                                                  const u32* __restrict__ lstart, i64 n,
                                                  i64 nl, const u32* __restrict__ todo, const u32* __restrict__ ntodo,
                                                  u8* __restrict__ bst, u32* __restrict__ gp,
                                                  u32* __restrict__ tmp_v, u32* __restrict__ tmp_s,
                                                  u32* __restrict__ scnt, int tomb, const i32* __restrict__ gate) {
  if (*gate & RGA_E_UNGROUPED) return;
  for (u32 item = blockIdx.x; item < *ntodo; item += gridDim.x) {
    __syncthreads();
    rga_big_list<SRC>(o, R, todo[item], lstart, n, nl, bst, gp, tmp_v, tmp_s, scnt, tomb != 0);
  }
}
