// smx_rga_out.h -- output compaction: each list's survivors copied to their place in the
// output.  Part of the smx_rga.hip unit: included once, there.
#pragma once

#ifndef RGA_OUT_PRE
#define RGA_OUT_PRE 2
#endif
#ifndef RGA_OUT_LPW
#define RGA_OUT_LPW 1  // lists per wave in k_rga_out_fused (4: 28.8 us either way, round 4)
#endif

// One survivor to its place `at` in the output: its value, its source event (s: the tmp_s
// word, the tombstone bit stripped) and, in list mode, its tombstone flag.
__device__ __forceinline__ void rga_put_survivor(const smx_rga_out& out, u32 at, u32 v, u32 s) {
  out.out_value[at] = v;
  out.out_src[at] = (i32)(s & ~RGA_TOMB_BIT);
  if (out.out_tomb) out.out_tomb[at] = s & RGA_TOMB_BIT ? 1 : 0;
}

// Per list (one wave each): its output offset = the survivor sums of the earlier chunks
// + the counts of the chunk's earlier lists (one 16-byte read of each per lane, a wave
// sum), then its survivors, in list order, to their place in the output.  The last
// list's wave writes the total.  n_lists <= RGA_FUSED_MAX.
// RGA_OUT_LPW consecutive lists per wave (one 256-list chunk): one offset sum serves
// them all (the next list's offset is this one's plus its count), and all their first
// survivors are read before it is known.
__global__ void __launch_bounds__(BLOCK) k_rga_out_fused(const u32* __restrict__ tmp_v, const u32* __restrict__ tmp_s,
                                                        const u32* __restrict__ lstart, const u32* __restrict__ scnt,
                                                        i64 nl, smx_rga_out out, const i32* __restrict__ gate) {
  constexpr int LPW = RGA_OUT_LPW;
  if (*gate & RGA_E_UNGROUPED) return;
  static_assert(RGA_CS_LISTS % LPW == 0, "a wave's lists share a chunk");
  const u32 lane = threadIdx.x & (WAVE - 1);
  const i64 l0 = ((i64)blockIdx.x * (BLOCK / WAVE) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE))) * LPW;
  if (l0 >= nl) return;
  const u32 c = (u32)l0 / RGA_CS_LISTS, c0 = c * RGA_CS_LISTS;
  const uint4 cs = reinterpret_cast<const uint4*>(scnt - RGA_CS_MAX)[lane];
  const uint4 ls = reinterpret_cast<const uint4*>(scnt + c0)[lane];
  u32 s0[LPW], m[LPW];
#pragma unroll
  for (int j = 0; j < LPW; ++j) {
    const bool v = l0 + j < nl;
    s0[j] = v ? lstart[l0 + j] : 0u;
    m[j] = v ? scnt[l0 + j] : 0u;
  }
  u32 pv[LPW][RGA_OUT_PRE], ps[LPW][RGA_OUT_PRE];
#pragma unroll
  for (int j = 0; j < LPW; ++j)
#pragma unroll
    for (int i = 0; i < RGA_OUT_PRE; ++i) {
      const u32 x = lane + (u32)i * WAVE;
      pv[j][i] = x < m[j] ? __builtin_nontemporal_load(&tmp_v[s0[j] + x]) : 0u;
      ps[j][i] = x < m[j] ? __builtin_nontemporal_load(&tmp_s[s0[j] + x]) : 0u;
    }
  const u32 q = 4 * lane;
  u32 part = (q < c ? cs.x : 0u) + (q + 1 < c ? cs.y : 0u) + (q + 2 < c ? cs.z : 0u) + (q + 3 < c ? cs.w : 0u);
  const u32 r = (u32)l0 - c0;
  part += (q < r ? ls.x : 0u) + (q + 1 < r ? ls.y : 0u) + (q + 2 < r ? ls.z : 0u) + (q + 3 < r ? ls.w : 0u);
  u32 d = (u32)__builtin_amdgcn_readlane((int)wave_incl_sum_u32(part), WAVE - 1);
#pragma unroll
  for (int j = 0; j < LPW; ++j) {
    if (l0 + j >= nl) break;
#pragma unroll
    for (int i = 0; i < RGA_OUT_PRE; ++i) {
      const u32 x = lane + (u32)i * WAVE;
      if (x >= m[j]) break;
      rga_put_survivor(out, d + x, pv[j][i], ps[j][i]);
    }
    for (u32 x = lane + RGA_OUT_PRE * WAVE; x < m[j]; x += WAVE)
      rga_put_survivor(out, d + x, __builtin_nontemporal_load(&tmp_v[s0[j] + x]),
                       __builtin_nontemporal_load(&tmp_s[s0[j] + x]));
    if (lane == 0) {
      out.out_offsets[l0 + j] = d;
      if (l0 + j == nl - 1) {
        out.out_offsets[nl] = d + m[j];
        out.counts[0] = d + m[j];
      }
    }
    d += m[j];
  }
}

// Per list (one wave each): its survivors, in list order, to their place in the output.
// (k_rga_out_fused: RGA_OUT_PRE loads per lane issued with the offset's loads)
__global__ void __launch_bounds__(BLOCK) k_rga_out(const u32* __restrict__ tmp_v, const u32* __restrict__ tmp_s,
                                                  const u32* __restrict__ lstart, const u32* __restrict__ scnt,
                                                  const u32* __restrict__ soff, i64 nl, smx_rga_out out,
                                                  const i32* __restrict__ gate) {
  if (*gate & RGA_E_UNGROUPED) return;
  const u32 lane = threadIdx.x & (WAVE - 1);
  const i64 l = (i64)blockIdx.x * (BLOCK / WAVE) + threadIdx.x / WAVE;
  if (l >= nl) return;
  const u32 s0 = lstart[l], m = scnt[l], d = soff[l];
  for (u32 x = lane; x < m; x += WAVE)
    rga_put_survivor(out, d + x, __builtin_nontemporal_load(&tmp_v[s0 + x]),
                     __builtin_nontemporal_load(&tmp_s[s0 + x]));
  if (lane == 0) out.out_offsets[l] = d;
}

__global__ void k_rga_fin(const u32* __restrict__ soff_total, i64 n_lists, smx_rga_out out, const i32* __restrict__ gate) {
  if (*gate & RGA_E_UNGROUPED) return;
  out.out_offsets[n_lists] = *soff_total;
  out.counts[0] = *soff_total;
}
