// smx_wave_sort.h -- sorting inside one wave: lane exchanges by a constant xor mask and the
// in-register bitonic networks on them.  Part of the smx_rga.hip unit: included once, there.
#pragma once

// v from lane ^ lm (lm a constant after unrolling): DPP for 1, 2, 3, 7, 15, a swizzle
// within 32 lanes for 4, 8, 16, 31, a permute otherwise.
__device__ __forceinline__ u32 xshfl(u32 v, u32 lm) {
  switch (lm) {
    case 1: return (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false);
    case 2: return (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, false);
    case 3: return (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x1B, 0xF, 0xF, false);
    case 7: return (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, false);
    case 15: return (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xF, 0xF, false);
    case 4: return (u32)__builtin_amdgcn_ds_swizzle((int)v, (4 << 10) | 0x1f);
    case 8: return (u32)__builtin_amdgcn_ds_swizzle((int)v, (8 << 10) | 0x1f);
    case 16: return (u32)__builtin_amdgcn_ds_swizzle((int)v, (16 << 10) | 0x1f);
    case 31: return (u32)__builtin_amdgcn_ds_swizzle((int)v, (31 << 10) | 0x1f);
    default: return (u32)__shfl_xor((int)v, (int)lm);
  }
}

// Ascending bitonic network (all-ascending form: the first step of each merge compares
// e with its mirror e ^ (kk - 1)) over 64 * K (key, payload) pairs, e = k * 64 + lane;
// the partner of (lane, k) under mask m is (lane ^ (m & 63), k ^ (m >> 6)).  Steps are
// template-expanded so every exchange pattern is a constant.
template <int K, u32 KK, u32 J>
__device__ __forceinline__ void wave_bitonic_step(u64 (&key)[8], u32 (&pay)[8], u32 lane) {
  constexpr u32 mask = J == (KK >> 1) ? KK - 1 : J;
  constexpr u32 lm = mask & 63u, sm = mask >> 6;
  u64 nk[K];
  u32 np[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int src = k ^ (int)sm;
    u64 ok = key[src];
    u32 op = pay[src];
    if (lm) {
      ok = ((u64)xshfl((u32)(ok >> 32), lm) << 32) | xshfl((u32)ok, lm);
      op = xshfl(op, lm);
    }
    const bool lower = (((u32)k * 64u + lane) & J) == 0;
    const bool take = lower ? ok < key[k] : key[k] < ok;
    nk[k] = take ? ok : key[k];
    np[k] = take ? op : pay[k];
  }
#pragma unroll
  for (int k = 0; k < K; ++k) {
    key[k] = nk[k];
    pay[k] = np[k];
  }
  if constexpr (J > 1) wave_bitonic_step<K, KK, (J >> 1)>(key, pay, lane);
}

template <int K, u32 KK = 2>
__device__ __forceinline__ void wave_bitonic(u64 (&key)[8], u32 (&pay)[8], u32 lane) {
  wave_bitonic_step<K, KK, (KK >> 1)>(key, pay, lane);
  if constexpr (KK < 64u * K) wave_bitonic<K, KK * 2>(key, pay, lane);
}

// The same network over 64 * K packed 32-bit keys (rank fields above the event bits).
template <int K, u32 KK, u32 J>
__device__ __forceinline__ void wave_bitonic32_step(u32 (&key)[8], u32 lane) {
  constexpr u32 mask = J == (KK >> 1) ? KK - 1 : J;
  constexpr u32 lm = mask & 63u, sm = mask >> 6;
  u32 nk[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    u32 ok = key[k ^ (int)sm];
    if (lm) ok = xshfl(ok, lm);
    const bool lower = (((u32)k * 64u + lane) & J) == 0;
    nk[k] = lower ? min(ok, key[k]) : max(ok, key[k]);
  }
#pragma unroll
  for (int k = 0; k < K; ++k) key[k] = nk[k];
  if constexpr (J > 1) wave_bitonic32_step<K, KK, (J >> 1)>(key, lane);
}

template <int K, u32 KK = 2>
__device__ __forceinline__ void wave_bitonic32(u32 (&key)[8], u32 lane) {
  wave_bitonic32_step<K, KK, (KK >> 1)>(key, lane);
  if constexpr (KK < 64u * K) wave_bitonic32<K, KK * 2>(key, lane);
}
