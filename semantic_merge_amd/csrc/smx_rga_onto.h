// smx_rga_onto.h -- smx_rga_replay_onto's pre-pass: the jobs' lengths, slice starts and
// source descriptors, and the input checks.  Part of the smx_rga.hip unit: included once, there.
//
// Job j replays its base's events followed by its own; both stay where the caller put them
// in the columns (a base once, whatever the number of jobs that name it), and the list
// kernels read them through OntoSrc (smx_rga_list.h).  What a list is to smx_rga_replay a
// job is here: its slice of tmp_v / tmp_s / the long jobs' records starts at
// r(j) = the lengths of the jobs before it, so those arrays are sized by n_out.
#pragma once

// The offsets and job_base of smx_rga_onto (the columns travel in an smx_rga_ops).
struct RgaOntoJobs {
  i64 n_total, n_bases, n_jobs, n_out;
  const i64* base_off;
  const i64* own_off;
  const i32* job_base;
};

// offsets[i] of an array that must not decrease inside [0, n_total]
__device__ __forceinline__ bool rga_onto_off_bad(const i64* off, i64 i, i64 n_total) {
  const i64 a = off[i];
  return a < 0 || a > n_total || (i > 0 && off[i - 1] > a);
}

// Per job: len[j] = its base's events + its own, its descriptor (b0, lb, o0 - lb: OntoSrc);
// len[n_jobs] = 0, so that the exclusive scan of len also gives the end of the last slice.
// Checks every offset and every job_base: a bad one raises both error bits, at which
// every list and output kernel leaves before it reads a column.  sum: the lengths' total
// in 64 bits (k_rga_onto_fit).  Also zeroes the survivor chunk sums (k_rga_bounds' duty).
__global__ void __launch_bounds__(BLOCK) k_rga_onto_jobs(RgaOntoJobs q, u32* __restrict__ len,
                                                         uint4* __restrict__ jobs, u32* __restrict__ csum,
                                                         unsigned long long* __restrict__ sum, i32* __restrict__ err) {
  if (blockIdx.x == 0 && threadIdx.x < RGA_CS_MAX) csum[threadIdx.x] = 0u;
  const i64 top = q.n_bases > q.n_jobs ? q.n_bases : q.n_jobs;
  bool bad = false;
  unsigned long long acc = 0;
  for (i64 i = (i64)blockIdx.x * BLOCK + threadIdx.x; i <= top; i += (i64)gridDim.x * BLOCK) {
    if (i <= q.n_bases) bad |= rga_onto_off_bad(q.base_off, i, q.n_total);
    if (i <= q.n_jobs) bad |= rga_onto_off_bad(q.own_off, i, q.n_total);
    if (i == 0) bad |= q.base_off[q.n_bases] > q.own_off[0];  // the bases lie before the own events
    if (i == q.n_jobs) len[i] = 0u;
    if (i >= q.n_jobs) continue;
    const i64 b = q.job_base[i], o0 = q.own_off[i], o1 = q.own_off[i + 1];
    bool ok = o0 >= 0 && o1 >= o0 && o1 <= q.n_total && b >= (i64)SMX_NONE && b < q.n_bases;
    i64 b0 = 0, lb = 0;
    if (ok && b >= 0) {
      b0 = q.base_off[b];
      lb = q.base_off[b + 1] - b0;
      ok = b0 >= 0 && lb >= 0 && b0 + lb <= q.n_total;
    }
    bad |= !ok;
    const u32 l = ok ? (u32)(lb + o1 - o0) : 0u;  // (at most 2 n_total < 2^32)
    len[i] = l;
    jobs[i] = make_uint4((u32)b0, ok ? (u32)lb : 0u, (u32)(o0 - lb), 0u);
    acc += l;
  }
#pragma unroll
  for (int d = WAVE / 2; d > 0; d >>= 1) acc += __shfl_xor(acc, d, WAVE);
  if ((threadIdx.x & (WAVE - 1)) == 0 && acc) atomicAdd(sum, acc);
  if (bad) atomicOr(err, (i32)(RGA_E_INPUT | RGA_E_UNGROUPED));
}

// The jobs' events must fit the slices and the output (n_out): else both error bits.
__global__ void k_rga_onto_fit(const unsigned long long* __restrict__ sum, i64 n_out, i32* __restrict__ err) {
  if (*sum > (unsigned long long)n_out) atomicOr(err, (i32)(RGA_E_INPUT | RGA_E_UNGROUPED));
}
