// smx_rga_chain.h -- smx_rga_replay_chain's pre-pass: the input checks, the links' lengths,
// the jobs' slice starts and the per-event column map.  Part of the smx_rga.hip unit: included
// once, there.
//
// Job j replays the events of its segments job_seg[job_off[j] .. job_off[j + 1]), one segment
// after another; every segment stays where the caller put it in the columns, whatever the
// number of jobs that name it.  A link is one (job, segment) entry of job_seg.  The jobs'
// slices are laid out in job order, so one exclusive scan of the links' lengths gives every
// link's first slot (lpos), and job j's slice starts at lpos[job_off[j]].  The list kernels
// read a job through ChainSrc (smx_rga_list.h): event e of the job at slice start s0 is column
// cmap[s0 + e].
#pragma once

// The offsets and the link table of smx_rga_chain (the columns travel in an smx_rga_ops).
struct RgaChainJobs {
  i64 n_total, n_segs, n_jobs, n_links, n_out;
  const i64* seg_off;
  const i64* job_off;
  const i32* job_seg;
};

// Raises both error bits on a bad input: every list and output kernel, and k_rga_chain_map,
// leave at once, so no kernel reads a column, or writes a slice, through an unchecked offset.
//  * every entry of seg_off and job_off: negative, decreasing or past n_total / n_links;
//  * per job, a wave: each link's segment inside [0, n_segs), strictly above the link before
//    it in the job, and llen[k] = the segment's length (0 for a bad link);
//  * llen of the links outside every job, and llen[n_links], are 0, so that the exclusive
//    scan of llen also gives the end of the last slice;
//  * sum: the lengths' total in 64 bits (k_rga_onto_fit; a job's own length is below 2^30,
//    its segments being distinct ranges of the columns, but the jobs' sum is not).
// Also zeroes the survivor chunk sums (k_rga_bounds' duty).
__global__ void __launch_bounds__(BLOCK) k_rga_chain_check(RgaChainJobs q, u32* __restrict__ llen,
                                                           u32* __restrict__ csum,
                                                           unsigned long long* __restrict__ sum,
                                                           i32* __restrict__ err) {
  if (blockIdx.x == 0 && threadIdx.x < RGA_CS_MAX) csum[threadIdx.x] = 0u;
  bool bad = false;
  i64 top = q.n_segs > q.n_jobs ? q.n_segs : q.n_jobs;
  if (q.n_links > top) top = q.n_links;
  // the links that belong to a job: [jlo, jhi) when job_off is sound (else an error anyway)
  const i64 j0 = q.job_off[0], j1 = q.job_off[q.n_jobs];
  const i64 jlo = j0 < 0 ? 0 : j0 > q.n_links ? q.n_links : j0;
  const i64 jhi = j1 < jlo ? jlo : j1 > q.n_links ? q.n_links : j1;
  for (i64 i = (i64)blockIdx.x * BLOCK + threadIdx.x; i <= top; i += (i64)gridDim.x * BLOCK) {
    if (i <= q.n_segs) bad |= rga_onto_off_bad(q.seg_off, i, q.n_total);
    if (i <= q.n_jobs) bad |= rga_onto_off_bad(q.job_off, i, q.n_links);
    if (i <= q.n_links && (i < jlo || i >= jhi)) llen[i] = 0u;
  }
  const u32 lane = threadIdx.x & (WAVE - 1);
  const i64 nw = (i64)gridDim.x * (BLOCK / WAVE);
  unsigned long long acc = 0;
  for (i64 j = (i64)blockIdx.x * (BLOCK / WAVE) + threadIdx.x / WAVE; j < q.n_jobs; j += nw) {
    const i64 a = q.job_off[j], b = q.job_off[j + 1];
    if (a < 0 || b < a || b > q.n_links) continue;  // (raised by the loop above)
    for (i64 k = a + lane; k < b; k += WAVE) {
      const i64 s = q.job_seg[k];
      bool ok = s >= 0 && s < q.n_segs && (k == a || (i64)q.job_seg[k - 1] < s);
      i64 len = 0;
      if (ok) {
        const i64 c0 = q.seg_off[s], c1 = q.seg_off[s + 1];
        ok = c0 >= 0 && c1 >= c0 && c1 <= q.n_total;
        len = ok ? c1 - c0 : 0;
      }
      bad |= !ok;
      llen[k] = (u32)len;  // (at most n_total < 2^30)
      acc += (unsigned long long)len;
    }
  }
#pragma unroll
  for (int d = WAVE / 2; d > 0; d >>= 1) acc += __shfl_xor(acc, d, WAVE);
  if (lane == 0 && acc) atomicAdd(sum, acc);
  if (bad) atomicOr(err, (i32)(RGA_E_INPUT | RGA_E_UNGROUPED));
}

// After the scan (lpos) and the fit check: lstart[j] = lpos[job_off[j]], n_jobs + 1 of them, and
// the column map, a wave per link: cmap[lpos[k] + i] = seg_off[job_seg[k]] + i.  Leaves at once
// on an error: past the checks every link lies in [0, n_total) and every slot in [0, n_out).
__global__ void __launch_bounds__(BLOCK) k_rga_chain_map(RgaChainJobs q, const u32* __restrict__ lpos,
                                                         u32* __restrict__ lstart, u32* __restrict__ cmap,
                                                         const i32* __restrict__ gate) {
  if (*gate & RGA_E_UNGROUPED) return;
  for (i64 j = (i64)blockIdx.x * BLOCK + threadIdx.x; j <= q.n_jobs; j += (i64)gridDim.x * BLOCK)
    lstart[j] = lpos[q.job_off[j]];
  const u32 lane = threadIdx.x & (WAVE - 1);
  const i64 nw = (i64)gridDim.x * (BLOCK / WAVE);
  for (i64 k = (i64)blockIdx.x * (BLOCK / WAVE) + threadIdx.x / WAVE; k < q.n_links; k += nw) {
    const u32 p0 = lpos[k], len = lpos[k + 1] - p0;
    if (len == 0) continue;
    const u32 c0 = (u32)q.seg_off[q.job_seg[k]];
    for (u32 i = lane; i < len; i += WAVE) cmap[p0 + i] = c0 + i;
  }
}
