// smx_shard.h -- the sharded merge (include/smx.h smx_shard_step, smx_shard_range_info): its
// summary, table and halo kernels and shard_impl, over the launchers and plans of
// smx_compose.hip.  Part of that unit: included once, there, after the orchestration.
#pragma once

// summary[0..21]
__global__ void k_shard_summary(const ComposeMeta* meta, i64* summary) {
  for (int k = 0; k < SMX_N_KINDS; ++k) summary[k] = (i64)meta->kcnt[k];
  summary[18] = (i64)meta->n_ren_side[0];
  summary[19] = (i64)meta->n_ren_side[1];
  summary[20] = (i64)meta->n_move_none;
  summary[21] = (i64)((meta->f_fail & 1 ? 1 : 0) | (meta->bad_sym ? 2 : 0) | (meta->f_fail & 2 ? 4 : 0));
}

// An empty shard hands the incoming open region (device- or host-held) straight on.
__global__ void k_pass_region(const i64* in_dev, i64 in_ahead, i64 in_d, i64* summary) {
  if (in_dev) {
    in_ahead = in_dev[0];
    in_d = in_dev[1];
  }
  summary[22] = in_d > 0 ? 1 : 0;
  summary[23] = in_d > 0 ? in_ahead : 0;
  summary[24] = in_d > 0 ? in_d : 0;
  summary[25] = summary[26] = summary[27] = 0;
}

__global__ void k_shard_walk_sum(const ComposeMeta* meta, i64* summary) {
  summary[22] = (i64)meta->out_open;
  summary[23] = (i64)meta->out_ahead;
  summary[24] = (i64)meta->out_d;
  summary[25] = (i64)meta->n_conf;
  summary[26] = (i64)meta->n_skip;
  summary[27] = (i64)meta->halo_overflow;
}

__global__ void k_shard_tab_sum(const ComposeMeta* meta, i64* summary, int bucketed) {
  for (int i = 0; i < 3; ++i) summary[28 + i] = bucketed ? (i64)bit_width32(meta->vbits[i]) : 32;
  summary[31] = (i64)meta->tab_over;
}
__global__ void k_tab_over_reset(ComposeMeta* meta) { meta->tab_over = 0; }

// fin from the reduced partial tables: packed with the global widths when they
// fit in 64 bits (meta->vbits takes the global widths, for k_emit).
__global__ void k_fin_from_tab(const void* __restrict__ tabv, const i64* __restrict__ glob, i64 n_sym,
                               int tagbits, ComposeMeta* meta, int4* __restrict__ fin) {
  u32 w[3];
  const u64* tab = (const u64*)tabv;
  const u32* tab32 = (const u32*)tabv;
  for (int i = 0; i < 3; ++i)
    w[i] = (u32)min(max(tagbits ? (i64)(i32)tab32[3 * n_sym + i] : glob[i], (i64)0), (i64)32);
  const FinPack FP = fin_pack_make(w[0], w[1], w[2], true);
  if (blockIdx.x == 0 && threadIdx.x < 3)
    meta->vbits[threadIdx.x] = w[threadIdx.x] >= 32 ? ~0u : ((1u << w[threadIdx.x]) - 1u);
  for (i64 s = (i64)blockIdx.x * BLOCK + threadIdx.x; s < n_sym; s += (i64)gridDim.x * BLOCK) {
    int va, vf, vc;
    if (tagbits) {
      const u32 m = (1u << (31 - tagbits)) - 1u;
      const u32 a = tab32[s], f = tab32[n_sym + s], c = tab32[2 * n_sym + s];
      va = a ? (int)(a & m) - 1 : -1, vf = f ? (int)(f & m) - 1 : -1, vc = c ? (int)(c & m) - 1 : -1;
    } else {
      const u64 a = tab[s], f = tab[n_sym + s], c = tab[2 * n_sym + s];
      va = a ? (int)(u32)a - 1 : -1, vf = f ? (int)(u32)f - 1 : -1, vc = c ? (int)(u32)c - 1 : -1;
    }
    fin_put(FP, fin, (u32)s, va, vf, vc);
  }
}

// This shard's halo from the all-gather of every shard's ORDER outputs (smx_shard
// .order_gather): for each branch b, the first H renames of b on the following shards
// in shard order -- entry i is taken from the shard q whose cumulative count first
// exceeds i -- and halo_dev = (count, count, more, more).
__global__ void k_halo_gather(const i64* __restrict__ g, int W, int r, i64 H, u32* hs0, u32* hs1, i32* hc0, i32* hc1,
                              i32* hr0, i32* hr1, i64* halo_dev) {
  const i64 row = SMX_SHARD_SUMMARY + 3 * H;  // int64 words per shard
  for (int b = 0; b < 2; ++b) {
    u32* hs = b ? hs1 : hs0;
    i32* hc = b ? hc1 : hc0;
    i32* hr = b ? hr1 : hr0;
    i64 total = 0;
    for (int q = r + 1; q < W; ++q) total += max(g[q * row + 18 + b], (i64)0);
    const i64 got = min(total, H);
    for (i64 i = (i64)blockIdx.x * BLOCK + threadIdx.x; i < got; i += (i64)gridDim.x * BLOCK) {
      i64 cum = 0;
      int q = r + 1;
      for (; q < W; ++q) {
        const i64 c = min(max(g[q * row + 18 + b], (i64)0), H);
        if (i < cum + c) break;
        cum += c;
      }
      const i64 off = i - cum;
      const i32* X = reinterpret_cast<const i32*>(g + q * row + SMX_SHARD_SUMMARY);  // [3][2H] int32
      hs[i] = (u32)X[b * H + off];
      hc[i] = X[2 * H + b * H + off];
      hr[i] = X[4 * H + b * H + off];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      halo_dev[b] = got;
      halo_dev[2 + b] = total > got ? 1 : 0;
    }
  }
}

static int shard_impl(const smx_ops* ops, const smx_shard* sh, const smx_compose_out* out, void* ws,
                      size_t ws_bytes, hipStream_t st, int step) {
  if (!sh || !sh->summary) return set_err(SMX_E_ARG, "null shard / summary");
  Layout L{};
  int rc = check_args(ops, out, ws, ws_bytes, &L);
  if (rc) return rc;
  const i64 na = ops->n_a, nb = ops->n_b, n = na + nb, n_sym = ops->n_sym;
  StageTimer tm(st, profiling_on() != 0);
  Ctx C = make_ctx(ops, out, ws, L, st, &tm, sh->src_a, sh->src_b);
  C.src_map = sh->src_map;
  if (sh->src_map && ops->b_gap != 0) return set_err(SMX_E_ARG, "src_map needs b_gap = 0");
  if (n == 0) {  // an empty shard: neutral summaries and outputs
    if (step == SMX_SHARD_ORDER) HIP_TRY(hipMemsetAsync(sh->summary, 0, SMX_SHARD_SUMMARY * 8, st));
    if (step == SMX_SHARD_WALK) {
      // the open region passes through unchanged (or none comes in): always rewrite
      // the outgoing state, a previous round may have left another one
      hipLaunchKernelGGL(k_pass_region, dim3(1), dim3(1), 0, st, (const i64*)sh->in_state_dev,
                         (i64)sh->in_ahead, (i64)sh->in_d, sh->summary);
      HIP_TRY(hipGetLastError());
    }
    if (step == SMX_SHARD_TABLES && sh->part_tab)
      HIP_TRY(hipMemsetAsync(sh->part_tab, 0, (size_t)3 * n_sym * (sh->tab32 > 0 ? 4 : 8), st));
    if (step == SMX_SHARD_EMIT) HIP_TRY(hipMemsetAsync(out->counts, 0, 2 * sizeof(int64_t), st));
    return SMX_OK;
  }
  // The bucketed table records are consumed by SMX_SHARD_TABLES (k_tb_unskip kills the
  // walk's skipped renames in place): a second TABLES needs a SCATTER (or ORDER) first.
  // Tracked per workspace on the host, where the steps are issued in stream order.
  auto records_state = [&](int set) -> int {  // set: 1 scattered, 2 consumed; -1 query
    static std::mutex mu;
    static std::vector<std::pair<void*, int>> st_of;
    std::lock_guard<std::mutex> g(mu);
    for (auto& e : st_of)
      if (e.first == ws) {
        if (set >= 0) e.second = set;
        return e.second;
      }
    if (set >= 0) {
      if (st_of.size() >= 64) st_of.erase(st_of.begin());
      st_of.push_back({ws, set});
    }
    return set >= 0 ? set : 0;
  };
  auto order_outputs = [&]() -> int {
    hipLaunchKernelGGL(k_shard_summary, dim3(1), dim3(1), 0, st, C.ws<ComposeMeta>(B_META), sh->summary);
    if (sh->halo_cap > 0)
      hipLaunchKernelGGL(k_halo_export, dim3(1), dim3(EX_NT), 0, st, walk_args(C, nullptr), sh->export_sym,
                         sh->export_cls, sh->export_src, (u64)sh->halo_cap);
    HIP_TRY(hipGetLastError());
    // the table records, bucketed while the host exchanges the summaries and walks
    records_state(1);
    return launch_tb_prescatter(C);
  };
  switch (step) {
    case SMX_SHARD_ORDER:
    case SMX_SHARD_ORDER_FIX: {
      if (sh->halo_cap < 0 || (sh->halo_cap > 0 && (!sh->export_sym || !sh->export_cls || !sh->export_src)))
        return set_err(SMX_E_ARG, "bad export buffers");
      const i64 tgt = knob("SMX_WIN_TGT", WIN_TGT);
      if (step == SMX_SHARD_ORDER && !sh->src_map) {  // asynchronous: failures show in summary[21]
        g_plan = SMX_PLAN_PRESORTED;
        if ((rc = run_presorted(C, tgt))) return rc;
        return order_outputs();
      }
      ComposeMeta hm;
      if (step == SMX_SHARD_ORDER) {
        // a sample-sorted shard's branch logs are in any order: the generic plan
        if ((rc = run_order(C, true, false, &hm))) return rc;  // times its own stages
      } else {
        if ((rc = read_meta(C, &hm))) return rc;
        // a compacted shard (b_gap = 0) may take the generic plan
        if (hm.f_fail && (rc = order_fallbacks(C, ops->b_gap == 0, false, &hm, tgt, true))) return rc;
      }
      if ((rc = order_outputs())) return rc;
      if (hm.bad_sym) return set_err(SMX_E_ARG, "invalid input: sym[i] >= n_sym or kind[i] >= 18");
      if (hm.f_fail)
        return set_err(SMX_E_ARG, "sharded merge needs timestamp-ordered branch logs in every shard");
      break;
    }
    case SMX_SHARD_WALK: {
      tm.begin(ST_WALK);
      if (sh->order_gather && sh->halo_cap > 0) {
        if (!sh->halo_dev || !sh->halo_sym[0] || !sh->halo_sym[1] || !sh->halo_cls[0] || !sh->halo_cls[1] ||
            !sh->halo_src[0] || !sh->halo_src[1] || sh->world < 1 || sh->rank < 0 || sh->rank >= sh->world)
          return set_err(SMX_E_ARG, "order_gather needs writable halo buffers and halo_dev");
        hipLaunchKernelGGL(k_halo_gather, dim3(SMX_CEIL_DIV(sh->halo_cap, (i64)BLOCK)), dim3(BLOCK), 0, st,
                           sh->order_gather, (int)sh->world, (int)sh->rank, (i64)sh->halo_cap,
                           (u32*)sh->halo_sym[0], (u32*)sh->halo_sym[1], (i32*)sh->halo_cls[0],
                           (i32*)sh->halo_cls[1], (i32*)sh->halo_src[0], (i32*)sh->halo_src[1],
                           (i64*)sh->halo_dev);
        HIP_TRY(hipGetLastError());
      }
      if ((rc = launch_walk(C, sh))) return rc;
      hipLaunchKernelGGL(k_shard_walk_sum, dim3(1), dim3(1), 0, st, C.ws<ComposeMeta>(B_META), sh->summary);
      HIP_TRY(hipGetLastError());
      tm.end(ST_WALK);
      break;
    }
    case SMX_SHARD_TABLES: {
      if (!sh->part_tab) return set_err(SMX_E_ARG, "null part_tab");
      if (records_state(-1) != 1)
        return set_err(SMX_E_ARG, "SMX_SHARD_TABLES needs the records bucketed by SMX_SHARD_ORDER / "
                                  "ORDER_FIX / SCATTER since the last TABLES");
      records_state(2);
      tm.begin(ST_TABLES);
      bool bucketed = false;
      // (ORDER / ORDER_FIX / SCATTER bucketed the records)
      if (sh->tab32 < 0 || sh->tab32 > 8 || (sh->tab32 > 0 && ((u64)sh->rank + 1u) >> sh->tab32))
        return set_err(SMX_E_ARG, "tab32: the tag (rank + 1) must fit tab32 <= 8 bits");
      hipLaunchKernelGGL(k_tab_over_reset, dim3(1), dim3(1), 0, st, C.ws<ComposeMeta>(B_META));
      if ((rc = launch_tables(C, sh->part_tab, (u32)sh->rank + 1u, sh->tab32, &bucketed, true))) return rc;
      hipLaunchKernelGGL(k_shard_tab_sum, dim3(1), dim3(1), 0, st, C.ws<ComposeMeta>(B_META), sh->summary,
                         bucketed ? 1 : 0);
      HIP_TRY(hipGetLastError());
      tm.end(ST_TABLES);
      break;
    }
    case SMX_SHARD_SCATTER: {
      records_state(1);
      if ((rc = launch_tb_prescatter(C))) return rc;
      break;
    }
    case SMX_SHARD_EMIT: {
      if (!sh->fin_tab || (!sh->glob && sh->tab32 == 0)) return set_err(SMX_E_ARG, "null fin_tab / glob");
      if (sh->tab32 < 0 || sh->tab32 > 8) return set_err(SMX_E_ARG, "tab32 must be 0..8");
      tm.begin(ST_EMIT);
      hipLaunchKernelGGL(k_fin_from_tab, dim3(grid_for(n_sym)), dim3(BLOCK), 0, st, (const void*)sh->fin_tab,
                         sh->glob, n_sym, (int)sh->tab32, C.ws<ComposeMeta>(B_META), C.ws<int4>(B_FIN));
      if ((rc = launch_emit(C, true, sh))) return rc;
      tm.end(ST_EMIT);
      ComposeMeta hm;
      if (sh->summary_host) {  // what the move prefix needs, as the host gathered it
        hm.kcnt[KMOVE] = (u64)sh->summary_host[KMOVE];
        hm.n_move_none = (u64)sh->summary_host[20];
      } else if ((rc = read_meta(C, &hm))) {
        return rc;
      }
      tm.begin(ST_MVPREFIX);
      if ((rc = run_mvprefix(C, hm, sh->mv_prefix))) return rc;
      tm.end(ST_MVPREFIX);
      break;
    }
    default:
      return set_err(SMX_E_ARG, "unknown shard step");
  }
  tm.flush();
  return SMX_OK;
}

// smx_shard_range_info (include/smx.h): one block for the keys, then a grid over both
// slices for the order check (a violation stores 0; every writer stores the same).
__device__ __forceinline__ i64 rinfo_key(u64 v) { return (i64)(v ^ 0x8000000000000000ull); }
__global__ void k_range_info(const u64* __restrict__ ts, i64 off_a, i64 n_a, i64 off_b, i64 n_b, int rh,
                             int sa, int sb, i64* __restrict__ out) {
  const int t = threadIdx.x;
  if (t == 0) {
    out[0] = n_a;
    out[1] = n_b;
    out[2] = n_a ? rinfo_key(ts[off_a]) : 0;
    out[3] = n_a ? rinfo_key(ts[off_a + n_a - 1]) : 0;
    out[4] = n_b ? rinfo_key(ts[off_b]) : 0;
    out[5] = n_b ? rinfo_key(ts[off_b + n_b - 1]) : 0;
    out[6] = 1;
    out[7] = sa;
    out[8] = sb;
  }
  for (int i = t; i < 4 * rh; i += blockDim.x) {
    const int br = i / (2 * rh), j = i % (2 * rh);
    const i64 o = br ? off_b : off_a, n = br ? n_b : n_a;
    const i64 h = n < rh ? n : rh;
    i64 pos;
    if (n == 0) pos = -1;
    else if (j < rh) pos = j < h ? o + j : o;                         // head, padded
    else pos = j - rh < rh - h ? o : o + n - h + (j - rh - (rh - h));  // tail, right-aligned
    out[9 + i] = pos < 0 ? 0 : rinfo_key(ts[pos]);
  }
}
__global__ void k_range_order(const u64* __restrict__ ts, i64 off_a, i64 n_a, i64 off_b, i64 n_b,
                              i64* __restrict__ out) {
  bool bad = false;
  for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < n_a + n_b; i += (i64)gridDim.x * blockDim.x) {
    const bool b = i >= n_a;
    const i64 k = b ? i - n_a : i;
    if (k == 0) continue;
    const i64 o = b ? off_b : off_a;
    bad |= ts[o + k] < ts[o + k - 1];
  }
  if (__syncthreads_or(bad) && threadIdx.x == 0) out[6] = 0;
}
extern "C" int smx_shard_range_info(const uint64_t* ts, int64_t off_a, int64_t n_a, int64_t off_b, int64_t n_b,
                                    int32_t rh, int32_t check_order, int32_t signed_a, int32_t signed_b, int64_t* out,
                                    void* stream) {
  if (!ts || !out || n_a < 0 || n_b < 0 || rh < 1 || off_a < 0 || off_b < 0)
    return set_err(SMX_E_ARG, "smx_shard_range_info: bad argument");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_range_info, dim3(1), dim3(BLOCK), 0, st, (const u64*)ts, off_a, n_a, off_b, n_b, rh,
                     signed_a, signed_b, (i64*)out);
  if (check_order && n_a + n_b > 1)
    hipLaunchKernelGGL(k_range_order, dim3(grid_for(n_a + n_b, BLOCK * 16)), dim3(BLOCK), 0, st, (const u64*)ts,
                       off_a, n_a, off_b, n_b, (i64*)out);
  HIP_TRY(hipGetLastError());
  return SMX_OK;
}

extern "C" int smx_shard_step(const smx_ops* ops, const smx_shard* shard, const smx_compose_out* out,
                              void* workspace, size_t workspace_bytes, void* stream, int step) {
  return entry(ops, [&] { return shard_impl(ops, shard, out, workspace, workspace_bytes, (hipStream_t)stream, step); });
}
