// groupby.hip — tsdbhip_groupby_plan and tsdbhip_desc_gather: the host side
// of k_groupby.hip. Included by api.hip (unity build).
//
// tsdbhip_groupby_plan, all on the slot's stream:
//   k_gb_keys                       checks, group keys, drop flags, AND / OR   [sync 1]
//   per live digit, least significant first, the drop flag last:
//     k_gb_count, scan, k_gb_scatter
//   k_gb_heads, scan, k_gb_emit     group boundaries and keys
//   k_gb_first, k_gb_masks, k_gb_finalize   tags                               [sync 2]
//   copies of the outputs                                                     [sync 3]
// Sync 1 tells the host the first offending span (nothing is written after an
// error), how many spans were dropped and which digit positions are live: a
// position whose AND equals its OR over the grouped spans has a single live
// bucket and its pass is not launched at all.
#include "groupby_host.h"

static int groupby_plan(Slot* ctx, const tsdbhip_keys_desc* d, tsdbhip_groups_out* out) {
  out->n_groups = out->n_grouped = out->n_dropped = 0;
  ctx->timing = tsdbhip_timing();
  ctx->h2d_bytes = 0;
  ctx->reuse_inputs = false;
  if (const char* why = gb_check_desc(d)) {
    set_error(ctx, "tsdbhip_groupby_plan: %s", why);
    return TSDBHIP_E_INVALID_ARG;
  }
  const uint32_t n = d->n_spans;
  const uint32_t klen = (uint32_t)d->n_group_bys * d->value_width;
  const uint32_t tag_stride = TSDBHIP_MAX_TAGS * ((uint32_t)d->name_width + d->value_width);
  if (!out->group_span_start || (n && (!out->order || !out->group_ntags || !out->group_tags || !out->group_common ||
                                       (klen && !out->group_key)))) {
    set_error(ctx, "tsdbhip_groupby_plan: null output array");
    return TSDBHIP_E_INVALID_ARG;
  }
  if (n == 0) {
    out->group_span_start[0] = 0;
    return TSDBHIP_OK;
  }
  const bool dev = (d->flags & TSDBHIP_DESC_DEVICE) != 0;
  if (!dev) {
    const int64_t bad = gb_check_key_off(d->key_off, n, d->key_nbytes);
    if (bad >= 0) {
      set_error(ctx, "tsdbhip_groupby_plan: key_off out of range at span %lld", (long long)bad);
      return TSDBHIP_E_INVALID_ARG;
    }
  }
  hipStream_t st = ctx->stream;
  const bool timed = ctx->opt.events != 2;

  GbKeysArgs k = {};
  k.n = n;
  k.mw = d->metric_width;
  k.nw = d->name_width;
  k.vw = d->value_width;
  k.ngb = d->n_group_bys;
  k.klen = klen;
  k.key_off = stage(ctx, "gb_koff", d->key_off, (size_t)n + 1, dev);
  k.key = stage(ctx, "gb_key", d->key_bytes, d->key_nbytes, dev, 16);
  k.key_nbytes = d->key_nbytes;
  const uint8_t* kept = d->span_kept ? stage(ctx, "gb_kept", d->span_kept, n, dev) : nullptr;
  std::memcpy(k.gb, d->group_bys ? d->group_bys : (const uint8_t*)"", (size_t)d->n_group_bys * d->name_width);
  k.gkey = scratch<uint8_t>(ctx, "gb_gkey", (size_t)n * klen);
  k.drop = scratch<uint8_t>(ctx, "gb_drop", n);
  k.ntags = scratch<uint8_t>(ctx, "gb_ntags", n);
  uint32_t* idx_a = scratch<uint32_t>(ctx, "gb_idx_a", n);
  uint32_t* idx_b = scratch<uint32_t>(ctx, "gb_idx_b", n);
  k.idx0 = idx_a;
  // the call's small state: [0,1] error word, [2] dropped spans, [4,20) AND
  // words, [20,36) OR words, [36,37] the number of groups
  constexpr size_t SM_WORDS = 40;
  uint32_t* sm = scratch<uint32_t>(ctx, "gb_small", SM_WORDS);
  {
    uint32_t* h = (uint32_t*)ctx->host_small;
    std::memset(h, 0, SM_WORDS * 4);
    h[0] = h[1] = ~0u;
    for (int w = 0; w < (int)GB_KEY_WORDS; w++) h[4 + w] = ~0u;
    HIPCHK(hipMemcpyAsync(sm, h, SM_WORDS * 4, hipMemcpyHostToDevice, st));
  }
  k.err = (unsigned long long*)sm;
  k.n_dropped = sm + 2;
  k.andw = sm + 4;
  k.orw = sm + 20;
  uint64_t* d_ngroups = (uint64_t*)(sm + 36);
  if (timed) HIPCHK(hipEventRecord(ctx->ev[0], st));
  LAUNCH(k_gb_keys, dim3(grid_for(n, 256)), dim3(256), 0, st, k);
  HIPCHK(hipGetLastError());
  uint32_t smh[SM_WORDS];
  readback(ctx, smh, sm, sizeof smh);  // [sync 1]
  unsigned long long err;
  std::memcpy(&err, smh, 8);
  if (err != ~0ull) {
    const unsigned long long span = err >> 8;
    const uint32_t cls = (uint32_t)(err & 0xFF);
    if (cls == GB_E_UNSORTED) {
      set_error(ctx, "tsdbhip_groupby_plan: span %llu is not after span %llu under SpanCmp", span, span - 1);
      return TSDBHIP_E_UNSORTED;
    }
    if (cls == GB_E_SHAPE) set_error(ctx, "tsdbhip_groupby_plan: bad row key length at span %llu", span);
    else set_error(ctx, "tsdbhip_groupby_plan: key_off out of range at span %llu", span);
    return TSDBHIP_E_INVALID_ARG;
  }
  const uint32_t n_dropped = smh[2], ng = n - n_dropped;
  out->n_dropped = n_dropped;
  out->n_grouped = ng;
  tsdbhip_timing tm = {};
  tm.hot_kernel = TSDBHIP_HOT_GROUPBY;
  tm.alg_bytes = d->key_nbytes + 8ull * ((uint64_t)n + 1) + (kept ? n : 0);
  if (ng == 0) {  // every span dropped: no group
    out->group_span_start[0] = 0;
    tm.h2d_bytes = ctx->h2d_bytes;
    ctx->timing = tm;
    return TSDBHIP_OK;
  }

  // ---- the sort: live digits from the least significant, dropped spans last ----
  struct Pass { const uint8_t* dig; uint32_t stride, off; };
  std::vector<Pass> passes;
  for (uint32_t p = klen; p-- > 0;) {
    const uint32_t x = (smh[4 + p / 4] ^ smh[20 + p / 4]) >> (8 * (p % 4));
    if (x & 0xFFu) passes.push_back(Pass{k.gkey, klen, p});
  }
  if (n_dropped) passes.push_back(Pass{k.drop, 1, 0});
  const uint32_t nbt = (n + GB_TILE - 1) / GB_TILE;
  const uint32_t* ord = idx_a;
  if (!passes.empty()) {
    uint64_t* counts = scratch<uint64_t>(ctx, "gb_counts", 256ull * nbt);
    uint64_t* offs = scratch<uint64_t>(ctx, "gb_offs", 256ull * nbt);
    uint64_t* tot = scratch<uint64_t>(ctx, "gb_tot", 1);
    uint32_t *src = idx_a, *dst = idx_b;
    if (timed) HIPCHK(hipEventRecord(ctx->ev[8], st));
    for (const Pass& p : passes) {
      GbSortArgs s = {};
      s.n = n;
      s.nb = nbt;
      s.src = src;
      s.dst = dst;
      s.dig = p.dig;
      s.stride = p.stride;
      s.off = p.off;
      s.counts = counts;
      s.offs = offs;
      LAUNCH(k_gb_count, dim3(nbt), dim3(GB_THREADS), 0, st, s);
      dscan_u64(ctx, counts, offs, 256ull * nbt, tot, "gb");
      LAUNCH(k_gb_scatter, dim3(nbt), dim3(GB_THREADS), 0, st, s);
      std::swap(src, dst);
    }
    if (timed) HIPCHK(hipEventRecord(ctx->ev[9], st));
    HIPCHK(hipGetLastError());
    ord = src;
  }

  // ---- group boundaries, keys and tags ----
  GbGroupArgs g = {};
  g.ng = ng;
  g.klen = klen;
  g.mw = k.mw;
  g.nw = k.nw;
  g.vw = k.vw;
  g.tag_stride = tag_stride;
  g.ord = ord;
  g.gkey = k.gkey;
  g.key_off = k.key_off;
  g.key = k.key;
  g.kept = kept;
  g.ntags = k.ntags;
  g.heads = scratch<uint64_t>(ctx, "gb_heads", ng);
  uint64_t* hscan = scratch<uint64_t>(ctx, "gb_hscan", ng);
  g.hscan = hscan;
  g.n_groups = d_ngroups;
  g.gid = scratch<uint32_t>(ctx, "gb_gid", ng);
  g.first = scratch<uint32_t>(ctx, "gb_first", ng);
  g.common = scratch<uint32_t>(ctx, "gb_common", ng);
  g.gss = scratch<uint32_t>(ctx, "gb_gss", (size_t)ng + 1);
  g.out_key = scratch<uint8_t>(ctx, "gb_okey", (size_t)ng * klen);
  g.out_ntags = scratch<uint8_t>(ctx, "gb_ontags", ng);
  g.out_tags = scratch<uint8_t>(ctx, "gb_otags", (size_t)ng * tag_stride);
  g.out_common = scratch<uint8_t>(ctx, "gb_ocommon", ng);
  HIPCHK(hipMemsetAsync(g.first, 0xFF, 4ull * ng, st));
  HIPCHK(hipMemsetAsync(g.common, 0xFF, 4ull * ng, st));
  const dim3 gg(grid_for(ng, 256));
  LAUNCH(k_gb_heads, gg, dim3(256), 0, st, g);
  dscan_u64(ctx, g.heads, hscan, ng, d_ngroups, "gbh");
  LAUNCH(k_gb_emit, gg, dim3(256), 0, st, g);
  LAUNCH(k_gb_first, gg, dim3(256), 0, st, g);
  LAUNCH(k_gb_masks, gg, dim3(256), 0, st, g);
  LAUNCH(k_gb_finalize, gg, dim3(256), 0, st, g);
  HIPCHK(hipGetLastError());
  if (timed) HIPCHK(hipEventRecord(ctx->ev[1], st));
  uint64_t G64 = 0;
  readback(ctx, &G64, d_ngroups, 8);  // [sync 2]
  const uint32_t G = (uint32_t)G64;
  out->n_groups = G;
  if (timed) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]) == hipSuccess) tm.total_ms = ms;
    if (!passes.empty() && hipEventElapsedTime(&ms, ctx->ev[8], ctx->ev[9]) == hipSuccess) tm.hot_ms = ms;
    (void)hipGetLastError();
  }
  tm.n_grid = passes.size();
  tm.h2d_bytes = ctx->h2d_bytes;
  if (G > out->group_capacity) {
    ctx->timing = tm;
    set_error(ctx, "tsdbhip_groupby_plan: %u groups, capacity %u", G, out->group_capacity);
    return TSDBHIP_E_CAPACITY;
  }
  HIPCHK(hipMemcpyAsync(out->order, ord, 4ull * ng, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(out->group_span_start, g.gss, 4ull * (G + 1), hipMemcpyDeviceToHost, st));
  if (klen) HIPCHK(hipMemcpyAsync(out->group_key, g.out_key, (size_t)G * klen, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(out->group_ntags, g.out_ntags, G, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(out->group_tags, g.out_tags, (size_t)G * tag_stride, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(out->group_common, g.out_common, G, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));  // [sync 3]
  tm.alg_bytes += 4ull * ng + 4ull * (G + 1) + (uint64_t)G * (klen + tag_stride + 2);
  ctx->timing = tm;
  return TSDBHIP_OK;
}

extern "C" int tsdbhip_groupby_plan(tsdbhip_ctx* c, const tsdbhip_keys_desc* d, tsdbhip_groups_out* out) {
  if (!c || !d || !out) return TSDBHIP_E_INVALID_ARG;
  try {
    Lease L(plain_of(c));
    return groupby_plan(L.s, d, out);
  } catch (Fail& f) {
    return f.code;
  }
}

// ------------------------------------------------------------ gather ------
// The gathered descriptor's six arrays are owned by the context under keys
// derived from the address of `out`, like a generated dataset's.
static const char* const GATHER_FIELDS[] = {"srs", "base", "ncells", "qoff", "voff", "vlen"};
static std::string gather_key(const tsdbhip_sg_desc* d, const char* f) {
  char b[64];
  snprintf(b, sizeof b, "gth%p_%s", (const void*)d, f);
  return b;
}

extern "C" int tsdbhip_desc_gather(tsdbhip_ctx* c, const tsdbhip_sg_desc* in, const uint32_t* order, uint32_t n,
                                   tsdbhip_sg_desc* out) {
  if (!c || !in || !out || in == out || (n && !order)) return TSDBHIP_E_INVALID_ARG;
  if (!(in->flags & TSDBHIP_DESC_DEVICE) || (in->flags & TSDBHIP_SHARDED)) {
    set_error(c, "tsdbhip_desc_gather: the input must be a device-resident, unsharded descriptor");
    return TSDBHIP_E_INVALID_ARG;
  }
  const int64_t bad = gather_check_order(order, n, in->n_spans);
  if (bad >= 0) {
    set_error(c, "tsdbhip_desc_gather: order[%lld] = %u is not a span of the input (%u spans)", (long long)bad,
              order[bad], in->n_spans);
    return TSDBHIP_E_INVALID_ARG;
  }
  c = plain_of(c);
  try {
    Lease L(c);
    Slot* ctx = L.s;
    ctx->timing = tsdbhip_timing();
    hipStream_t st = ctx->stream;
    auto al = [&](const char* f, size_t bytes) -> void* {
      const std::string key = gather_key(out, f);
      void* q = nullptr;
      {
        std::lock_guard<std::mutex> lk(c->mu);
        auto it = c->owned.find(key);
        if (it != c->owned.end()) {
          q = it->second.p;
          c->owned.erase(it);
        }
      }
      if (q) HIPCHK(hipFree(q));
      q = nullptr;
      HIPCHK(hipMalloc(&q, bytes + 64));
      {
        std::lock_guard<std::mutex> lk(c->mu);
        c->owned[key] = Buf{q, bytes + 64};
      }
      HIPCHK(hipMemsetAsync(q, 0, bytes + 64, st));
      return q;
    };
    GatherArgs a = {};
    a.n = n;
    a.in_srs = in->span_row_start;
    a.in_base = in->row_base;
    a.in_ncells = in->row_ncells;
    a.in_qoff = in->row_qual_off;
    a.in_voff = in->row_val_off;
    a.in_vlen = in->row_val_len;
    a.out_srs = (uint64_t*)al("srs", 8ull * ((size_t)n + 1));
    uint64_t total = 0;
    if (n) {
      uint32_t* d_order = scratch<uint32_t>(ctx, "gth_order", n);
      HIPCHK(hipMemcpyAsync(d_order, order, 4ull * n, hipMemcpyHostToDevice, st));
      a.order = d_order;
      a.cnt = scratch<uint64_t>(ctx, "gth_cnt", n);
      LAUNCH(k_gather_count, dim3(grid_for(n, 256)), dim3(256), 0, st, a);
      dscan_u64(ctx, a.cnt, a.out_srs, n, a.out_srs + n, "gth");
      HIPCHK(hipGetLastError());
      readback(ctx, &total, a.out_srs + n, 8);
    }
    a.n_rows = total;
    a.out_base = (uint32_t*)al("base", 4 * total);
    a.out_ncells = (uint32_t*)al("ncells", 4 * total);
    a.out_qoff = (uint64_t*)al("qoff", 8 * total);
    a.out_voff = (uint64_t*)al("voff", 8 * total);
    a.out_vlen = (uint32_t*)al("vlen", 4 * total);
    if (total) LAUNCH(k_gather_rows, dim3(grid_for(total, 256, 0x7fffffff)), dim3(256), 0, st, a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    *out = *in;  // the query fields, the flags, the borrowed qualifier / value bytes
    out->n_spans = n;
    out->n_rows = total;
    out->span_row_start = a.out_srs;
    out->row_base = a.out_base;
    out->row_ncells = a.out_ncells;
    out->row_qual_off = a.out_qoff;
    out->row_val_off = a.out_voff;
    out->row_val_len = a.out_vlen;
    out->span0 = 0;
  } catch (Fail& f) {
    return f.code;
  }
  return TSDBHIP_OK;
}

extern "C" int tsdbhip_desc_gather_free(tsdbhip_ctx* c, tsdbhip_sg_desc* out) {
  if (!c || !out) return TSDBHIP_E_INVALID_ARG;
  c = plain_of(c);
  hipSetDevice(c->device);
  hipDeviceSynchronize();  // (no call may still read the arrays)
  {
    std::lock_guard<std::mutex> lock(c->mu);
    for (const char* f : GATHER_FIELDS) {
      auto it = c->owned.find(gather_key(out, f));
      if (it != c->owned.end()) {
        if (it->second.p) hipFree(it->second.p);
        c->owned.erase(it);
      }
    }
  }
  out->span_row_start = nullptr;
  out->row_base = nullptr;
  out->row_ncells = nullptr;
  out->row_qual_off = nullptr;
  out->row_val_off = nullptr;
  out->row_val_len = nullptr;
  return TSDBHIP_OK;
}
