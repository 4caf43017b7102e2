// findspans.hip — tsdbhip_find_spans: the host side of k_findspans.hip.
// Included by api.hip (unity build).
//
// All on the slot's stream:
//   k_fs_keys                       checks, identity, AND / OR of the digits   [sync 1]
//   k_fs_digits                     the live digits, dense
//   per live digit, least significant first: k_gb_count, scan, k_gb_scatter
//   k_fs_heads, two scans           span index / output row, key offsets      [sync 2]
//   k_fs_emit                       the outputs (a device descriptor: in place;
//                                   a host one: scratch, then copies)          [sync 3]
// Sync 1 tells the host the first offending row (an error returns before any
// sort kernel runs) and which digit positions are live; sync 2 the counts,
// checked against the capacities before anything is written.
#include "findspans_host.h"

static int find_spans(Slot* ctx, const tsdbhip_scan_desc* d, tsdbhip_spans_out* out) {
  out->n_spans = out->n_rows = out->n_skipped = 0;
  out->key_used = 0;
  ctx->timing = tsdbhip_timing();
  ctx->h2d_bytes = 0;
  ctx->reuse_inputs = false;
  char msg[160];
  if (const char* why = fs_check_desc(d, out)) {
    set_error(ctx, "tsdbhip_find_spans: %s", why);
    return TSDBHIP_E_INVALID_ARG;
  }
  const uint32_t n = d->n_rows;
  const bool dev = (d->flags & TSDBHIP_DESC_DEVICE) != 0;
  hipStream_t st = ctx->stream;
  auto empty = [&]() -> int {  // no row added: the reference returns null
    if (dev) {
      if (out->span_row_start) HIPCHK(hipMemsetAsync(out->span_row_start, 0, 8, st));
      if (out->key_off) HIPCHK(hipMemsetAsync(out->key_off, 0, 8, st));
      HIPCHK(hipStreamSynchronize(st));
    } else {
      if (out->span_row_start) out->span_row_start[0] = 0;
      if (out->key_off) out->key_off[0] = 0;
    }
    return TSDBHIP_OK;
  };
  if (n == 0) return empty();
  if (!dev) {
    const uint64_t err = fs_first_error(fs_rows_of(d));
    if (err != FS_NO_ERROR) {
      const int rc = fs_error(err, msg, sizeof msg);
      set_error(ctx, "tsdbhip_find_spans: %s", msg);
      return rc;
    }
  }
  const bool timed = ctx->opt.events != 2;
  const bool cells = d->row_qual_off != nullptr;
  const uint32_t P = TSDBHIP_MAX_TAGS * ((uint32_t)d->name_width + d->value_width);

  FsKeysArgs k = {};
  k.in = fs_rows_of(d);
  k.in.key_off = stage(ctx, "fs_koff", d->key_off, (size_t)n + 1, dev);
  k.in.key = stage(ctx, "fs_key", d->key_bytes, d->key_nbytes, dev, 16);
  k.in.status = d->row_status ? stage(ctx, "fs_status", d->row_status, n, dev) : nullptr;
  const uint64_t *in_qoff = nullptr, *in_voff = nullptr;
  const uint32_t *in_qlen = nullptr, *in_vlen = nullptr;
  if (cells) {
    in_qoff = stage(ctx, "fs_qoff", d->row_qual_off, n, dev);
    in_qlen = stage(ctx, "fs_qlen", d->row_qual_len, n, dev);
    in_voff = stage(ctx, "fs_voff", d->row_val_off, n, dev);
    in_vlen = stage(ctx, "fs_vlen", d->row_val_len, n, dev);
  }
  k.in.qoff = in_qoff;
  k.in.qlen = in_qlen;
  k.P = P;
  uint32_t* idx_a = scratch<uint32_t>(ctx, "fs_idx_a", n);
  uint32_t* idx_b = scratch<uint32_t>(ctx, "fs_idx_b", n);
  k.idx0 = idx_a;
  // the call's small state: [0,1] error word, [4,40) AND words, [40,76) OR
  // words, [76,80) the scans' totals
  constexpr size_t SM_WORDS = 80, SM_AND = 4, SM_OR = 40, SM_TOT = 76;
  uint32_t* sm = scratch<uint32_t>(ctx, "fs_small", SM_WORDS);
  {
    uint32_t* h = (uint32_t*)ctx->host_small;
    std::memset(h, 0, SM_WORDS * 4);
    h[0] = h[1] = ~0u;
    for (size_t w = 0; w < FS_WORDS; w++) h[SM_AND + w] = ~0u;
    HIPCHK(hipMemcpyAsync(sm, h, SM_WORDS * 4, hipMemcpyHostToDevice, st));
  }
  k.err = (unsigned long long*)sm;
  k.andw = sm + SM_AND;
  k.orw = sm + SM_OR;
  uint64_t* d_totals = (uint64_t*)(sm + SM_TOT);
  if (timed) HIPCHK(hipEventRecord(ctx->ev[0], st));
  const unsigned grid = grid_for(n, 256, 0x7fffffff);
  LAUNCH(k_fs_keys, dim3(std::min(grid, FS_KEYS_BLOCKS)), dim3(256), 0, st, k);
  HIPCHK(hipGetLastError());
  uint32_t smh[SM_WORDS];
  readback(ctx, smh, sm, sizeof smh);  // [sync 1]
  unsigned long long err;
  std::memcpy(&err, smh, 8);
  if (err != FS_NO_ERROR) {
    const int rc = fs_error(err, msg, sizeof msg);
    set_error(ctx, "tsdbhip_find_spans: %s", msg);
    return rc;
  }
  tsdbhip_timing tm = {};
  tm.hot_kernel = TSDBHIP_HOT_FIND_SPANS;

  // ---- the live digits, dense, and the sort from the least significant ----
  FsDigitArgs g = {};
  g.n = n;
  g.mw = d->metric_width;
  g.nw = d->name_width;
  g.vw = d->value_width;
  g.P = P;
  g.key_off = k.in.key_off;
  g.key = k.in.key;
  uint32_t n_live = 0;
  for (uint32_t p = 0; p <= P; p++) {
    const uint32_t x = (smh[SM_AND + p / 4] ^ smh[SM_OR + p / 4]) >> (8 * (p % 4));
    if (x & 0xFFu) g.live[n_live++] = (uint8_t)p;
  }
  g.n_live = n_live;
  uint8_t* dense = scratch<uint8_t>(ctx, "fs_dense", (size_t)n * n_live);
  g.dense = dense;
  const uint32_t* ord = idx_a;
  if (n_live) {
    LAUNCH(k_fs_digits, dim3(grid), dim3(256), 0, st, g);
    const uint32_t nbt = (n + GB_TILE - 1) / GB_TILE;
    uint64_t* counts = scratch<uint64_t>(ctx, "fs_counts", 256ull * nbt);
    uint64_t* offs = scratch<uint64_t>(ctx, "fs_offs", 256ull * nbt);
    uint64_t* tot = scratch<uint64_t>(ctx, "fs_tot", 1);
    uint32_t *src = idx_a, *dst = idx_b;
    if (timed) HIPCHK(hipEventRecord(ctx->ev[8], st));
    for (uint32_t j = n_live; j-- > 0;) {
      GbSortArgs s = {};
      s.n = n;
      s.nb = nbt;
      s.src = src;
      s.dst = dst;
      s.dig = dense;
      s.stride = n_live;
      s.off = j;
      s.counts = counts;
      s.offs = offs;
      LAUNCH(k_gb_count, dim3(nbt), dim3(GB_THREADS), 0, st, s);
      dscan_u64(ctx, counts, offs, 256ull * nbt, tot, "fs");
      LAUNCH(k_gb_scatter, dim3(nbt), dim3(GB_THREADS), 0, st, s);
      std::swap(src, dst);
    }
    if (timed) HIPCHK(hipEventRecord(ctx->ev[9], st));
    HIPCHK(hipGetLastError());
    ord = src;
  }

  // ---- span boundaries and output positions ----
  FsSpanArgs a = {};
  a.n = n;
  a.n_live = n_live;
  a.mw = d->metric_width;
  a.cells = cells;
  a.ord = ord;
  a.dense = dense;
  a.key_off = k.in.key_off;
  a.key = k.in.key;
  a.status = k.in.status;
  a.in_qoff = in_qoff;
  a.in_qlen = in_qlen;
  a.in_voff = in_voff;
  a.in_vlen = in_vlen;
  a.flags = scratch<uint64_t>(ctx, "fs_flags", n);
  uint64_t* fscan = scratch<uint64_t>(ctx, "fs_fscan", n);
  a.fscan = fscan;
  a.klen = scratch<uint64_t>(ctx, "fs_klen", n);
  uint64_t* kscan = scratch<uint64_t>(ctx, "fs_kscan", n);
  a.kscan = kscan;
  a.totals = d_totals;
  LAUNCH(k_fs_heads, dim3(grid), dim3(256), 0, st, a);
  dscan_u64(ctx, a.flags, fscan, n, d_totals, "fsf");
  dscan_u64(ctx, a.klen, kscan, n, d_totals + 1, "fsk");
  HIPCHK(hipGetLastError());
  uint64_t tot[2] = {0, 0};
  readback(ctx, tot, d_totals, sizeof tot);  // [sync 2]
  const uint32_t S = (uint32_t)(tot[0] >> 32), R = (uint32_t)tot[0];
  const uint64_t key_used = tot[1];
  out->n_skipped = n - R;
  tm.n_grid = n_live;
  const uint64_t in_bytes = 8ull * ((uint64_t)n + 1) + (k.in.status ? n : 0) + (cells ? 24ull * n : 0);
  // keys read twice (k_fs_keys, k_fs_digits); a pass reads index + digit twice and writes the index
  tm.alg_bytes = 2 * d->key_nbytes + in_bytes + (uint64_t)n * n_live + (uint64_t)n_live * 14ull * n;
  auto stamp = [&]() {
    if (timed) {
      float ms = 0;
      if (hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]) == hipSuccess) tm.total_ms = ms;
      if (n_live && hipEventElapsedTime(&ms, ctx->ev[8], ctx->ev[9]) == hipSuccess) tm.hot_ms = ms;
      (void)hipGetLastError();
    }
    tm.h2d_bytes = ctx->h2d_bytes;
    ctx->timing = tm;
  };
  if (R == 0) {  // every row NONE
    if (timed) HIPCHK(hipEventRecord(ctx->ev[1], st));
    HIPCHK(hipStreamSynchronize(st));
    stamp();
    return empty();
  }
  out->n_spans = S;
  out->n_rows = R;
  out->key_used = key_used;
  if (S > out->span_capacity || key_used > out->key_capacity) {
    if (timed) HIPCHK(hipEventRecord(ctx->ev[1], st));
    HIPCHK(hipStreamSynchronize(st));
    stamp();
    set_error(ctx, "tsdbhip_find_spans: %u spans (capacity %u), %llu key bytes (capacity %llu)", S,
              out->span_capacity, (unsigned long long)key_used, (unsigned long long)out->key_capacity);
    return TSDBHIP_E_CAPACITY;
  }
  if (dev) {
    a.row_order = out->row_order;
    a.span_row_start = out->span_row_start;
    a.row_base = out->row_base;
    a.row_ncells = out->row_ncells;
    a.row_qual_off = out->row_qual_off;
    a.row_val_off = out->row_val_off;
    a.row_val_len = out->row_val_len;
    a.out_key_off = out->key_off;
    a.out_key = out->key_bytes;
  } else {
    a.row_order = scratch<uint32_t>(ctx, "fs_o_order", R);
    a.span_row_start = scratch<uint64_t>(ctx, "fs_o_srs", (size_t)S + 1);
    a.row_base = scratch<uint32_t>(ctx, "fs_o_base", R);
    a.out_key_off = scratch<uint64_t>(ctx, "fs_o_koff", (size_t)S + 1);
    a.out_key = scratch<uint8_t>(ctx, "fs_o_key", key_used);
    if (cells) {
      a.row_ncells = scratch<uint32_t>(ctx, "fs_o_ncells", R);
      a.row_qual_off = scratch<uint64_t>(ctx, "fs_o_qoff", R);
      a.row_val_off = scratch<uint64_t>(ctx, "fs_o_voff", R);
      a.row_val_len = scratch<uint32_t>(ctx, "fs_o_vlen", R);
    }
  }
  LAUNCH(k_fs_emit, dim3(grid), dim3(256), 0, st, a);
  HIPCHK(hipGetLastError());
  if (timed) HIPCHK(hipEventRecord(ctx->ev[1], st));
  if (!dev) {
    HIPCHK(hipMemcpyAsync(out->row_order, a.row_order, 4ull * R, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(out->span_row_start, a.span_row_start, 8ull * (S + 1ull), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(out->row_base, a.row_base, 4ull * R, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(out->key_off, a.out_key_off, 8ull * (S + 1ull), hipMemcpyDeviceToHost, st));
    if (key_used) HIPCHK(hipMemcpyAsync(out->key_bytes, a.out_key, key_used, hipMemcpyDeviceToHost, st));
    if (cells) {
      HIPCHK(hipMemcpyAsync(out->row_ncells, a.row_ncells, 4ull * R, hipMemcpyDeviceToHost, st));
      HIPCHK(hipMemcpyAsync(out->row_qual_off, a.row_qual_off, 8ull * R, hipMemcpyDeviceToHost, st));
      HIPCHK(hipMemcpyAsync(out->row_val_off, a.row_val_off, 8ull * R, hipMemcpyDeviceToHost, st));
      HIPCHK(hipMemcpyAsync(out->row_val_len, a.row_val_len, 4ull * R, hipMemcpyDeviceToHost, st));
    }
  }
  HIPCHK(hipStreamSynchronize(st));  // [sync 3]
  // heads + scans, then the outputs: the order, the base times, the cells, the span arrays and keys
  tm.alg_bytes += 48ull * n + 2 * key_used + 8ull * R + (cells ? 48ull * R : 0) + 16ull * (S + 1ull);
  stamp();
  return TSDBHIP_OK;
}

extern "C" int tsdbhip_find_spans(tsdbhip_ctx* c, const tsdbhip_scan_desc* d, tsdbhip_spans_out* out) {
  if (!c || !d || !out) return TSDBHIP_E_INVALID_ARG;
  try {
    Lease L(plain_of(c));
    return find_spans(L.s, d, out);
  } catch (Fail& f) {
    return f.code;
  }
}
