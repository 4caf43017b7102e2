// scanrows.hip — tsdbhip_scan_rows: the host side of k_scanrows.hip.
// Included by api.hip (unity build).
//
// All on the slot's stream:
//   k_sr_match            the key checks, the range and the tag filter: a flag
//                         and a key length per row
//   two scans             output row, output key offset                [sync 1]
//   k_sr_emit             the outputs (a device table: in place; a host one:
//                         scratch, then copies)                        [sync 2]
// Sync 1 brings the error word and both totals in one readback: an error or a
// capacity miss returns before anything is written.
#include "scanrows_host.h"

// "scan_rows_load" auto: the loader that measured faster, "lds", on all four queries of
// profiles/scan_rows.json
static bool sr_auto_lds() { return true; }

static int scan_rows(Slot* ctx, const tsdbhip_scan_desc* d, const tsdbhip_scan_query* qin, tsdbhip_scan_sel* out) {
  out->n_selected = 0;
  out->key_used = 0;
  ctx->timing = tsdbhip_timing();
  ctx->h2d_bytes = 0;
  ctx->reuse_inputs = false;
  char msg[160];
  if (const char* why = sr_check_args(d, qin, out)) {
    set_error(ctx, "tsdbhip_scan_rows: %s", why);
    return TSDBHIP_E_INVALID_ARG;
  }
  const uint32_t n = d->n_rows;
  const bool dev = (d->flags & TSDBHIP_DESC_DEVICE) != 0;
  hipStream_t st = ctx->stream;
  auto empty = [&]() -> int {
    if (dev) {
      if (out->key_off) HIPCHK(hipMemsetAsync(out->key_off, 0, 8, st));
      HIPCHK(hipStreamSynchronize(st));
    } else if (out->key_off) {
      out->key_off[0] = 0;
    }
    return TSDBHIP_OK;
  };
  if (n == 0) return empty();
  if (!dev) {
    const uint64_t err = sr_first_error(fs_rows_of(d));
    if (err != FS_NO_ERROR) {
      const int rc = fs_error(err, msg, sizeof msg);
      set_error(ctx, "tsdbhip_scan_rows: %s", msg);
      return rc;
    }
  }
  const bool timed = ctx->opt.events != 2;
  const bool cells = d->row_qual_off != nullptr;

  SrMatchArgs k = {};
  std::vector<uint64_t> ids;
  sr_build_query(d, qin, &k.q, &ids);
  k.in = fs_rows_of(d);
  k.in.status = nullptr;  // (passed through unread)
  k.in.qoff = nullptr;
  k.in.qlen = nullptr;
  k.in.key_off = stage(ctx, "sr_koff", d->key_off, (size_t)n + 1, dev);
  k.in.key = stage(ctx, "sr_key", d->key_bytes, d->key_nbytes, dev, 16);
  const uint8_t* in_status = d->row_status ? stage(ctx, "sr_status", d->row_status, n, dev) : nullptr;
  const uint64_t *in_qoff = nullptr, *in_voff = nullptr;
  const uint32_t *in_qlen = nullptr, *in_vlen = nullptr;
  if (cells) {
    in_qoff = stage(ctx, "sr_qoff", d->row_qual_off, n, dev);
    in_qlen = stage(ctx, "sr_qlen", d->row_qual_len, n, dev);
    in_voff = stage(ctx, "sr_voff", d->row_val_off, n, dev);
    in_vlen = stage(ctx, "sr_vlen", d->row_val_len, n, dev);
  }
  {
    uint64_t* d_ids = scratch<uint64_t>(ctx, "sr_ids", ids.size());
    if (!ids.empty()) {  // (pageable: the copy has read it when the call returns to here)
      HIPCHK(hipMemcpyAsync(d_ids, ids.data(), ids.size() * 8, hipMemcpyHostToDevice, st));
      HIPCHK(hipStreamSynchronize(st));
    }
    k.q.ids = d_ids;
  }
  // the call's small state: [0] the error word, [1] rows selected, [2] their key bytes
  uint64_t* sm = scratch<uint64_t>(ctx, "sr_small", 3);
  {
    uint64_t* h = (uint64_t*)ctx->host_small;
    h[0] = FS_NO_ERROR;
    h[1] = h[2] = 0;
    HIPCHK(hipMemcpyAsync(sm, h, 24, hipMemcpyHostToDevice, st));
  }
  k.err = (unsigned long long*)sm;
  k.flags = scratch<uint64_t>(ctx, "sr_flags", n);
  k.klen = scratch<uint64_t>(ctx, "sr_klen", n);
  uint64_t* fscan = scratch<uint64_t>(ctx, "sr_fscan", n);
  uint64_t* kscan = scratch<uint64_t>(ctx, "sr_kscan", n);
  const bool lds = ctx->opt.scan_rows_load < 0 ? sr_auto_lds() : ctx->opt.scan_rows_load == 1;
  const unsigned cap = ctx->opt.scan_rows_blocks > 0 ? (unsigned)ctx->opt.scan_rows_blocks : SR_BLOCKS;
  const unsigned mgrid = grid_for(n, SR_THREADS, cap);
  if (timed) {
    HIPCHK(hipEventRecord(ctx->ev[0], st));
    HIPCHK(hipEventRecord(ctx->ev[8], st));
  }
  if (lds) LAUNCH(k_sr_match<true>, dim3(mgrid), dim3(SR_THREADS), 0, st, k);
  else LAUNCH(k_sr_match<false>, dim3(mgrid), dim3(SR_THREADS), 0, st, k);
  if (timed) HIPCHK(hipEventRecord(ctx->ev[9], st));
  dscan_u64(ctx, k.flags, fscan, n, sm + 1, "srf");
  dscan_u64(ctx, k.klen, kscan, n, sm + 2, "srk");
  HIPCHK(hipGetLastError());
  uint64_t smh[3];
  readback(ctx, smh, sm, sizeof smh);  // [sync 1]
  if (smh[0] != FS_NO_ERROR) {
    const int rc = fs_error(smh[0], msg, sizeof msg);
    set_error(ctx, "tsdbhip_scan_rows: %s", msg);
    return rc;
  }
  const uint32_t S = (uint32_t)smh[1];
  const uint64_t key_used = smh[2];
  tsdbhip_timing tm = {};
  tm.hot_kernel = TSDBHIP_HOT_SCAN_ROWS;
  // the match: offsets and keys read, a flag and a length written; the scans read and write both twice
  tm.alg_bytes = 8ull * ((uint64_t)n + 1) + d->key_nbytes + 16ull * n + 64ull * n;
  auto stamp = [&]() {
    if (timed) {
      float ms = 0;
      if (hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]) == hipSuccess) tm.total_ms = ms;
      if (hipEventElapsedTime(&ms, ctx->ev[8], ctx->ev[9]) == hipSuccess) tm.hot_ms = ms;
      (void)hipGetLastError();
    }
    tm.h2d_bytes = ctx->h2d_bytes;
    ctx->timing = tm;
  };
  out->n_selected = S;
  out->key_used = key_used;
  if (S == 0 || S > out->row_capacity || key_used > out->key_capacity) {
    if (timed) HIPCHK(hipEventRecord(ctx->ev[1], st));
    HIPCHK(hipStreamSynchronize(st));
    stamp();
    if (S == 0) return empty();
    set_error(ctx, "tsdbhip_scan_rows: %u rows (capacity %u), %llu key bytes (capacity %llu)", S, out->row_capacity,
              (unsigned long long)key_used, (unsigned long long)out->key_capacity);
    return TSDBHIP_E_CAPACITY;
  }
  SrEmitArgs a = {};
  a.n = n;
  a.cells = cells;
  a.key_off = k.in.key_off;
  a.key = k.in.key;
  a.status = in_status;
  a.in_qoff = in_qoff;
  a.in_qlen = in_qlen;
  a.in_voff = in_voff;
  a.in_vlen = in_vlen;
  a.flags = k.flags;
  a.fscan = fscan;
  a.kscan = kscan;
  a.totals = sm + 1;
  if (dev) {
    a.row_index = out->row_index;
    a.out_key_off = out->key_off;
    a.out_key = out->key_bytes;
    a.out_status = out->row_status;
    a.out_qoff = out->row_qual_off;
    a.out_qlen = out->row_qual_len;
    a.out_voff = out->row_val_off;
    a.out_vlen = out->row_val_len;
  } else {
    a.row_index = scratch<uint32_t>(ctx, "sr_o_index", S);
    a.out_key_off = scratch<uint64_t>(ctx, "sr_o_koff", (size_t)S + 1);
    a.out_key = scratch<uint8_t>(ctx, "sr_o_key", key_used);
    if (in_status) a.out_status = scratch<uint8_t>(ctx, "sr_o_status", S);
    if (cells) {
      a.out_qoff = scratch<uint64_t>(ctx, "sr_o_qoff", S);
      a.out_qlen = scratch<uint32_t>(ctx, "sr_o_qlen", S);
      a.out_voff = scratch<uint64_t>(ctx, "sr_o_voff", S);
      a.out_vlen = scratch<uint32_t>(ctx, "sr_o_vlen", S);
    }
  }
  LAUNCH(k_sr_emit, dim3(grid_for(n, 256, 0x7fffffff)), dim3(256), 0, st, a);
  HIPCHK(hipGetLastError());
  if (timed) HIPCHK(hipEventRecord(ctx->ev[1], st));
  if (!dev) {
    HIPCHK(hipMemcpyAsync(out->row_index, a.row_index, 4ull * S, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(out->key_off, a.out_key_off, 8ull * (S + 1ull), hipMemcpyDeviceToHost, st));
    if (key_used) HIPCHK(hipMemcpyAsync(out->key_bytes, a.out_key, key_used, hipMemcpyDeviceToHost, st));
    if (in_status) HIPCHK(hipMemcpyAsync(out->row_status, a.out_status, S, hipMemcpyDeviceToHost, st));
    if (cells) {
      HIPCHK(hipMemcpyAsync(out->row_qual_off, a.out_qoff, 8ull * S, hipMemcpyDeviceToHost, st));
      HIPCHK(hipMemcpyAsync(out->row_qual_len, a.out_qlen, 4ull * S, hipMemcpyDeviceToHost, st));
      HIPCHK(hipMemcpyAsync(out->row_val_off, a.out_voff, 8ull * S, hipMemcpyDeviceToHost, st));
      HIPCHK(hipMemcpyAsync(out->row_val_len, a.out_vlen, 4ull * S, hipMemcpyDeviceToHost, st));
    }
  }
  HIPCHK(hipStreamSynchronize(st));  // [sync 2]
  // the emit: flags read, a selected row's scans, offsets and key read; its index, offset, key and metadata written
  tm.alg_bytes += 8ull * n + 32ull * S + 2 * key_used + 12ull * S + (in_status ? 2ull * S : 0) + (cells ? 48ull * S : 0);
  stamp();
  return TSDBHIP_OK;
}

extern "C" int tsdbhip_scan_rows(tsdbhip_ctx* c, const tsdbhip_scan_desc* d, const tsdbhip_scan_query* q,
                                 tsdbhip_scan_sel* out) {
  if (!c || !d || !q || !out) return TSDBHIP_E_INVALID_ARG;
  try {
    Lease L(plain_of(c));
    return scan_rows(L.s, d, q, out);
  } catch (Fail& f) {
    return f.code;
  }
}
