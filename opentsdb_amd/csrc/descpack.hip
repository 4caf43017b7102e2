// descpack.hip — tsdbhip_desc_pack: the host side of k_descpack.hip.
// Included by api.hip (unity build).
//
// All on the slot's stream:
//   k_gather_count, scan                 span_row_start                       [sync 1]
//   k_gather_rows                        the rows' metadata, source offsets
//   k_pack_sizes, three scans            the bounds check, the new offsets,
//                                        the piece starts                     [sync 2]
//   k_pack_copy                          the bytes                            [sync 3]
// Sync 1 sizes the row arrays. Sync 2 brings the error word and the three
// totals in one readback: an offending row returns before any byte is read and
// before *out is written. The arrays become the context's (and *out is
// written) only when the call has succeeded; until then they are the call's.
#include "descpack_host.h"

// "desc_pack_load" auto: "unaligned". The two loaders tie on the C3* class shape of profiles/desc_pack.json
// (medians inside each other's ranges) and "unaligned" is the faster one on its two smaller shapes
static bool pack_auto_shift() { return false; }

static const char* const PACK_FIELDS[] = {"srs", "base", "ncells", "qoff", "voff", "vlen", "qual", "val"};
static std::string pack_key(const tsdbhip_sg_desc* d, const char* f) {
  char b[64];
  snprintf(b, sizeof b, "pck%p_%s", (const void*)d, f);
  return b;
}

namespace {
// the call's allocations until they are committed to the context
struct PackBufs {
  void* p[8] = {};
  size_t n[8] = {};
  ~PackBufs() {
    for (void* q : p)
      if (q) hipFree(q);
  }
};
}  // namespace

// the context's arrays of a packed descriptor at `out` (none: nothing happens)
static void pack_release(tsdbhip_ctx* c, const tsdbhip_sg_desc* out) {
  std::lock_guard<std::mutex> lock(c->mu);
  for (const char* f : PACK_FIELDS) {
    auto it = c->owned.find(pack_key(out, f));
    if (it != c->owned.end()) {
      if (it->second.p) hipFree(it->second.p);
      c->owned.erase(it);
    }
  }
}

static int desc_pack(tsdbhip_ctx* c, Slot* ctx, const tsdbhip_sg_desc* in, const uint32_t* order, uint32_t n,
                     tsdbhip_sg_desc* out) {
  ctx->timing = tsdbhip_timing();
  ctx->h2d_bytes = 0;
  ctx->reuse_inputs = false;
  hipStream_t st = ctx->stream;
  const bool timed = ctx->opt.events != 2;
  PackBufs B;
  // field f of PACK_FIELDS: `bytes` and 64 more; the first `zero` of them cleared
  auto al = [&](int f, size_t bytes, size_t zero) -> void* {
    HIPCHK(hipMalloc(&B.p[f], bytes + 64));
    B.n[f] = bytes + 64;
    if (zero) HIPCHK(hipMemsetAsync(B.p[f], 0, zero, st));
    return B.p[f];
  };
  if (timed) HIPCHK(hipEventRecord(ctx->ev[0], st));
  GatherArgs a = {};
  a.n = n;
  a.in_srs = in->span_row_start;
  a.in_base = in->row_base;
  a.in_ncells = in->row_ncells;
  a.in_qoff = in->row_qual_off;
  a.in_voff = in->row_val_off;
  a.in_vlen = in->row_val_len;
  a.out_srs = (uint64_t*)al(0, 8ull * ((size_t)n + 1), 8ull * ((size_t)n + 1) + 64);
  uint64_t total = 0;
  std::vector<uint32_t> every;
  if (n) {
    if (!order) {  // every span in its own order
      every.resize(n);
      for (uint32_t i = 0; i < n; i++) every[i] = i;
      order = every.data();
    }
    uint32_t* d_order = scratch<uint32_t>(ctx, "pck_order", n);
    HIPCHK(hipMemcpyAsync(d_order, order, 4ull * n, hipMemcpyHostToDevice, st));
    a.order = d_order;
    a.cnt = scratch<uint64_t>(ctx, "pck_cnt", n);
    LAUNCH(k_gather_count, dim3(grid_for(n, 256)), dim3(256), 0, st, a);
    dscan_u64(ctx, a.cnt, a.out_srs, n, a.out_srs + n, "pck");
    HIPCHK(hipGetLastError());
    readback(ctx, &total, a.out_srs + n, 8);  // [sync 1]
  }
  a.n_rows = total;
  a.out_base = (uint32_t*)al(1, 4 * total, 4 * total + 64);
  a.out_ncells = (uint32_t*)al(2, 4 * total, 4 * total + 64);
  a.out_qoff = (uint64_t*)al(3, 8 * total, 8 * total + 64);
  a.out_voff = (uint64_t*)al(4, 8 * total, 8 * total + 64);
  a.out_vlen = (uint32_t*)al(5, 4 * total, 4 * total + 64);
  // the call's small state: [0] the error word, [1] row bytes, [2] qualifier extent, [3] value extent, [4] pieces
  uint64_t smh[5] = {PK_NO_ERROR, 0, 0, 0, 0};
  PackArgs k = {};
  PackCopyArgs cp = {};
  const uint64_t* pstart = nullptr;
  if (total) {
    LAUNCH(k_gather_rows, dim3(grid_for(total, 256, 0x7fffffff)), dim3(256), 0, st, a);
    uint64_t* sm = scratch<uint64_t>(ctx, "pck_small", 5);
    std::memcpy(ctx->host_small, smh, sizeof smh);
    HIPCHK(hipMemcpyAsync(sm, ctx->host_small, sizeof smh, hipMemcpyHostToDevice, st));
    k.n_rows = total;
    k.ncells = a.out_ncells;
    k.vlen = a.out_vlen;
    k.g_qoff = a.out_qoff;
    k.g_voff = a.out_voff;
    k.src_qoff = scratch<uint64_t>(ctx, "pck_sqoff", total);
    k.src_voff = scratch<uint64_t>(ctx, "pck_svoff", total);
    k.in_qn = in->qual_nbytes;
    k.in_vn = in->val_nbytes;
    k.err = (unsigned long long*)sm;
    k.row_bytes = sm + 1;
    k.qsz = scratch<uint64_t>(ctx, "pck_qsz", total);
    k.vsz = scratch<uint64_t>(ctx, "pck_vsz", total);
    k.pcs = scratch<uint64_t>(ctx, "pck_pcs", total);
    uint64_t* d_pstart = scratch<uint64_t>(ctx, "pck_pstart", total);
    LAUNCH(k_pack_sizes, dim3(grid_for(total, 256, 0x7fffffff)), dim3(256), 0, st, k);
    // (the source offsets are saved: the scans may now write the new ones over them)
    dscan_u64(ctx, k.qsz, a.out_qoff, total, sm + 2, "pckq");
    dscan_u64(ctx, k.vsz, a.out_voff, total, sm + 3, "pckv");
    dscan_u64(ctx, k.pcs, d_pstart, total, sm + 4, "pckp");
    HIPCHK(hipGetLastError());
    readback(ctx, smh, sm, sizeof smh);  // [sync 2]
    pstart = d_pstart;
  }
  if (smh[0] != PK_NO_ERROR) {
    set_error(ctx, "tsdbhip_desc_pack: gathered row %llu lies outside the input's qual_bytes / val_bytes",
              (unsigned long long)smh[0]);
    return TSDBHIP_E_INVALID_ARG;
  }
  const uint64_t q_used = smh[2], v_used = smh[3];
  const uint64_t qn = pack_nbytes(q_used), vn = pack_nbytes(v_used);
  // the copy stores every byte of [0, used): only the tail up to nbytes + 64 is cleared
  cp.n_rows = total;
  cp.n_pieces = smh[4];
  cp.in_qual = in->qual_bytes;
  cp.in_val = in->val_bytes;
  cp.out_qual = (uint8_t*)al(6, qn, 0);
  cp.out_val = (uint8_t*)al(7, vn, 0);
  HIPCHK(hipMemsetAsync(cp.out_qual + q_used, 0, qn + 64 - q_used, st));
  HIPCHK(hipMemsetAsync(cp.out_val + v_used, 0, vn + 64 - v_used, st));
  if (total) {
    const bool shift = ctx->opt.desc_pack_load < 0 ? pack_auto_shift() : ctx->opt.desc_pack_load == 1;
    // the piece blocks, then the blocks that look at every row and copy the small ones
    cp.piece_blocks = cp.n_pieces ? grid_for((cp.n_pieces + PK_RUN - 1) / PK_RUN, PK_WAVES, 1u << 24) : 0;
    const unsigned grid = cp.piece_blocks + grid_for(total, PK_THREADS, 1u << 24);
    if (timed) HIPCHK(hipEventRecord(ctx->ev[8], st));
    auto go = [&](auto kern) {
      LAUNCH(kern, dim3(grid), dim3(PK_THREADS), 0, st, cp, pstart, (const uint32_t*)a.out_ncells,
             (const uint32_t*)a.out_vlen, (const uint64_t*)k.src_qoff, (const uint64_t*)k.src_voff,
             (const uint64_t*)a.out_qoff, (const uint64_t*)a.out_voff);
    };
    if (shift) go(k_pack_copy<true>);
    else go(k_pack_copy<false>);
    if (timed) HIPCHK(hipEventRecord(ctx->ev[9], st));
    HIPCHK(hipGetLastError());
  }
  if (timed) HIPCHK(hipEventRecord(ctx->ev[1], st));
  HIPCHK(hipStreamSynchronize(st));  // [sync 3]
  tsdbhip_timing tm = {};
  tm.hot_kernel = TSDBHIP_HOT_DESC_PACK;
  // the rows' bytes read, the buffers written (tails included); the metadata: the order and the spans' row
  // ranges read, span_row_start written, 28 B a row gathered (read and written), the new offsets written
  tm.alg_bytes = smh[1] + (qn + 64) + (vn + 64) + 4ull * n + 16ull * n + 8ull * ((uint64_t)n + 1) + 56ull * total +
                 16ull * total;
  if (timed) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]) == hipSuccess) tm.total_ms = ms;
    if (total && hipEventElapsedTime(&ms, ctx->ev[8], ctx->ev[9]) == hipSuccess) tm.hot_ms = ms;
    (void)hipGetLastError();
  }
  ctx->timing = tm;
  // commit: a descriptor packed at this address before gives way
  pack_release(c, out);
  {
    std::lock_guard<std::mutex> lk(c->mu);
    for (int f = 0; f < 8; f++) {
      c->owned[pack_key(out, PACK_FIELDS[f])] = Buf{B.p[f], B.n[f]};
      B.p[f] = nullptr;
    }
  }
  *out = *in;  // the query fields and the flags
  out->n_spans = n;
  out->n_rows = total;
  out->span_row_start = a.out_srs;
  out->row_base = a.out_base;
  out->row_ncells = a.out_ncells;
  out->row_qual_off = a.out_qoff;
  out->row_val_off = a.out_voff;
  out->row_val_len = a.out_vlen;
  out->qual_bytes = cp.out_qual;
  out->qual_nbytes = qn;
  out->val_bytes = cp.out_val;
  out->val_nbytes = vn;
  out->span0 = 0;
  // the certificate: an input's is handed on (the copied bytes are the same bytes), else the output is
  // proven as tsdbhip_desc_certify would (outside the call's timing, which stays the copy's)
  if (!(out->flags & TSDBHIP_DESC_QUALS_PROVEN)) cert_stamp(ctx, out);
  return TSDBHIP_OK;
}

extern "C" int tsdbhip_desc_pack(tsdbhip_ctx* c, const tsdbhip_sg_desc* in, const uint32_t* order, uint32_t n,
                                 tsdbhip_sg_desc* out) {
  if (!c || !in || !out) return TSDBHIP_E_INVALID_ARG;
  if (const char* why = pack_check_args(in, order, n, out)) {
    set_error(c, "tsdbhip_desc_pack: %s", why);
    return TSDBHIP_E_INVALID_ARG;
  }
  if (order) {
    const int64_t bad = gather_check_order(order, n, in->n_spans);
    if (bad >= 0) {
      set_error(c, "tsdbhip_desc_pack: order[%lld] = %u is not a span of the input (%u spans)", (long long)bad,
                order[bad], in->n_spans);
      return TSDBHIP_E_INVALID_ARG;
    }
  }
  c = plain_of(c);
  try {
    Lease L(c);
    return desc_pack(c, L.s, in, order, n, out);
  } catch (Fail& f) {
    return f.code;
  }
}

extern "C" int tsdbhip_desc_pack_free(tsdbhip_ctx* c, tsdbhip_sg_desc* out) {
  if (!c || !out) return TSDBHIP_E_INVALID_ARG;
  c = plain_of(c);
  hipSetDevice(c->device);
  hipDeviceSynchronize();  // (no call may still read the arrays)
  pack_release(c, out);
  out->span_row_start = nullptr;
  out->row_base = nullptr;
  out->row_ncells = nullptr;
  out->row_qual_off = nullptr;
  out->row_val_off = nullptr;
  out->row_val_len = nullptr;
  out->qual_bytes = nullptr;
  out->val_bytes = nullptr;
  out->qual_nbytes = 0;
  out->val_nbytes = 0;
  return TSDBHIP_OK;
}
