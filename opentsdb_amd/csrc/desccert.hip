// desccert.hip — tsdbhip_desc_certify: the host side of k_desccert.hip.
// Included by api.hip (unity build), before the producers that certify what
// they produced (tsdbhip_synth_generate, tsdbhip_desc_pack).
//
// On the slot's stream: the count cleared, k_desc_certify, one readback of the
// count (the call's only sync). The grid is one resident generation of blocks
// at most, each wave striding over the rows.

// the blocks of k_desc_certify resident on the slot's device (cached a device)
static unsigned cert_resident(Slot* ctx) {
  static std::mutex mu;
  static std::map<int, unsigned> res;
  std::lock_guard<std::mutex> lk(mu);
  unsigned& r = res[ctx->device];
  if (!r) {
    int cu = 0, nb = 0;
    if (hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, ctx->device) != hipSuccess || cu < 1) cu = 1;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, (const void*)k_desc_certify, CERT_THREADS, 0) != hipSuccess ||
        nb < 1)
      nb = 1;
    (void)hipGetLastError();
    r = (unsigned)cu * (unsigned)nb;
  }
  return r;
}

// The rows of the device descriptor d that fail TSDBHIP_DESC_QUALS_PROVEN's
// statement. `timing`: the call is tsdbhip_desc_certify itself and leaves its
// tsdbhip_timing (a producer keeps its own).
static uint64_t cert_count(Slot* ctx, const tsdbhip_sg_desc* d, bool timing) {
  hipStream_t st = ctx->stream;
  const bool timed = timing && ctx->opt.events != 2;
  if (timing) {
    ctx->timing = tsdbhip_timing();
    ctx->h2d_bytes = 0;
  }
  uint64_t bad = 0;
  if (timed) HIPCHK(hipEventRecord(ctx->ev[0], st));
  if (d->n_rows) {
    CertArgs a = {};
    a.n_rows = d->n_rows;
    a.ncells = d->row_ncells;
    a.qoff = d->row_qual_off;
    a.qual = d->qual_bytes;
    a.qn = d->qual_nbytes;
    a.n_bad = scratch<unsigned long long>(ctx, "cert_bad", 1);
    HIPCHK(hipMemsetAsync(a.n_bad, 0, 8, st));
    const unsigned grid = grid_for(d->n_rows, CERT_WAVES, cert_resident(ctx));
    if (timed) HIPCHK(hipEventRecord(ctx->ev[8], st));
    LAUNCH(k_desc_certify, dim3(grid), dim3(CERT_THREADS), 0, st, a);
    if (timed) HIPCHK(hipEventRecord(ctx->ev[9], st));
    HIPCHK(hipGetLastError());
    if (timed) HIPCHK(hipEventRecord(ctx->ev[1], st));
    readback(ctx, &bad, a.n_bad, 8);
  } else if (timed) {
    HIPCHK(hipEventRecord(ctx->ev[1], st));
    HIPCHK(hipStreamSynchronize(st));
  }
  if (timing) {
    tsdbhip_timing tm = {};
    tm.hot_kernel = TSDBHIP_HOT_DESC_CERTIFY;
    tm.alg_bytes = d->qual_nbytes + 12ull * d->n_rows;  // the qualifier buffer (the rows lie inside it), two fields a row
    if (timed) {
      float ms = 0;
      if (hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]) == hipSuccess) tm.total_ms = ms;
      if (d->n_rows && hipEventElapsedTime(&ms, ctx->ev[8], ctx->ev[9]) == hipSuccess) tm.hot_ms = ms;
      (void)hipGetLastError();
    }
    ctx->timing = tm;
  }
  return bad;
}

// ... and the flag set or cleared accordingly
static void cert_stamp(Slot* ctx, tsdbhip_sg_desc* d) {
  if (cert_count(ctx, d, false) == 0) d->flags |= TSDBHIP_DESC_QUALS_PROVEN;
  else d->flags &= ~TSDBHIP_DESC_QUALS_PROVEN;
}

extern "C" int tsdbhip_desc_certify(tsdbhip_ctx* c, tsdbhip_sg_desc* d, uint64_t* n_unproven_rows) {
  if (!c || !d) return TSDBHIP_E_INVALID_ARG;
  if (!(d->flags & TSDBHIP_DESC_DEVICE)) {
    set_error(c, "tsdbhip_desc_certify: the descriptor is not device resident");
    return TSDBHIP_E_INVALID_ARG;
  }
  if (d->n_rows && (!d->row_ncells || !d->row_qual_off || !d->qual_bytes)) {
    set_error(c, "tsdbhip_desc_certify: a row array of the descriptor is NULL");
    return TSDBHIP_E_INVALID_ARG;
  }
  c = plain_of(c);
  try {
    Lease L(c);
    const uint64_t bad = cert_count(L.s, d, true);
    if (n_unproven_rows) *n_unproven_rows = bad;
    if (bad == 0) d->flags |= TSDBHIP_DESC_QUALS_PROVEN;
    else d->flags &= ~TSDBHIP_DESC_QUALS_PROVEN;
  } catch (Fail& f) {
    return f.code;
  }
  return TSDBHIP_OK;
}
