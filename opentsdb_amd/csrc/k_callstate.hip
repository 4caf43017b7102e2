// k_callstate.hip — the device state of one spangroup_run call (Small), the
// mapped output block's header, and the kernels that move, publish, snapshot
// and reset that state. Included by api.hip (unity build), at global scope
// after `using namespace tsdb`: the host parts share these types.
#pragma once

// segments of the k_ds_reg / k_ds_spans leftover lists (Small.seg, Small.seg2)
constexpr uint32_t CK_NSEG = 64;
// The mapped output block's header: the call-state snapshot (Small), the
// call's end stamp in its last word (small_snap / check_stamp)
constexpr size_t OUT_HDR = 1024;
// fields one packed agreement moves at most (XMove, xchg_minmax)
constexpr uint32_t XM_MAX = 14;

// Device state of one spangroup_run call (err_raise keys, grid range, flags,
// counters); read back at the call's host round trips.
struct Small {
  unsigned long long err;  // first error (err_raise key), ERR_NONE: none
  uint32_t gflags[2];
  uint32_t reserved;
  unsigned long long range[2];
  unsigned long long fstar;
  unsigned long long n_input;
  unsigned long long nan_t;
  unsigned long long bad_at;
  uint64_t n_kept;
  uint64_t e_total;
  uint64_t T;
  unsigned long long bound[4];  // [min first ts, max last ts, max first ts, min last ts] of the kept spans
  uint32_t cnt[6];  // list counters, zero at the start of a call (no memsets):
                    // [0] assembly queue, [1] decode fallback, [2] direct list,
                    // [3] [4] k_ds_spans int / float leftovers, [5] lockstep
                    // proposal
  uint32_t seg[CK_NSEG];  // k_ds_spans integer leftovers, per segment
  uint32_t seg2[CK_NSEG];  // k_ds_reg leftovers, per segment
  // k_ds_reg's aligned-group reduction (FAP): the spans' class keys
  // (t0 << 32 | n, step) as [min, max, min, max], and a span outside it
  unsigned long long fap_key[4];
  uint32_t fap_broken, fap_done;  // (fap_done: the optimistic finish wrote the results)
  unsigned long long fap_valid;    // this rank's aligned-group partials stand (MIN over ranks when sharded)
  // sharded calls: two 64-bit hashes of the rank's grid bitmap (k_grid_popc /
  // k_grid_scan_blocks), and the agreed header words of the one collective
  // after the local grids (XH_*: MIN, or complemented MAX, over the ranks)
  unsigned long long ghash[2];
  // the lockstep proposal (k_direct_opt): class keys [min, max, min, max];
  // ls_broken: k_lockstep found a qualifier off the proposal (MAX over ranks)
  unsigned long long ls_key[4];
  uint32_t ls_broken, ls_pad;
  unsigned long long xh[14];  // (XH_N, + the aligned-group validity in an optimistic call)
  // the uniform-group proposal (assembly): the kept spans' class keys
  // (x0 << 32 | n, step << 32 | q0) as [min, max, min, max]; a span that
  // proposes none holds ~0 in the first word
  unsigned long long ukey[4];
  uint32_t ug_done;   // k_ug_ds_reg's blocks done (its last block runs the tail)
  uint32_t ug_tried;  // (speculative k_ug_ds_reg) the group was attempted
  uint32_t ug_go;     // (speculative) ug_spec_fits() of the kept spans, by the kept-list kernel
  uint32_t ug_pad2;
};
// Small.xh slots of the grid-agreement header. Every rank decides from these
// agreed words alone (never from its own lo / hi against them), so the ranks
// take the same branch: the grids agree iff min lo == max lo, min hi == max
// hi and both hashes are equal everywhere (the hashes are over word indices
// relative to each rank's own lo; equal lo makes them comparable)
enum { XH_ERR = 0, XH_GF0, XH_GF1, XH_FSTAR, XH_LO, XH_HI, XH_H1MIN, XH_H1MAX, XH_H2MIN, XH_H2MAX, XH_LOMAX, XH_HIMIN, XH_N };

// the agreement test on the agreed header (identical on every rank)
__host__ __device__ inline bool xh_grids_agree(const unsigned long long* xh) {
  return xh[XH_LO] == ~xh[XH_LOMAX] && ~xh[XH_HI] == xh[XH_HIMIN] && xh[XH_H1MIN] == ~xh[XH_H1MAX] &&
         xh[XH_H2MIN] == ~xh[XH_H2MAX];
}
static_assert(sizeof(Small) <= OUT_HDR - 8, "Small and the call's stamp must fit the output header");

// Packing of small call-state fields for one MIN allreduce (a MAX field
// travels complemented): one thread moves up to 8 words in or out of a
// contiguous u64 buffer. kinds: 0 u64, 1 ~u64, 2 ~u32 (to u64); out: the same
// inverses.
struct XMove {
  uint32_t n;
  uint8_t kind[XM_MAX];
  uint64_t* buf;          // [n] the packed words
  void* field[XM_MAX];    // the call-state fields
  uint64_t imm[XM_MAX];   // kinds 3 / 4
  int32_t out;            // 0: fields -> buf, 1: buf -> fields
};
DEVI void xmove_one(const XMove& m, uint32_t i) {
  const uint8_t k = m.kind[i];
  const bool cpl = k == 1 || k == 2 || k == 4 || k == 6;  // MAX kinds travel complemented
  if (!m.out) {
    const uint64_t v = k == 2 ? (uint64_t)*(const uint32_t*)m.field[i]
                       : (k == 3 || k == 4) ? m.imm[i] : *(const uint64_t*)m.field[i];
    m.buf[i] = cpl ? ~v : v;
  } else if (k <= 2) {
    const uint64_t v = cpl ? ~m.buf[i] : m.buf[i];
    if (k == 2) *(uint32_t*)m.field[i] = (uint32_t)v;
    else *(uint64_t*)m.field[i] = v;
  }
}
DEVI void xmove_run(const XMove& m) {
  for (uint32_t i = 0; i < m.n; i++) xmove_one(m, i);
}
// a thread a field (one thread walking them paid a dependent round trip each:
// 6.7 us for the 12-field header)
__global__ void __launch_bounds__(64) k_xmove(XMove m) {
  if (threadIdx.x < m.n) xmove_one(m, threadIdx.x);
}

// dst (global geometry [dst_lo, ...]) = src (a rank's bitmap over [src_lo,
// ...], src_lo >= dst_lo) shifted into place; bits outside src read as 0.
__global__ void __launch_bounds__(256) k_bitmap_remap(const uint32_t* src, uint64_t src_words, int64_t src_lo,
                                                      uint32_t* dst, uint64_t dst_words, int64_t dst_lo) {
  const uint64_t w = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (w >= dst_words) return;
  const int64_t sb = (int64_t)(32 * w) - (src_lo - dst_lo);  // src bit of dst bit 32 w
  const int64_t i0 = sb >= 0 ? sb / 32 : -((31 - sb) / 32);   // floor(sb / 32)
  const uint32_t sh = (uint32_t)(sb - 32 * i0);
  auto at = [&](int64_t i) { return i >= 0 && (uint64_t)i < src_words ? src[i] : 0u; };
  const uint32_t a = at(i0), b = at(i0 + 1);
  dst[w] = sh ? (a >> sh) | (b << (32 - sh)) : a;
}

// The call state to the host (host_publish) after a producer that could not
// publish it itself (a multi-block kernel, a collective).
__global__ void __launch_bounds__(64) k_publish(HostPub pub, const uint64_t* src) { host_publish(pub, src); }

// The call state's snapshot into mapped host memory and, with `init`, its
// reset: word by word over the block's threads, every thread of the block
// calling (one thread copying the ~1 KB across PCIe took most of a 10-12 us
// single-block launch)
static_assert(sizeof(Small) % 8 == 0, "Small is copied in 8-byte words");
// The call's stamp (the word after the snapshot, OUT_HDR - 8): the call's
// sequence number, stored last by thread 0 with a system-scope release once
// every thread's snapshot words are fenced. Every host-visible result of the
// call was written before it: the finalize's small results into the same
// mapped block and the reduce's long results into registered caller buffers
// by kernels that completed earlier in the stream, the aligned-group finish's
// results by this block before the fence. The host checks the stamp before it
// reads any of them (check_stamp).
DEVI void small_snap(Small* sm, Small* snap, const Small* init, uint64_t seq) {
  constexpr uint32_t NW = sizeof(Small) / 8;
  const volatile uint64_t* s = (const volatile uint64_t*)sm;
  uint64_t* d = (uint64_t*)snap;
  for (uint32_t i = threadIdx.x; i < NW; i += blockDim.x) d[i] = s[i];
  __threadfence_system();  // (the snapshot's host writes complete before this kernel does)
  __syncthreads();  // (every word read and fenced before any is reset, and before the stamp)
  if (threadIdx.x == 0)
    __hip_atomic_store((uint64_t*)((uint8_t*)snap + OUT_HDR - 8), seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  if (!init) return;
  const uint64_t* in = (const uint64_t*)init;
  uint64_t* w = (uint64_t*)sm;
  for (uint32_t i = threadIdx.x; i < NW; i += blockDim.x) w[i] = in[i];
}

// End of a call, after the finalize: the call state is snapshot ahead of the
// outputs (one D2H copy brings both back) and reset for the next call; the
// words of the grid points are cleared, which leaves the bitmap zero.
// Small unsharded calls also compute the lazy error index here (block 0,
// before the snapshot; bad.n_kept = 0: k_bad_index ran).
// (the optimistic aligned-group finish: `done` null, or the call is over only
// when *done; otherwise the state is snapshot for the host and left as it is)
__global__ void __launch_bounds__(256) k_call_end(Small* sm, Small* snap, const Small* init, uint32_t* bitmap,
                                                  const uint32_t* grid, uint64_t T, int64_t lo, BadArgs bad,
                                                  uint64_t seq, const uint32_t* done = nullptr) {
  __shared__ unsigned long long s_min[4];
  if (done) {
    __shared__ uint64_t s_t;
    __shared__ uint32_t s_over;
    if (threadIdx.x == 0) {
      s_over = *(volatile const uint32_t*)done;
      s_t = sm->T;
    }
    __syncthreads();
    if (!s_over) {
      if (blockIdx.x == 0) small_snap(sm, snap, nullptr, seq);
      return;
    }
    T = s_t;
  }
  if (blockIdx.x == 0) {
    if (bad.n_kept) {
      unsigned long long m = ~0ull;
      for (uint32_t k = threadIdx.x; k < bad.n_kept; k += 256) m = min(m, (unsigned long long)bad_key(bad, k));
      for (int o = 1; o < WAVE; o <<= 1) m = min(m, (unsigned long long)shfl_xor_u64(m, o));
      if (lane_id() == 0) s_min[threadIdx.x / WAVE] = m;
      __syncthreads();
      if (threadIdx.x == 0) {
        m = min(min(s_min[0], s_min[1]), min(s_min[2], s_min[3]));
        if (m != ~0ull) atomicMin(&sm->bad_at, m);
        __threadfence();
      }
    }
    __syncthreads();  // (bad_at final)
    small_snap(sm, snap, init, seq);
    __syncthreads();  // (the ranks above read the bitmap cleared below)
  }
  if (bitmap)
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < T; i += (uint64_t)gridDim.x * 256)
      bitmap[(uint64_t)((int64_t)grid[i] - lo) >> 5] = 0u;
}

// p[0, n) = v
__global__ void k_fill_u64(unsigned long long* p, uint32_t n, unsigned long long v) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) p[i] = v;
}

// TSDBHIP_CHECK_CLEAN: counts non-zero words of a buffer (debug of the
// zero-on-entry invariants)
__global__ void k_count_nonzero(const uint32_t* p, uint64_t n, unsigned long long* out) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256)
    if (p[i]) atomicAdd(out, 1ull);
}
