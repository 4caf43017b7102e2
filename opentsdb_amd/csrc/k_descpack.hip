// k_descpack.hip — kernels of tsdbhip_desc_pack: the rows of gathered spans
// copied into new buffers in packing.pack_spans' layout (qualifiers at 0 mod
// 8, values at 0 mod 16, gaps and tail zero), from source rows at any offset.
//
//   (gather)      k_gather_count, dscan_u64, k_gather_rows (k_groupby.hip): the
//                 spans' rows in the given order, offsets still the source's
//   k_pack_sizes  a lane per gathered row: the row inside the source buffers
//                 (first offending row: one atomicMin word), the source offsets
//                 saved, the row's aligned extents and its piece count
//   (scans)       dscan_u64 over the qualifier extents, the value extents (the
//                 new offsets) and the piece counts
//   k_pack_copy   a wave per run of PK_RUN consecutive pieces. A piece is up to
//                 four wave instructions of one row's aligned extent in one
//                 buffer, each 64 lanes x one unit contiguous: 16-B units for
//                 values (1 KB an instruction, 4 KB a piece), 8-B units for
//                 qualifiers (their extents are multiples of 8: 512 B, 2 KB).
//                 The destination is unit-aligned and stored whole, the bytes
//                 between a row's end and its extent as zeros by the same
//                 stores: the extents tile the buffers, nothing else clears them.
//                 A row whose two extents are at most 64 B has no pieces: the
//                 kernel's last blocks copy such rows a lane each.
//                 The source is read at the row's own residue, <false> by one
//                 unit-wide load at that address, <true> by dword-aligned loads
//                 and v_alignbyte_b32 by the residue (wave-uniform per row).
#pragma once
#include "dev_common.h"

namespace tsdb {

constexpr uint32_t PK_THREADS = 256, PK_WAVES = PK_THREADS / WAVE;
constexpr uint32_t PK_INSTR = 4;  // wave instructions a piece
constexpr uint32_t PK_QUNIT = 8, PK_VUNIT = 16;
constexpr uint32_t PK_QPIECE = PK_INSTR * WAVE * PK_QUNIT;  // 2 KB of qualifier extent
constexpr uint32_t PK_VPIECE = PK_INSTR * WAVE * PK_VUNIT;  // 4 KB of value extent
constexpr uint32_t PK_RUN = 4;  // consecutive pieces a wave copies after one search
constexpr uint32_t PK_SMALL = 64;  // a row whose extents are both at most this long is copied by one lane
#ifndef TSDBHIP_PACK_NT
#define TSDBHIP_PACK_NT 0  // 1: the source loads non-temporal (A/B builds; measured no faster: DESIGN.md)
#endif
constexpr bool PK_NT = TSDBHIP_PACK_NT != 0;
constexpr unsigned long long PK_NO_ERROR = ~0ull;

struct PackArgs {
  uint64_t n_rows;    // gathered rows
  const uint32_t* ncells;  // [n_rows] the gathered metadata
  const uint32_t* vlen;
  const uint64_t* g_qoff;  // [n_rows] source offsets as gathered (k_pack_sizes reads them ...
  const uint64_t* g_voff;
  uint64_t* src_qoff;      // ... and saves them here before the scans overwrite them)
  uint64_t* src_voff;
  uint64_t in_qn, in_vn;   // the source's qual_nbytes / val_nbytes
  unsigned long long* err;  // the first gathered row outside the source buffers
  uint64_t* row_bytes;      // += the rows' own bytes (alg_bytes)
  uint64_t* qsz;            // [n_rows] align8(2 ncells)
  uint64_t* vsz;            // [n_rows] align16(vlen)
  uint64_t* pcs;            // [n_rows] pieces of the row: qualifiers first, then values (a small row: 0)
};

DEVI uint64_t pk_qpieces(uint64_t qsz) { return (qsz + PK_QPIECE - 1) / PK_QPIECE; }
DEVI uint64_t pk_vpieces(uint64_t vsz) { return (vsz + PK_VPIECE - 1) / PK_VPIECE; }
// a small row (both extents at most PK_SMALL bytes) has no pieces: a lane copies it whole
DEVI bool pk_small(uint64_t qsz, uint64_t vsz) { return qsz <= PK_SMALL && vsz <= PK_SMALL; }
DEVI uint64_t pk_pieces(uint64_t qsz, uint64_t vsz) { return pk_small(qsz, vsz) ? 0 : pk_qpieces(qsz) + pk_vpieces(vsz); }

__global__ void __launch_bounds__(256) k_pack_sizes(PackArgs a) {
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint64_t mine = 0;
  if (r < a.n_rows) {
    const uint64_t qlen = 2ull * a.ncells[r], vl = a.vlen[r], qo = a.g_qoff[r], vo = a.g_voff[r];
    if (qo > a.in_qn || qlen > a.in_qn - qo || vo > a.in_vn || vl > a.in_vn - vo) atomicMin(a.err, (unsigned long long)r);
    a.src_qoff[r] = qo;
    a.src_voff[r] = vo;
    const uint64_t qsz = (qlen + 7) & ~7ull, vsz = (vl + 15) & ~15ull;
    a.qsz[r] = qsz;
    a.vsz[r] = vsz;
    a.pcs[r] = pk_pieces(qsz, vsz);
    mine = qlen + vl;
  }
  for (int d = WAVE / 2; d > 0; d >>= 1) mine += __shfl_down(mine, d, WAVE);
  if (lane_id() == 0 && mine) atomicAdd((unsigned long long*)a.row_bytes, (unsigned long long)mine);
}

// the low `keep` bytes of a little-endian dword (keep <= 0: none, >= 4: all)
DEVI uint32_t pk_keep(uint32_t w, int64_t keep) {
  if (keep >= 4) return w;
  if (keep <= 0) return 0;
  return w & ((1u << (8 * (uint32_t)keep)) - 1u);
}

// U / 4 dwords from p, which is a multiple of `AL` bytes
template <uint32_t U, uint32_t AL>
DEVI void pk_load(const uint8_t* p, uint32_t* w) {
  typedef uint32_t vec_t __attribute__((ext_vector_type(U / 4), aligned(AL)));
  vec_t v;
  if (PK_NT) v = __builtin_nontemporal_load((const vec_t*)p);
  else v = *(const vec_t*)p;
  for (uint32_t j = 0; j < U / 4; j++) w[j] = v[j];
}

// A whole piece of row bytes from p to the unit-aligned q: every load first, then the stores (four loads in
// flight a lane), no lane idle, nothing to mask, no branch between the stores. SB: p's residue mod 4, the
// loads dword-aligned below p and shifted (0: p is aligned to AL and loaded as it is).
template <uint32_t U, uint32_t AL, bool SHIFTED>
DEVI void pk_whole(const uint8_t* p, uint8_t* q, uint32_t sb, uint32_t lane) {
  typedef uint32_t out_t __attribute__((ext_vector_type(U / 4)));
  uint32_t w[PK_INSTR][U / 4 + 1];
#pragma unroll
  for (uint32_t i = 0; i < PK_INSTR; i++) {
    const uint8_t* pi = p + (i * WAVE + lane) * U;
    if (SHIFTED) {
      pk_load<U, 4>(pi - sb, w[i]);
      pk_load<4, 4>(pi - sb + U, w[i] + U / 4);
    } else {
      pk_load<U, AL>(pi, w[i]);
    }
  }
#pragma unroll
  for (uint32_t i = 0; i < PK_INSTR; i++) {
    out_t v;
    for (uint32_t j = 0; j < U / 4; j++) v[j] = SHIFTED ? __builtin_amdgcn_alignbyte(w[i][j + 1], w[i][j], sb) : w[i][j];
    *(out_t*)(q + (i * WAVE + lane) * U) = v;
  }
}

// One unit of a row's extent: row bytes [b, min(b + U, len)) from src + so + b to the unit-aligned dst + b,
// the rest of the unit zeros. b < alignU(len), so at least one byte of the row is in this unit;
// src[0, in_n + 64) is readable.
template <uint32_t U, bool SHIFT>
DEVI void pk_unit(const uint8_t* src, uint64_t so, uint64_t len, uint8_t* dst, uint64_t b) {
  typedef uint32_t out_t __attribute__((ext_vector_type(U / 4)));
  const uint8_t* row = src + so;
  const uint32_t sb = (uint32_t)((uintptr_t)row & 3u);  // the row's residue: the same for every unit of it
  const int64_t valid = (int64_t)(len - b);
  uint32_t w[U / 4];
  if (!SHIFT || sb == 0) {
    // one load at the row's residue; it ends before row + len + U <= src + in_n + 16
    pk_load<U, SHIFT ? 4 : 1>(row + b, w);
  } else if (so + b < sb) {
    // the aligned dword would begin before the buffer's first byte: byte by byte, the row's own bytes
    for (uint32_t j = 0; j < U / 4; j++) w[j] = 0;
    const uint32_t nb = valid < (int64_t)U ? (uint32_t)valid : U;
    for (uint32_t k = 0; k < nb; k++) w[k / 4] |= (uint32_t)row[b + k] << (8 * (k % 4));
  } else {
    // dwords from row + b - sb; the last one ends before row + len + U + 4 <= src + in_n + 20
    const uint8_t* p = row + b - sb;
    uint32_t t[U / 4 + 1];
    pk_load<U, 4>(p, t);
    pk_load<4, 4>(p + U, t + U / 4);
    for (uint32_t j = 0; j < U / 4; j++) w[j] = __builtin_amdgcn_alignbyte(t[j + 1], t[j], sb);
  }
  out_t v;
  for (uint32_t j = 0; j < U / 4; j++) v[j] = pk_keep(w[j], valid - 4 * (int64_t)j);  // (no byte of the next source row)
  *(out_t*)(dst + b) = v;
}

// One piece: instructions [0, PK_INSTR) of 64 units each from `off` on, inside
// the row's extent [0, ext) at dst; the row's `len` bytes are at src + so.
template <uint32_t U, bool SHIFT>
DEVI void pk_piece(const uint8_t* src, uint64_t so, uint64_t len, uint8_t* dst, uint64_t ext, uint64_t off,
                   uint32_t lane) {
  const uint8_t* row = src + so;
  const uint32_t sb = (uint32_t)((uintptr_t)row & 3u);
  if (off + PK_INSTR * WAVE * U <= len && (!SHIFT || so + off >= sb)) {  // (wave-uniform)
    // (the last load ends before row + len + 4 <= src + in_n + 4)
    if (!SHIFT) pk_whole<U, 1, false>(row + off, dst + off, 0, lane);
    else if (sb == 0) pk_whole<U, 4, false>(row + off, dst + off, 0, lane);
    else pk_whole<U, 4, true>(row + off, dst + off, sb, lane);
    return;
  }
  // the row's last piece (and the one at the buffer's first bytes), an instruction at a time
#pragma unroll
  for (uint32_t i = 0; i < PK_INSTR; i++) {
    const uint64_t o = off + (uint64_t)i * WAVE * U;
    if (o >= ext) break;  // (wave-uniform: the whole instruction lies past the extent)
    const uint64_t b = o + (uint64_t)lane * U;
    if (b < ext) pk_unit<U, SHIFT>(src, so, len, dst, b);
  }
}

// The metadata arrays are parameters of their own, const and __restrict__: nothing the kernel stores can
// alias them, so a row's offsets and lengths (wave-uniform in the piece waves) come by scalar loads.
struct PackCopyArgs {
  uint64_t n_rows, n_pieces;
  uint32_t piece_blocks;  // blocks [0, piece_blocks) copy pieces, the others small rows
  const uint8_t* in_qual;
  const uint8_t* in_val;
  uint8_t* out_qual;
  uint8_t* out_val;
};

// Blocks [0, piece_blocks): a wave per run of PK_RUN pieces. The other blocks: a lane per row, the waves
// striding over every row of the table 64 at a time; a lane copies its row if it is a small one (both extents
// at most PK_SMALL bytes: up to 8 qualifier units and 4 value units) and leaves a row of pieces alone. Rows of
// a few cells would otherwise be a piece of one or two busy lanes each, found by a search of its own.
template <bool SHIFT>
__global__ void __launch_bounds__(PK_THREADS)
    k_pack_copy(PackCopyArgs a, const uint64_t* __restrict__ pstart, const uint32_t* __restrict__ ncells,
                const uint32_t* __restrict__ vlen, const uint64_t* __restrict__ src_qoff,
                const uint64_t* __restrict__ src_voff, const uint64_t* __restrict__ dst_qoff,
                const uint64_t* __restrict__ dst_voff) {
  const uint32_t lane = lane_id();
  if (blockIdx.x >= a.piece_blocks) {
    const uint64_t t0 = (uint64_t)(blockIdx.x - a.piece_blocks) * PK_THREADS + threadIdx.x;
    const uint64_t nt = (uint64_t)(gridDim.x - a.piece_blocks) * PK_THREADS;
    for (uint64_t r = t0; r < a.n_rows; r += nt) {
      const uint64_t qlen = 2ull * ncells[r], vl = vlen[r];
      const uint64_t qsz = (qlen + 7) & ~7ull, vsz = (vl + 15) & ~15ull;
      if (!pk_small(qsz, vsz)) continue;
      const uint64_t sq = src_qoff[r], sv = src_voff[r];
      uint8_t* dq = a.out_qual + dst_qoff[r];
      uint8_t* dv = a.out_val + dst_voff[r];
      for (uint64_t b = 0; b < qsz; b += PK_QUNIT) pk_unit<PK_QUNIT, SHIFT>(a.in_qual, sq, qlen, dq, b);
      for (uint64_t b = 0; b < vsz; b += PK_VUNIT) pk_unit<PK_VUNIT, SHIFT>(a.in_val, sv, vl, dv, b);
    }
    return;
  }
  const uint64_t gwave = (uint64_t)blockIdx.x * PK_WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
  const uint64_t nwaves = (uint64_t)a.piece_blocks * PK_WAVES;
  for (uint64_t p0 = gwave * PK_RUN; p0 < a.n_pieces; p0 += nwaves * PK_RUN) {
    // the row of piece p0: the last r with pstart[r] <= p0 (a row without pieces shares its successor's start
    // and comes before it, so that r holds p0)
    uint64_t lo = 0, hi = a.n_rows;
    while (hi - lo > 1) {
      const uint64_t mid = lo + (hi - lo) / 2;
      if (pstart[mid] <= p0) lo = mid;
      else hi = mid;
    }
    uint64_t r = lo, ps = pstart[r];
    const uint64_t p1 = p0 + PK_RUN < a.n_pieces ? p0 + PK_RUN : a.n_pieces;
    uint64_t qlen = 2ull * ncells[r], vl = vlen[r];
    for (uint64_t p = p0; p < p1; p++) {
      uint64_t qsz = (qlen + 7) & ~7ull, vsz = (vl + 15) & ~15ull;
      while (p - ps >= pk_pieces(qsz, vsz)) {  // (p < n_pieces: a later row holds it)
        ps += pk_pieces(qsz, vsz);
        r++;
        qlen = 2ull * ncells[r];
        vl = vlen[r];
        qsz = (qlen + 7) & ~7ull;
        vsz = (vl + 15) & ~15ull;
      }
      const uint64_t k = p - ps, nq = pk_qpieces(qsz);
      if (k < nq)
        pk_piece<PK_QUNIT, SHIFT>(a.in_qual, src_qoff[r], qlen, a.out_qual + dst_qoff[r], qsz, k * PK_QPIECE, lane);
      else
        pk_piece<PK_VUNIT, SHIFT>(a.in_val, src_voff[r], vl, a.out_val + dst_voff[r], vsz, (k - nq) * PK_VPIECE, lane);
    }
  }
}

}  // namespace tsdb
