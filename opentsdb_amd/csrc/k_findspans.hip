// k_findspans.hip — kernels of tsdbhip_find_spans: the TreeMap<byte[], Span>
// under SpanCmp that TsdbQuery.findSpans fills row by row (TsdbQuery.java:
// 240-285, 594-621), for a batch of scanned rows in delivery order.
//
//   k_fs_keys     a lane per row, grid-stride: fs_check_row (first offending row: one
//                 atomicMin word), the identity index, and the AND / OR of every
//                 sort-key digit over all rows (a digit position whose AND ==
//                 OR is equal in every row and costs no pass)
//   k_fs_digits   a lane per row: its live digits into a dense
//                 [n_rows x n_live] table, most significant first (the padded
//                 key of up to 129 B a row is never materialised)
//   (sort)        k_groupby's stable LSD passes k_gb_count / scan /
//                 k_gb_scatter over the table's columns, unchanged
//   k_fs_heads    a lane per sorted position: head flag (dense row differs from
//                 its predecessor's: the other digits are equal in all rows) and
//                 added flag, packed into one scan word, and the head's key length
//   k_fs_emit     a lane per sorted position: an added row's output entries at
//                 its scanned position; a head's span_row_start, key_off and key
#pragma once
#include "dev_common.h"
#include "findspans_host.h"

namespace tsdb {

constexpr uint32_t FS_MAX_DIGITS = TSDBHIP_MAX_TAGS * 16 + 1;  // 129: the padded tag part and the tag count
constexpr uint32_t FS_KEY_WORDS = (FS_MAX_DIGITS + 3) / 4;      // 33 AND / OR words of 4 digits
constexpr uint32_t FS_KEYS_BLOCKS = 2048;                       // k_fs_keys' grid at most (8 blocks a CU)
constexpr uint32_t FS_WORDS = 36;                               // ... as the call's small state holds them

struct FsKeysArgs {
  FsRows in;
  uint32_t P;      // TSDBHIP_MAX_TAGS * (nw + vw): digits 0..P-1 the padded tag part, digit P the tag count
  uint32_t* idx0;  // [n] the identity
  unsigned long long* err;
  uint32_t* andw;  // [FS_WORDS]
  uint32_t* orw;   // [FS_WORDS]
};

// Grid-stride: a lane keeps the AND / OR words of its rows in registers (the
// unrolled words have static indices) and the wave reduces them once at its
// end, so the two shared words a digit has see a few thousand waves, not one
// per 64 rows (at 4M rows of 31-byte keys: 0.33 ms a launch, 0.46 ms with a
// wave reduction per 64 rows; what is left is the byte loads of the keys).
__global__ void __launch_bounds__(256) k_fs_keys(FsKeysArgs a) {
  const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
  if (tid == 0 && a.in.key_off[a.in.n] != a.in.key_nbytes) atomicMin(a.err, (unsigned long long)FS_E_END);
  const uint32_t hdr = a.in.mw + 4;
  const uint32_t nwords = (a.P + 4) / 4;  // digits 0..P (uniform)
  uint32_t va[FS_KEY_WORDS], vo[FS_KEY_WORDS];
#pragma unroll
  for (uint32_t w = 0; w < FS_KEY_WORDS; w++) va[w] = ~0u, vo[w] = 0u;
  for (uint64_t r64 = tid; r64 < a.in.n; r64 += stride) {
    const uint32_t r = (uint32_t)r64;
    FsRow row;
    const uint32_t cls = fs_check_row(a.in, r, &row);
    a.idx0[r] = r;
    if (cls) {
      atomicMin(a.err, ((unsigned long long)r << 8) | cls);
      continue;
    }
    const uint8_t* tags = a.in.key + row.o0 + hdr;
    const uint32_t taglen = (uint32_t)(row.len - hdr);
#pragma unroll
    for (uint32_t w = 0; w < FS_KEY_WORDS; w++) {
      if (w < nwords) {
        uint32_t v = 0;
#pragma unroll
        for (uint32_t b = 0; b < 4; b++) v |= fs_digit(tags, taglen, row.nt, a.P, w * 4 + b) << (8 * b);
        va[w] &= v;
        vo[w] |= v;
      }
    }
  }
#pragma unroll
  for (uint32_t w = 0; w < FS_KEY_WORDS; w++) {
    if (w < nwords) {
      uint32_t xa = va[w], xo = vo[w];
#pragma unroll
      for (int m = 1; m < WAVE; m <<= 1) {
        xa &= (uint32_t)__shfl_xor((int)xa, m);
        xo |= (uint32_t)__shfl_xor((int)xo, m);
      }
      if (lane_id() == 0) {  // (an atomic only where it changes the word)
        const uint32_t ca = __hip_atomic_load(a.andw + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t co = __hip_atomic_load(a.orw + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((ca & xa) != ca) atomicAnd(a.andw + w, xa);
        if ((co | xo) != co) atomicOr(a.orw + w, xo);
      }
    }
  }
}

struct FsDigitArgs {
  uint32_t n, mw, nw, vw, P, n_live;
  const uint64_t* key_off;
  const uint8_t* key;
  uint8_t live[FS_MAX_DIGITS + 3];  // the live digit positions, ascending
  uint8_t* dense;                   // [n * n_live]
};

// (the keys passed k_fs_keys: every length is a valid shape)
__global__ void __launch_bounds__(256) k_fs_digits(FsDigitArgs a) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= a.n) return;
  const uint32_t hdr = a.mw + 4;
  const uint64_t o0 = a.key_off[r];
  const uint32_t taglen = (uint32_t)(a.key_off[r + 1] - o0) - hdr, nt = taglen / (a.nw + a.vw);
  const uint8_t* tags = a.key + o0 + hdr;
  uint8_t* out = a.dense + (uint64_t)r * a.n_live;
  for (uint32_t j = 0; j < a.n_live; j++) out[j] = (uint8_t)fs_digit(tags, taglen, nt, a.P, a.live[j]);
}

struct FsSpanArgs {
  uint32_t n, n_live, mw;
  bool cells;
  const uint32_t* ord;  // [n] row at sorted position i
  const uint8_t* dense;
  const uint64_t* key_off;
  const uint8_t* key;
  const uint8_t* status;  // null: every row is added
  const uint64_t* in_qoff;
  const uint32_t* in_qlen;
  const uint64_t* in_voff;
  const uint32_t* in_vlen;
  uint64_t* flags;          // [n] (head << 32) | added
  const uint64_t* fscan;    // its exclusive scan: (spans before i) << 32 | rows added before i
  uint64_t* klen;           // [n] the key length at a head, else 0
  const uint64_t* kscan;    // its exclusive scan
  const uint64_t* totals;   // [0] the flags' total, [1] the key bytes
  uint32_t* row_order;
  uint64_t* span_row_start;
  uint32_t* row_base;
  uint32_t* row_ncells;
  uint64_t* row_qual_off;
  uint64_t* row_val_off;
  uint32_t* row_val_len;
  uint64_t* out_key_off;
  uint8_t* out_key;
};

__global__ void __launch_bounds__(256) k_fs_heads(FsSpanArgs a) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  const uint32_t r = a.ord[i];
  bool head = i == 0;
  if (!head) {
    const uint8_t* x = a.dense + (uint64_t)r * a.n_live;
    const uint8_t* y = a.dense + (uint64_t)a.ord[i - 1] * a.n_live;
    for (uint32_t b = 0; b < a.n_live && !head; b++) head = x[b] != y[b];
  }
  const bool added = !a.status || a.status[r] != TSDBHIP_ROW_NONE;
  a.flags[i] = ((uint64_t)(head ? 1u : 0u) << 32) | (added ? 1u : 0u);
  a.klen[i] = head ? a.key_off[r + 1] - a.key_off[r] : 0ull;
}

// (launched after the host has checked the totals against the capacities:
// span < n_spans <= span_capacity, a key ends at or before key_used <=
// key_capacity, an output row < rows added <= n)
__global__ void __launch_bounds__(256) k_fs_emit(FsSpanArgs a) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) {
    const uint64_t tot = a.totals[0];
    a.span_row_start[tot >> 32] = tot & 0xFFFFFFFFull;
    a.out_key_off[tot >> 32] = a.totals[1];
  }
  if (i >= a.n) return;
  const uint32_t r = a.ord[i];
  const uint64_t f = a.flags[i], fs = a.fscan[i];
  const uint64_t o0 = a.key_off[r];
  const uint32_t p = (uint32_t)fs;
  if (f >> 32) {  // a head: the first delivered row of its span
    const uint32_t s = (uint32_t)(fs >> 32);
    const uint64_t ko = a.kscan[i], len = a.klen[i];
    a.span_row_start[s] = p;
    a.out_key_off[s] = ko;
    for (uint64_t b = 0; b < len; b++) a.out_key[ko + b] = a.key[o0 + b];
  }
  if (f & 1u) {
    a.row_order[p] = r;
    const uint8_t* t = a.key + o0 + a.mw;
    a.row_base[p] = ((uint32_t)t[0] << 24) | ((uint32_t)t[1] << 16) | ((uint32_t)t[2] << 8) | t[3];
    if (a.cells) {
      a.row_ncells[p] = a.in_qlen[r] / 2;
      a.row_qual_off[p] = a.in_qoff[r];
      a.row_val_off[p] = a.in_voff[r];
      a.row_val_len[p] = a.in_vlen[r];
    }
  }
}

}  // namespace tsdb
