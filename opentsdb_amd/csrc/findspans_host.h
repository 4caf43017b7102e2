// findspans_host.h — the argument and row checks of tsdbhip_find_spans. Plain
// C++ without a device, so that they also build into a stand-alone program
// under the host sanitizers (tests/san_findspans.cc). The per-row check and
// the sort-key digit are shared with the kernels (k_findspans.hip): a host
// descriptor is checked by fs_first_error before anything is staged, a device
// descriptor by k_fs_keys, both through fs_check_row.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/tsdbhip.h"

#if defined(__HIPCC__)
#define FS_HD __host__ __device__ inline
#else
#define FS_HD inline
#endif

namespace tsdb {

// error word: (row << 8) | class, min-reduced: the first offending row in
// delivery order, and on one row the argument errors, then the metric, then
// the compaction result. 0: key_off does not end at key_nbytes (before any row).
constexpr uint64_t FS_NO_ERROR = ~0ull;
constexpr uint64_t FS_E_END = 0;
constexpr uint32_t FS_E_OFF = 1;        // key_off decreasing / past key_nbytes
constexpr uint32_t FS_E_SHAPE = 2;      // key length
constexpr uint32_t FS_E_STATUS = 3;     // row_status above TSDBHIP_ROW_OOB
constexpr uint32_t FS_E_CELL = 4;       // an added row's odd row_qual_len / row_qual_off
constexpr uint32_t FS_E_METRIC = 5;     // key does not start with the metric
constexpr uint32_t FS_E_ROW_ERROR = 6;  // TSDBHIP_ROW_ERROR
constexpr uint32_t FS_E_ROW_OOB = 7;    // TSDBHIP_ROW_OOB

// the rows of a scan as the checks read them (host or device pointers)
struct FsRows {
  uint32_t n, mw, nw, vw;
  const uint64_t* key_off;
  const uint8_t* key;
  uint64_t key_nbytes;
  const uint8_t* status;  // null: every row is added
  const uint64_t* qoff;   // null: no cells
  const uint32_t* qlen;
  uint8_t metric[8];
};

struct FsRow {
  uint64_t o0, len;  // the key: key[o0, o0 + len)
  uint32_t nt;       // its tag pairs
  bool added;        // status != NONE
};

// A key at key[o0, o1): 0, or FS_E_OFF / FS_E_SHAPE (the part of the row
// check that tsdbhip_scan_rows shares, scanrows_host.h). Reads no key byte.
FS_HD uint32_t fs_check_key(const FsRows& a, uint64_t o0, uint64_t o1) {
  const uint32_t pair = a.nw + a.vw, hdr = a.mw + 4;
  if (!(o0 <= o1 && o1 <= a.key_nbytes)) return FS_E_OFF;
  const uint64_t len = o1 - o0;
  if (len < hdr || (len - hdr) % pair != 0 || (len - hdr) / pair > TSDBHIP_MAX_TAGS) return FS_E_SHAPE;
  return 0;
}

// Row r (r < a.n): 0 and *row filled in, or the class of what is wrong with
// it. No key byte is read before it is proven inside [0, key_nbytes).
FS_HD uint32_t fs_check_row(const FsRows& a, uint32_t r, FsRow* row) {
  const uint32_t pair = a.nw + a.vw, hdr = a.mw + 4;
  const uint64_t o0 = a.key_off[r], o1 = a.key_off[r + 1];
  if (const uint32_t cls = fs_check_key(a, o0, o1)) return cls;
  const uint64_t len = o1 - o0;
  const uint32_t st = a.status ? a.status[r] : (uint32_t)TSDBHIP_ROW_SINGLE;
  if (st > TSDBHIP_ROW_OOB) return FS_E_STATUS;
  const bool added = st != TSDBHIP_ROW_NONE && st != TSDBHIP_ROW_ERROR && st != TSDBHIP_ROW_OOB;
  if (added && a.qoff && ((a.qoff[r] & 1u) || (a.qlen[r] & 1u))) return FS_E_CELL;
  for (uint32_t i = 0; i < a.mw; i++)
    if (a.key[o0 + i] != a.metric[i]) return FS_E_METRIC;
  if (st == TSDBHIP_ROW_ERROR) return FS_E_ROW_ERROR;
  if (st == TSDBHIP_ROW_OOB) return FS_E_ROW_OOB;
  row->o0 = o0;
  row->len = len;
  row->nt = (uint32_t)((len - hdr) / pair);
  row->added = added;
  return 0;
}

// Digit d (0 most significant) of a row's sort key: its tag part zero-padded
// to P = TSDBHIP_MAX_TAGS * (name_width + value_width) bytes, then the tag
// count as digit P. This is SpanCmp after the metric: a key that is a prefix
// of another compares lower or equal on the padding, and the count breaks the
// tie in favour of the shorter key.
FS_HD uint32_t fs_digit(const uint8_t* tags, uint32_t taglen, uint32_t nt, uint32_t P, uint32_t d) {
  return d < taglen ? tags[d] : (d == P ? nt : 0u);
}

// Widths 1..8 and the arrays present. Null: fine; else what is wrong.
inline const char* fs_check_desc(const tsdbhip_scan_desc* d, const tsdbhip_spans_out* out) {
  if (d->metric_width < 1 || d->metric_width > 8 || d->name_width < 1 || d->name_width > 8 ||
      d->value_width < 1 || d->value_width > 8)
    return "a width outside 1..8";
  const int cells = (d->row_qual_off != nullptr) + (d->row_qual_len != nullptr) + (d->row_val_off != nullptr) +
                    (d->row_val_len != nullptr);
  if (cells != 0 && cells != 4) return "some but not all of the four cell arrays";
  if (d->n_rows == 0) return nullptr;
  if (!d->metric) return "metric is null";
  if (!d->key_off || (d->key_nbytes && !d->key_bytes)) return "key_off / key_bytes is null";
  if (!out->row_order || !out->span_row_start || !out->row_base || !out->key_off ||
      (out->key_capacity && !out->key_bytes))
    return "null output array";
  if (cells && (!out->row_ncells || !out->row_qual_off || !out->row_val_off || !out->row_val_len))
    return "null output cell array";
  return nullptr;
}

inline FsRows fs_rows_of(const tsdbhip_scan_desc* d) {
  FsRows a;
  memset(&a, 0, sizeof a);
  a.n = d->n_rows;
  a.mw = d->metric_width;
  a.nw = d->name_width;
  a.vw = d->value_width;
  a.key_off = d->key_off;
  a.key = d->key_bytes;
  a.key_nbytes = d->key_nbytes;
  a.status = d->row_status;
  a.qoff = d->row_qual_off;
  a.qlen = d->row_qual_len;
  if (d->metric) memcpy(a.metric, d->metric, d->metric_width <= 8 ? d->metric_width : 8);
  return a;
}

// A host descriptor's error word (what k_fs_keys leaves for a device one).
inline uint64_t fs_first_error(const FsRows& a) {
  if (a.n && a.key_off[a.n] != a.key_nbytes) return FS_E_END;
  FsRow row;
  for (uint32_t r = 0; r < a.n; r++)
    if (const uint32_t cls = fs_check_row(a, r, &row)) return ((uint64_t)r << 8) | cls;
  return FS_NO_ERROR;
}

// The return code and message of an error word.
inline int fs_error(uint64_t err, char* buf, size_t cap) {
  const unsigned long long row = err >> 8;
  switch ((uint32_t)(err & 0xFF)) {
    case FS_E_END: snprintf(buf, cap, "key_off does not end at key_nbytes"); return TSDBHIP_E_INVALID_ARG;
    case FS_E_OFF: snprintf(buf, cap, "key_off out of range at row %llu", row); return TSDBHIP_E_INVALID_ARG;
    case FS_E_SHAPE: snprintf(buf, cap, "bad row key length at row %llu", row); return TSDBHIP_E_INVALID_ARG;
    case FS_E_STATUS: snprintf(buf, cap, "unknown row_status at row %llu", row); return TSDBHIP_E_INVALID_ARG;
    case FS_E_CELL:
      snprintf(buf, cap, "odd row_qual_off / row_qual_len at row %llu", row);
      return TSDBHIP_E_INVALID_ARG;
    case FS_E_METRIC:
      snprintf(buf, cap, "row %llu does not start with the query's metric", row);
      return TSDBHIP_E_ILLEGAL_DATA;
    case FS_E_ROW_ERROR:
      snprintf(buf, cap, "row %llu: compaction reported illegal data (TSDBHIP_ROW_ERROR)", row);
      return TSDBHIP_E_ILLEGAL_DATA;
    default:
      snprintf(buf, cap, "row %llu: compaction ran out of bounds (TSDBHIP_ROW_OOB)", row);
      return TSDBHIP_E_OUT_OF_BOUNDS;
  }
}

}  // namespace tsdb
