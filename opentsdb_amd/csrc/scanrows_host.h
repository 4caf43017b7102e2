// scanrows_host.h — the argument checks, the query as the kernels read it and
// the per-row test of tsdbhip_scan_rows. Plain C++ without a device, so that
// they also build into a stand-alone program under the host sanitizers
// (tests/san_scanrows.cc). Shared with the kernels (k_scanrows.hip): the key
// check is findspans_host.h's fs_check_key, the row test sr_match; a host
// table is checked by sr_first_error before anything is staged, a device table
// by k_sr_match.
#pragma once
#include <algorithm>
#include <vector>

#include "findspans_host.h"

namespace tsdb {

constexpr uint32_t SR_FIXED = 0, SR_ANY = 1, SR_LIST = 2;
constexpr uint32_t SR_LIST_LINEAR = 16;  // a list of up to this many ids: a wave-uniform loop; longer: a binary search

// The query as k_sr_match takes it (a kernel argument: every field is
// wave-uniform). Names, values and ids are packed big-endian into a word, so
// that the unsigned order of the words is the byte order of the ids.
struct SrQuery {
  uint32_t t_start, t_stop;  // scan_start <= base_time < scan_stop, unsigned
  uint32_t filter;           // n_tags + n_group_bys > 0
  uint32_t n_items;          // tags and group-bys merged by name; > TSDBHIP_MAX_TAGS: no row matches
  uint64_t name[TSDBHIP_MAX_TAGS];
  uint64_t value[TSDBHIP_MAX_TAGS];     // SR_FIXED
  uint32_t kind[TSDBHIP_MAX_TAGS];
  uint32_t list_off[TSDBHIP_MAX_TAGS];  // SR_LIST: ids[list_off, list_off + list_n), ascending
  uint32_t list_n[TSDBHIP_MAX_TAGS];
  const uint64_t* ids;
};

template <class P>
FS_HD uint64_t sr_pack(P p, uint32_t at, uint32_t w) {
  uint64_t v = 0;
  for (uint32_t i = 0; i < w; i++) v = (v << 8) | (uint8_t)p[at + i];
  return v;
}

FS_HD bool sr_in_list(const uint64_t* ids, uint32_t n, uint64_t v) {
  if (n <= SR_LIST_LINEAR) {  // (uniform addresses)
    bool hit = false;
    for (uint32_t j = 0; j < n; j++) hit |= ids[j] == v;
    return hit;
  }
  uint32_t lo = 0, hi = n;  // the first id >= v
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (ids[mid] < v) lo = mid + 1;
    else hi = mid;
  }
  return lo < n && ids[lo] == v;
}

// The scanner's test of a key of a valid shape, k[0, len): inside the start /
// stop keys, and the regexp. The items are taken in order (a uniform loop); a
// lane looks for the earliest pair after the previous item's that has the
// item's name and an accepted value: the walk with an item cursor.
template <class P>
FS_HD bool sr_match(P k, uint32_t len, const FsRows& a, const SrQuery& q) {
  for (uint32_t i = 0; i < a.mw; i++)
    if ((uint8_t)k[i] != a.metric[i]) return false;
  const uint32_t t = (uint32_t)sr_pack(k, a.mw, 4);
  if (!(q.t_start <= t && t < q.t_stop)) return false;
  if (!q.filter) return true;
  if (q.n_items > TSDBHIP_MAX_TAGS) return false;
  const uint32_t pair = a.nw + a.vw;
  uint32_t pos = a.mw + 4;
  bool alive = true;
  for (uint32_t i = 0; i < q.n_items; i++) {
    const uint64_t name = q.name[i], value = q.value[i];
    const uint32_t kind = q.kind[i], ln = q.list_n[i];
    const uint64_t* ids = q.ids + q.list_off[i];
    bool found = false;
    while (alive && !found && pos < len) {
      const uint32_t p = pos;
      pos += pair;
      if (sr_pack(k, p, a.nw) != name) continue;
      if (kind == SR_ANY) found = true;
      else {
        const uint64_t v = sr_pack(k, p + a.nw, a.vw);
        found = kind == SR_FIXED ? v == value : sr_in_list(ids, ln, v);
      }
    }
    alive = alive && found;
  }
  return alive;
}

// A host table's error word (what k_sr_match leaves for a device one): the
// key_off and key shape classes of findspans_host.h, every row of the table.
inline uint64_t sr_first_error(const FsRows& a) {
  if (a.n && a.key_off[a.n] != a.key_nbytes) return FS_E_END;
  for (uint32_t r = 0; r < a.n; r++)
    if (const uint32_t cls = fs_check_key(a, a.key_off[r], a.key_off[r + 1])) return ((uint64_t)r << 8) | cls;
  return FS_NO_ERROR;
}

inline int sr_memcmp(const uint8_t* x, const uint8_t* y, uint32_t w) { return w ? memcmp(x, y, w) : 0; }

// The table, the query and the outputs. Null: fine; else what is wrong, in
// this order: the table, the counts, the order of the names, the arrays.
inline const char* sr_check_args(const tsdbhip_scan_desc* d, const tsdbhip_scan_query* q, const tsdbhip_scan_sel* out) {
  if (d->metric_width < 1 || d->metric_width > 8 || d->name_width < 1 || d->name_width > 8 ||
      d->value_width < 1 || d->value_width > 8)
    return "a width outside 1..8";
  const int cells = (d->row_qual_off != nullptr) + (d->row_qual_len != nullptr) + (d->row_val_off != nullptr) +
                    (d->row_val_len != nullptr);
  if (cells != 0 && cells != 4) return "some but not all of the four cell arrays";
  if (q->n_tags > TSDBHIP_MAX_TAGS) return "more than TSDBHIP_MAX_TAGS tags";
  if (q->n_group_bys > TSDBHIP_MAX_TAGS) return "more than TSDBHIP_MAX_TAGS group_bys";
  if (q->n_tags && !q->tags) return "tags is null";
  if (q->n_group_bys && !q->group_bys) return "group_bys is null";
  const uint32_t nw = d->name_width, pair = nw + d->value_width;
  for (uint32_t i = 1; i < q->n_tags; i++)
    if (sr_memcmp(q->tags + (i - 1) * pair, q->tags + i * pair, nw) >= 0) return "tags not strictly ascending by name";
  for (uint32_t i = 1; i < q->n_group_bys; i++)
    if (sr_memcmp(q->group_bys + (i - 1) * nw, q->group_bys + i * nw, nw) >= 0)
      return "group_bys not strictly ascending";
  for (uint32_t i = 0; i < q->n_tags; i++)
    for (uint32_t j = 0; j < q->n_group_bys; j++)
      if (sr_memcmp(q->tags + i * pair, q->group_bys + j * nw, nw) == 0) return "a name is both in tags and in group_bys";
  if (q->group_by_nvalues && !q->group_by_values)
    for (uint32_t j = 0; j < q->n_group_bys; j++)
      if (q->group_by_nvalues[j]) return "group_by_values is null";
  if (d->n_rows == 0) return nullptr;
  if (!d->metric) return "metric is null";
  if (!d->key_off || (d->key_nbytes && !d->key_bytes)) return "key_off / key_bytes is null";
  if (!out->row_index || !out->key_off || (out->key_capacity && !out->key_bytes)) return "null output array";
  if (d->row_status && !out->row_status) return "null output row_status";
  if (cells && (!out->row_qual_off || !out->row_qual_len || !out->row_val_off || !out->row_val_len))
    return "null output cell array";
  return nullptr;
}

// The query as the kernels read it (sr_check_args passed). ids receives every
// list's packed ids, each list ascending; q->ids is left for the caller to
// point at them (host: ids.data(); device: their copy).
inline void sr_build_query(const tsdbhip_scan_desc* d, const tsdbhip_scan_query* in, SrQuery* q,
                           std::vector<uint64_t>* ids) {
  memset(q, 0, sizeof *q);
  ids->clear();
  // TsdbQuery.java:410-411, 424 in 64 bits, then (int) (:378-382)
  const int64_t ts = (int64_t)in->start_time - 2 * 3600 - (int64_t)in->sample_interval;
  q->t_start = (uint32_t)(ts > 0 ? ts : 0);
  q->t_stop = (in->flags & TSDBHIP_SCAN_END_UNSET)
                  ? 0xFFFFFFFFu
                  : (uint32_t)((uint64_t)in->end_time + 3600 + 1 + (uint64_t)in->sample_interval);
  const uint32_t nw = d->name_width, vw = d->value_width, pair = nw + vw;
  q->n_items = in->n_tags + in->n_group_bys;
  q->filter = q->n_items > 0;
  if (q->n_items > TSDBHIP_MAX_TAGS) return;  // matches no row
  uint32_t t = 0, g = 0, voff = 0;
  for (uint32_t i = 0; i < q->n_items; i++) {  // the merge of :459-488
    const bool tag_next = t < in->n_tags && (g >= in->n_group_bys ||
                                             sr_memcmp(in->tags + t * pair, in->group_bys + g * nw, nw) < 0);
    if (tag_next) {
      q->name[i] = sr_pack(in->tags, t * pair, nw);
      q->value[i] = sr_pack(in->tags, t * pair + nw, vw);
      q->kind[i] = SR_FIXED;
      t++;
    } else {
      q->name[i] = sr_pack(in->group_bys, g * nw, nw);
      const uint32_t nv = in->group_by_nvalues ? in->group_by_nvalues[g] : 0;
      q->kind[i] = nv ? SR_LIST : SR_ANY;
      q->list_off[i] = (uint32_t)ids->size();
      q->list_n[i] = nv;
      for (uint32_t j = 0; j < nv; j++) ids->push_back(sr_pack(in->group_by_values, (voff + j) * vw, vw));
      std::sort(ids->begin() + q->list_off[i], ids->end());
      voff += nv;
      g++;
    }
  }
}

}  // namespace tsdb
