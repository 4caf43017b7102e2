// groupby_host.h — the host-side argument checks of tsdbhip_groupby_plan and
// tsdbhip_desc_gather. Plain C++ without a device, so that they also build
// into a stand-alone program under the host sanitizers (tests/san_groupby.cc).
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/tsdbhip.h"

namespace tsdb {

// Widths 1..8, at most TSDBHIP_MAX_TAGS GROUP BY tags, their names strictly
// ascending (unsigned bytes), the arrays present. Null: fine; else what is wrong.
inline const char* gb_check_desc(const tsdbhip_keys_desc* d) {
  if (d->metric_width < 1 || d->metric_width > 8 || d->name_width < 1 || d->name_width > 8 ||
      d->value_width < 1 || d->value_width > 8)
    return "a width outside 1..8";
  if (d->n_group_bys > TSDBHIP_MAX_TAGS) return "more than TSDBHIP_MAX_TAGS group_bys";
  if (d->n_group_bys && !d->group_bys) return "group_bys is null";
  for (uint32_t g = 1; g < d->n_group_bys; g++)
    if (memcmp(d->group_bys + (size_t)(g - 1) * d->name_width, d->group_bys + (size_t)g * d->name_width,
               d->name_width) >= 0)
      return "group_bys not strictly ascending";
  if (d->n_spans && (!d->key_off || (d->key_nbytes && !d->key_bytes))) return "key_off / key_bytes is null";
  return nullptr;
}

// A host descriptor's key_off: non-decreasing, inside key_bytes, ending at
// key_nbytes. -1: fine; else the first offending span (n_spans: the end).
inline int64_t gb_check_key_off(const uint64_t* key_off, uint32_t n_spans, uint64_t key_nbytes) {
  for (uint32_t s = 0; s < n_spans; s++)
    if (key_off[s] > key_off[s + 1] || key_off[s + 1] > key_nbytes) return s;
  if (n_spans && key_off[n_spans] != key_nbytes) return n_spans;
  return -1;
}

// tsdbhip_desc_gather's order: every entry a span of `in`. -1: fine; else the
// first offending position.
inline int64_t gather_check_order(const uint32_t* order, uint32_t n, uint32_t n_spans) {
  for (uint32_t i = 0; i < n; i++)
    if (order[i] >= n_spans) return i;
  return -1;
}

}  // namespace tsdb
