// descpack_host.h — the host-side argument checks and the placement rule of
// tsdbhip_desc_pack. Plain C++ without a device, like groupby_host.h.
#pragma once
#include <stdint.h>

#include "../../include/tsdbhip.h"
#include "groupby_host.h"

namespace tsdb {

// Null: fine; else what is wrong with the arguments (the order's entries are
// gather_check_order's business).
inline const char* pack_check_args(const tsdbhip_sg_desc* in, const uint32_t* order, uint32_t n,
                                   const tsdbhip_sg_desc* out) {
  if (in == out) return "in and out are the same descriptor";
  if (!(in->flags & TSDBHIP_DESC_DEVICE) || (in->flags & TSDBHIP_SHARDED))
    return "the input must be a device-resident, unsharded descriptor";
  if (!order && n != in->n_spans) return "a null order takes every span: n must equal the input's n_spans";
  if (n && (!in->span_row_start || (in->n_rows && (!in->row_base || !in->row_ncells || !in->row_qual_off ||
                                                   !in->row_val_off || !in->row_val_len))))
    return "a null array in the input";
  return nullptr;
}

// packing.pack_spans' buffer length for `used` bytes of aligned extents
inline uint64_t pack_nbytes(uint64_t used) { return ((used ? used : 1) + 15) & ~15ull; }

}  // namespace tsdb
