/* abi_check_findspans.c — include/tsdbhip.h as a plain C11 consumer sees the
 * two structs of tsdbhip_find_spans: sizeof / offsetof of every field, as
 * JSON, compared with the ctypes mirror (tests/test_find_spans.py). Needs no
 * library and no GPU. */
#include <stddef.h>
#include <stdio.h>

#include "tsdbhip.h"

#ifndef TSDBHIP_HAS_FIND_SPANS
#error "tsdbhip.h does not announce tsdbhip_find_spans"
#endif

#define F(st, f) printf("%s\"%s\": [%zu, %zu]", first++ ? ", " : "", #f, offsetof(st, f), sizeof(((st*)0)->f))
#define BEGIN(st) do { int first = 0; printf("%s\"%s\": {\"size\": %zu, \"fields\": {", nst++ ? ", " : "", #st, sizeof(st))
#define END() printf("}}"); } while (0)

int main(void) {
  int nst = 0;
  printf("{\"abi_version\": %d, \"has_find_spans\": %d, \"hot_find_spans\": %d, \"structs\": {", TSDBHIP_ABI_VERSION,
         TSDBHIP_HAS_FIND_SPANS, TSDBHIP_HOT_FIND_SPANS);
  BEGIN(tsdbhip_scan_desc);
  F(tsdbhip_scan_desc, flags);
  F(tsdbhip_scan_desc, n_rows);
  F(tsdbhip_scan_desc, metric_width);
  F(tsdbhip_scan_desc, name_width);
  F(tsdbhip_scan_desc, value_width);
  F(tsdbhip_scan_desc, reserved0);
  F(tsdbhip_scan_desc, reserved1);
  F(tsdbhip_scan_desc, metric);
  F(tsdbhip_scan_desc, key_off);
  F(tsdbhip_scan_desc, key_bytes);
  F(tsdbhip_scan_desc, key_nbytes);
  F(tsdbhip_scan_desc, row_status);
  F(tsdbhip_scan_desc, row_qual_off);
  F(tsdbhip_scan_desc, row_qual_len);
  F(tsdbhip_scan_desc, row_val_off);
  F(tsdbhip_scan_desc, row_val_len);
  END();
  BEGIN(tsdbhip_spans_out);
  F(tsdbhip_spans_out, span_capacity);
  F(tsdbhip_spans_out, n_spans);
  F(tsdbhip_spans_out, n_rows);
  F(tsdbhip_spans_out, n_skipped);
  F(tsdbhip_spans_out, key_capacity);
  F(tsdbhip_spans_out, key_used);
  F(tsdbhip_spans_out, row_order);
  F(tsdbhip_spans_out, span_row_start);
  F(tsdbhip_spans_out, row_base);
  F(tsdbhip_spans_out, row_ncells);
  F(tsdbhip_spans_out, row_qual_off);
  F(tsdbhip_spans_out, row_val_off);
  F(tsdbhip_spans_out, row_val_len);
  F(tsdbhip_spans_out, key_off);
  F(tsdbhip_spans_out, key_bytes);
  END();
  printf("}}\n");
  return 0;
}
