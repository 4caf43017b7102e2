/* abi_check_scanrows.c — include/tsdbhip.h as a plain C11 consumer sees the
 * two structs of tsdbhip_scan_rows: sizeof / offsetof of every field, as
 * JSON, compared with the ctypes mirror (tests/test_scan_rows.py). Needs no
 * library and no GPU. */
#include <stddef.h>
#include <stdio.h>

#include "tsdbhip.h"

#ifndef TSDBHIP_HAS_SCAN_ROWS
#error "tsdbhip.h does not announce tsdbhip_scan_rows"
#endif

#define F(st, f) printf("%s\"%s\": [%zu, %zu]", first++ ? ", " : "", #f, offsetof(st, f), sizeof(((st*)0)->f))
#define BEGIN(st) do { int first = 0; printf("%s\"%s\": {\"size\": %zu, \"fields\": {", nst++ ? ", " : "", #st, sizeof(st))
#define END() printf("}}"); } while (0)

int main(void) {
  int nst = 0;
  printf("{\"abi_version\": %d, \"has_scan_rows\": %d, \"hot_scan_rows\": %d, \"scan_end_unset\": %u, "
         "\"max_tags\": %d, \"structs\": {",
         TSDBHIP_ABI_VERSION, TSDBHIP_HAS_SCAN_ROWS, TSDBHIP_HOT_SCAN_ROWS, TSDBHIP_SCAN_END_UNSET, TSDBHIP_MAX_TAGS);
  BEGIN(tsdbhip_scan_query);
  F(tsdbhip_scan_query, start_time);
  F(tsdbhip_scan_query, end_time);
  F(tsdbhip_scan_query, sample_interval);
  F(tsdbhip_scan_query, flags);
  F(tsdbhip_scan_query, n_tags);
  F(tsdbhip_scan_query, n_group_bys);
  F(tsdbhip_scan_query, tags);
  F(tsdbhip_scan_query, group_bys);
  F(tsdbhip_scan_query, group_by_nvalues);
  F(tsdbhip_scan_query, group_by_values);
  END();
  BEGIN(tsdbhip_scan_sel);
  F(tsdbhip_scan_sel, row_capacity);
  F(tsdbhip_scan_sel, n_selected);
  F(tsdbhip_scan_sel, key_capacity);
  F(tsdbhip_scan_sel, key_used);
  F(tsdbhip_scan_sel, row_index);
  F(tsdbhip_scan_sel, key_off);
  F(tsdbhip_scan_sel, key_bytes);
  F(tsdbhip_scan_sel, row_status);
  F(tsdbhip_scan_sel, row_qual_off);
  F(tsdbhip_scan_sel, row_qual_len);
  F(tsdbhip_scan_sel, row_val_off);
  F(tsdbhip_scan_sel, row_val_len);
  END();
  printf("}}\n");
  return 0;
}
