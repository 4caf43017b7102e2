/* abi_check_groupby.c — include/tsdbhip.h as a plain C11 consumer sees the
 * two structs of tsdbhip_groupby_plan: sizeof / offsetof of every field, as
 * JSON, compared with the ctypes mirror (tests/test_groupby_plan.py). Needs
 * no library and no GPU. */
#include <stddef.h>
#include <stdio.h>

#include "tsdbhip.h"

#define F(st, f) printf("%s\"%s\": [%zu, %zu]", first++ ? ", " : "", #f, offsetof(st, f), sizeof(((st*)0)->f))
#define BEGIN(st) do { int first = 0; printf("%s\"%s\": {\"size\": %zu, \"fields\": {", nst++ ? ", " : "", #st, sizeof(st))
#define END() printf("}}"); } while (0)

int main(void) {
  int nst = 0;
  printf("{\"abi_version\": %d, \"max_tags\": %d, \"hot_groupby\": %d, \"structs\": {", TSDBHIP_ABI_VERSION,
         TSDBHIP_MAX_TAGS, TSDBHIP_HOT_GROUPBY);
  BEGIN(tsdbhip_keys_desc);
  F(tsdbhip_keys_desc, flags);
  F(tsdbhip_keys_desc, n_spans);
  F(tsdbhip_keys_desc, metric_width);
  F(tsdbhip_keys_desc, name_width);
  F(tsdbhip_keys_desc, value_width);
  F(tsdbhip_keys_desc, n_group_bys);
  F(tsdbhip_keys_desc, reserved0);
  F(tsdbhip_keys_desc, key_off);
  F(tsdbhip_keys_desc, key_bytes);
  F(tsdbhip_keys_desc, key_nbytes);
  F(tsdbhip_keys_desc, span_kept);
  F(tsdbhip_keys_desc, group_bys);
  END();
  BEGIN(tsdbhip_groups_out);
  F(tsdbhip_groups_out, group_capacity);
  F(tsdbhip_groups_out, n_groups);
  F(tsdbhip_groups_out, n_grouped);
  F(tsdbhip_groups_out, n_dropped);
  F(tsdbhip_groups_out, order);
  F(tsdbhip_groups_out, group_span_start);
  F(tsdbhip_groups_out, group_key);
  F(tsdbhip_groups_out, group_ntags);
  F(tsdbhip_groups_out, group_tags);
  F(tsdbhip_groups_out, group_common);
  END();
  printf("}}\n");
  return 0;
}
