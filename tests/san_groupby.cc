// san_groupby.cc — the host-side argument checks of tsdbhip_groupby_plan and
// tsdbhip_desc_gather (opentsdb_amd/csrc/groupby_host.h) as a stand-alone
// program, built with -fsanitize=address,undefined by
// tests/test_groupby_plan.py: key_off bounds, group_bys order, order range.
// Every array is heap-allocated at its exact size, so a read past an end is a
// sanitizer report. No device, no library.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../opentsdb_amd/csrc/groupby_host.h"

using namespace tsdb;

#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
      return 1;                                                   \
    }                                                             \
  } while (0)

static tsdbhip_keys_desc desc(const std::vector<uint8_t>& gb, uint8_t ngb, uint8_t mw, uint8_t nw, uint8_t vw,
                              const std::vector<uint64_t>& off, const std::vector<uint8_t>& bytes) {
  tsdbhip_keys_desc d;
  memset(&d, 0, sizeof d);
  d.n_spans = off.empty() ? 0 : (uint32_t)off.size() - 1;
  d.metric_width = mw;
  d.name_width = nw;
  d.value_width = vw;
  d.n_group_bys = ngb;
  d.key_off = off.data();
  d.key_bytes = bytes.data();
  d.key_nbytes = bytes.size();
  d.group_bys = gb.empty() ? nullptr : gb.data();
  return d;
}

int main() {
  const std::vector<uint8_t> bytes(62, 1);
  const std::vector<uint64_t> off = {0, 31, 62};
  // group_bys: every count up to TSDBHIP_MAX_TAGS, every width, exact-size arrays
  for (int nw = 1; nw <= 8; nw++)
    for (int ngb = 0; ngb <= TSDBHIP_MAX_TAGS; ngb++) {
      std::vector<uint8_t> gb((size_t)ngb * nw, 0);
      for (int g = 0; g < ngb; g++) gb[(size_t)g * nw + nw - 1] = (uint8_t)(g + 1);
      tsdbhip_keys_desc d = desc(gb, (uint8_t)ngb, 3, (uint8_t)nw, 3, off, bytes);
      CHECK(gb_check_desc(&d) == nullptr);
      if (ngb >= 2) {
        std::vector<uint8_t> dup = gb;  // the last name repeated
        memcpy(&dup[(size_t)(ngb - 1) * nw], &dup[(size_t)(ngb - 2) * nw], nw);
        d.group_bys = dup.data();
        CHECK(gb_check_desc(&d) != nullptr);
        std::vector<uint8_t> rev = gb;  // unsigned order: 0x80 after 0x7F
        rev[(size_t)(ngb - 2) * nw] = 0x80;
        d.group_bys = rev.data();
        CHECK(gb_check_desc(&d) != nullptr);
      }
    }
  {
    std::vector<uint8_t> gb(27, 0);
    for (int g = 0; g < 9; g++) gb[g * 3 + 2] = (uint8_t)(g + 1);
    tsdbhip_keys_desc d = desc(gb, 9, 3, 3, 3, off, bytes);
    CHECK(gb_check_desc(&d) != nullptr);  // n_group_bys = 9
    for (int w : {0, 9, 255}) {
      d = desc(gb, 2, (uint8_t)w, 3, 3, off, bytes);
      CHECK(gb_check_desc(&d) != nullptr);
      d = desc(gb, 2, 3, (uint8_t)w, 3, off, bytes);
      CHECK(gb_check_desc(&d) != nullptr);
      d = desc(gb, 2, 3, 3, (uint8_t)w, off, bytes);
      CHECK(gb_check_desc(&d) != nullptr);
    }
    d = desc(gb, 1, 3, 3, 3, off, bytes);
    d.group_bys = nullptr;
    CHECK(gb_check_desc(&d) != nullptr);
    d = desc(gb, 1, 3, 3, 3, off, bytes);
    d.key_off = nullptr;
    CHECK(gb_check_desc(&d) != nullptr);
    d = desc(gb, 0, 3, 3, 3, {}, {});  // no spans: nothing to point at
    d.key_off = nullptr;
    d.key_bytes = nullptr;
    CHECK(gb_check_desc(&d) == nullptr);
  }
  // key_off: n_spans + 1 entries exactly
  for (uint32_t n : {0u, 1u, 2u, 63u, 1000u}) {
    std::vector<uint64_t> o(n + 1);
    for (uint32_t s = 0; s <= n; s++) o[s] = 31ull * s;
    CHECK(gb_check_key_off(o.data(), n, 31ull * n) == -1);
    if (!n) continue;
    CHECK(gb_check_key_off(o.data(), n, 31ull * n + 1) == (int64_t)n);  // does not end at key_nbytes
    CHECK(gb_check_key_off(o.data(), n, 31ull * n - 1) == (int64_t)n - 1);  // runs past the key bytes
    std::vector<uint64_t> dec = o;
    dec[n / 2] = dec[n / 2 + (n / 2 < n ? 1 : 0)] + 1;
    if (n / 2 < n) CHECK(gb_check_key_off(dec.data(), n, 31ull * n) >= 0);
    std::vector<uint64_t> huge = o;
    huge[n] = ~0ull;
    CHECK(gb_check_key_off(huge.data(), n, 31ull * n) == (int64_t)n - 1);
  }
  // order: n entries exactly
  for (uint32_t n : {0u, 1u, 64u, 1000u}) {
    std::vector<uint32_t> ord(n);
    for (uint32_t i = 0; i < n; i++) ord[i] = (i * 7u) % 100u;
    CHECK(gather_check_order(ord.data(), n, 100) == -1);
    if (!n) continue;
    CHECK(gather_check_order(ord.data(), n, 0) == 0);
    ord[n - 1] = 100;
    CHECK(gather_check_order(ord.data(), n, 100) == (int64_t)n - 1);
    ord[n - 1] = ~0u;
    CHECK(gather_check_order(ord.data(), n, 100) == (int64_t)n - 1);
  }
  printf("groupby host checks ok\n");
  return 0;
}
