// san_findspans.cc — the argument and row checks of tsdbhip_find_spans
// (opentsdb_amd/csrc/findspans_host.h) as a stand-alone program, built with
// -fsanitize=address,undefined by tests/test_find_spans.py: the descriptor
// check, the per-row check the kernels share (every class, the first
// offending row, no key byte read before it is proven in range), the message
// and code of every class, and the sort-key digits against a literal SpanCmp.
// Every array is heap-allocated at its exact size, so a read past an end is a
// sanitizer report. No device, no library.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../opentsdb_amd/csrc/findspans_host.h"

using namespace tsdb;

#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
      return 1;                                                   \
    }                                                             \
  } while (0)

struct Scan {
  std::vector<uint8_t> metric, bytes, status;
  std::vector<uint64_t> off, qoff, voff;
  std::vector<uint32_t> qlen, vlen;
  tsdbhip_scan_desc d;
  // outputs: never written by the checks, only their presence matters
  std::vector<uint32_t> o32;
  std::vector<uint64_t> o64;
  std::vector<uint8_t> o8;
  tsdbhip_spans_out out;
};

static std::vector<uint8_t> key_of(uint8_t mw, uint8_t nw, uint8_t vw, uint32_t ntags, uint8_t seed) {
  std::vector<uint8_t> k(mw, 7);
  for (int i = 0; i < 4; i++) k.push_back((uint8_t)(seed + i));
  for (uint32_t t = 0; t < ntags; t++) {
    for (uint8_t i = 0; i < nw; i++) k.push_back(i + 1 == nw ? (uint8_t)(t + 1) : 0);
    for (uint8_t i = 0; i < vw; i++) k.push_back((uint8_t)(seed * 3 + i));
  }
  return k;
}

static void fill(Scan& s, uint8_t mw, uint8_t nw, uint8_t vw, const std::vector<std::vector<uint8_t>>& keys,
                 bool with_status, bool with_cells) {
  s.metric.assign(mw, 7);
  s.bytes.clear();
  s.off.assign(1, 0);
  for (const auto& k : keys) {
    s.bytes.insert(s.bytes.end(), k.begin(), k.end());
    s.off.push_back(s.bytes.size());
  }
  const size_t n = keys.size();
  s.status.assign(n, TSDBHIP_ROW_SINGLE);
  s.qoff.resize(n);
  s.voff.resize(n);
  s.qlen.assign(n, 4);
  s.vlen.assign(n, 9);
  for (size_t r = 0; r < n; r++) s.qoff[r] = 4 * r, s.voff[r] = 9 * r;
  memset(&s.d, 0, sizeof s.d);
  s.d.n_rows = (uint32_t)n;
  s.d.metric_width = mw;
  s.d.name_width = nw;
  s.d.value_width = vw;
  s.d.metric = s.metric.data();
  s.d.key_off = s.off.data();
  s.d.key_bytes = s.bytes.data();
  s.d.key_nbytes = s.bytes.size();
  if (with_status) s.d.row_status = s.status.data();
  if (with_cells) {
    s.d.row_qual_off = s.qoff.data();
    s.d.row_qual_len = s.qlen.data();
    s.d.row_val_off = s.voff.data();
    s.d.row_val_len = s.vlen.data();
  }
  s.o32.assign(1, 0);
  s.o64.assign(1, 0);
  s.o8.assign(1, 0);
  memset(&s.out, 0, sizeof s.out);
  s.out.span_capacity = (uint32_t)n;
  s.out.key_capacity = s.bytes.size();
  s.out.row_order = s.out.row_base = s.out.row_ncells = s.out.row_val_len = s.o32.data();
  s.out.span_row_start = s.out.row_qual_off = s.out.row_val_off = s.out.key_off = s.o64.data();
  s.out.key_bytes = s.o8.data();
}

static uint64_t first_error(const Scan& s) { return fs_first_error(fs_rows_of(&s.d)); }

static int code_of(uint64_t err, const char* word) {
  char buf[160];
  const int rc = fs_error(err, buf, sizeof buf);
  if (word && !strstr(buf, word)) {
    fprintf(stderr, "message '%s' lacks '%s'\n", buf, word);
    return 12345;
  }
  return rc;
}

// SpanCmp.compare (TsdbQuery.java:602-621), literally
static int span_cmp(const std::vector<uint8_t>& a, const std::vector<uint8_t>& b, int metric_width) {
  const int length = (int)(a.size() < b.size() ? a.size() : b.size());
  int i;
  for (i = 0; i < metric_width; i++)
    if (a[i] != b[i]) return (a[i] & 0xFF) - (b[i] & 0xFF);
  for (i += 4; i < length; i++)
    if (a[i] != b[i]) return (a[i] & 0xFF) - (b[i] & 0xFF);
  return (int)a.size() - (int)b.size();
}

static int digit_cmp(const std::vector<uint8_t>& a, const std::vector<uint8_t>& b, uint32_t mw, uint32_t pair) {
  const uint32_t P = TSDBHIP_MAX_TAGS * pair, hdr = mw + 4;
  const uint32_t la = (uint32_t)a.size() - hdr, lb = (uint32_t)b.size() - hdr;
  for (uint32_t d = 0; d <= P; d++) {
    const uint32_t x = fs_digit(a.data() + hdr, la, la / pair, P, d), y = fs_digit(b.data() + hdr, lb, lb / pair, P, d);
    if (x != y) return x < y ? -1 : 1;
  }
  return 0;
}

static int sign(int x) { return x < 0 ? -1 : (x > 0 ? 1 : 0); }

int main() {
  Scan s;
  // ---- descriptor ----
  std::vector<std::vector<uint8_t>> keys;
  for (uint32_t r = 0; r < 70; r++) keys.push_back(key_of(3, 3, 3, r % 9, (uint8_t)r));
  fill(s, 3, 3, 3, keys, true, true);
  CHECK(fs_check_desc(&s.d, &s.out) == nullptr);
  CHECK(first_error(s) == FS_NO_ERROR);
  for (int w : {0, 9, 255}) {
    Scan t;
    fill(t, 3, 3, 3, keys, true, true);
    t.d.metric_width = (uint8_t)w;
    CHECK(fs_check_desc(&t.d, &t.out) != nullptr);
    fill(t, 3, 3, 3, keys, true, true);
    t.d.name_width = (uint8_t)w;
    CHECK(fs_check_desc(&t.d, &t.out) != nullptr);
    fill(t, 3, 3, 3, keys, true, true);
    t.d.value_width = (uint8_t)w;
    CHECK(fs_check_desc(&t.d, &t.out) != nullptr);
  }
  {
    Scan t;
    fill(t, 3, 3, 3, keys, true, true);
    t.d.key_off = nullptr;
    CHECK(fs_check_desc(&t.d, &t.out) != nullptr);
    fill(t, 3, 3, 3, keys, true, true);
    t.d.metric = nullptr;
    CHECK(fs_check_desc(&t.d, &t.out) != nullptr);
    fill(t, 3, 3, 3, keys, true, true);
    t.d.row_val_len = nullptr;  // three of the four cell arrays
    CHECK(fs_check_desc(&t.d, &t.out) != nullptr);
    fill(t, 3, 3, 3, keys, true, true);
    t.out.row_ncells = nullptr;
    CHECK(fs_check_desc(&t.d, &t.out) != nullptr);
    fill(t, 3, 3, 3, keys, true, false);
    t.out.row_ncells = nullptr;  // no cells: not needed
    t.out.row_qual_off = t.out.row_val_off = nullptr;
    t.out.row_val_len = nullptr;
    CHECK(fs_check_desc(&t.d, &t.out) == nullptr);
    t.out.span_row_start = nullptr;
    CHECK(fs_check_desc(&t.d, &t.out) != nullptr);
    fill(t, 3, 3, 3, {}, false, false);  // no rows: nothing to point at
    t.d.key_off = nullptr;
    t.d.key_bytes = nullptr;
    t.d.metric = nullptr;
    memset(&t.out, 0, sizeof t.out);
    CHECK(fs_check_desc(&t.d, &t.out) == nullptr);
    CHECK(fs_first_error(fs_rows_of(&t.d)) == FS_NO_ERROR);
  }
  // ---- rows: every class, the first offender, the order on one row ----
  {
    Scan t;
    fill(t, 3, 3, 3, keys, true, true);
    t.status[40] = TSDBHIP_ROW_ERROR;
    CHECK(first_error(t) == ((40ull << 8) | FS_E_ROW_ERROR));
    CHECK(code_of(first_error(t), "row 40") == TSDBHIP_E_ILLEGAL_DATA);
    t.bytes[t.off[50] + 2] ^= 1;  // a foreign metric later: the lower row wins
    CHECK(first_error(t) == ((40ull << 8) | FS_E_ROW_ERROR));
    t.bytes[t.off[30]] ^= 0x80;  // and earlier
    CHECK(first_error(t) == ((30ull << 8) | FS_E_METRIC));
    CHECK(code_of(first_error(t), "row 30") == TSDBHIP_E_ILLEGAL_DATA);
    t.status[30] = TSDBHIP_ROW_OOB;  // on one row the metric wins
    CHECK(first_error(t) == ((30ull << 8) | FS_E_METRIC));
    t.bytes[t.off[30]] ^= 0x80;
    CHECK(first_error(t) == ((30ull << 8) | FS_E_ROW_OOB));
    CHECK(code_of(first_error(t), "row 30") == TSDBHIP_E_OUT_OF_BOUNDS);
    t.status[30] = 6;
    CHECK(first_error(t) == ((30ull << 8) | FS_E_STATUS));
    CHECK(code_of(first_error(t), "row 30") == TSDBHIP_E_INVALID_ARG);
    t.status[30] = TSDBHIP_ROW_NONE;
    t.qlen[30] = 3;  // a row that is not added: its cell is not looked at
    t.qoff[30] = 1;
    CHECK(first_error(t) == ((40ull << 8) | FS_E_ROW_ERROR));
    t.status[30] = TSDBHIP_ROW_TRIVIAL;
    CHECK(first_error(t) == ((30ull << 8) | FS_E_CELL));
    t.qlen[30] = 4;
    CHECK(first_error(t) == ((30ull << 8) | FS_E_CELL));  // the odd offset alone
    CHECK(code_of(first_error(t), "row 30") == TSDBHIP_E_INVALID_ARG);
    t.qoff[30] = 2;
    t.bytes[t.off[30]] ^= 0x80;  // an argument error before the metric
    t.qlen[30] = 1;
    CHECK(first_error(t) == ((30ull << 8) | FS_E_CELL));
  }
  {  // key shapes
    for (int cut : {1, 5}) {  // a tag part of one byte too many / too few
      std::vector<std::vector<uint8_t>> k2 = keys;
      if (cut == 1) k2[9].push_back(0);
      else k2[9].pop_back();
      Scan t;
      fill(t, 3, 3, 3, k2, false, false);
      CHECK(first_error(t) == ((9ull << 8) | FS_E_SHAPE));
      CHECK(code_of(first_error(t), "row 9") == TSDBHIP_E_INVALID_ARG);
    }
    std::vector<std::vector<uint8_t>> k2 = keys;
    k2[0] = std::vector<uint8_t>(6, 7);  // metric_width + 3 bytes
    k2[5] = key_of(3, 3, 3, 9, 1);       // nine pairs
    Scan t;
    fill(t, 3, 3, 3, k2, false, false);
    CHECK(first_error(t) == ((0ull << 8) | FS_E_SHAPE));
    k2[0] = key_of(3, 3, 3, 0, 1);  // no tags at all: fine
    fill(t, 3, 3, 3, k2, false, false);
    CHECK(first_error(t) == ((5ull << 8) | FS_E_SHAPE));
    k2[5] = key_of(3, 3, 3, 8, 1);
    fill(t, 3, 3, 3, k2, false, false);
    CHECK(first_error(t) == FS_NO_ERROR);
  }
  {  // key_off
    Scan t;
    fill(t, 3, 3, 3, keys, false, false);
    t.d.key_nbytes += 1;  // does not end at key_nbytes: before any row
    t.bytes[t.off[3]] ^= 1;
    CHECK(first_error(t) == FS_E_END);
    CHECK(code_of(first_error(t), "key_off") == TSDBHIP_E_INVALID_ARG);
    fill(t, 3, 3, 3, keys, false, false);
    t.off[35] = t.off[36] + 1;  // decreasing in the middle
    CHECK(first_error(t) == ((34ull << 8) | FS_E_SHAPE) || first_error(t) == ((35ull << 8) | FS_E_OFF));
    fill(t, 3, 3, 3, keys, false, false);
    t.off[35] = ~0ull - 3;  // far past the key bytes: never read
    CHECK(first_error(t) == ((34ull << 8) | FS_E_OFF));
    CHECK(code_of(first_error(t), "row 34") == TSDBHIP_E_INVALID_ARG);
  }
  // ---- the sort key is SpanCmp: widths, prefixes with all-zero extensions ----
  for (auto w : std::vector<std::vector<uint8_t>>{{3, 3, 3}, {2, 1, 4}, {1, 8, 8}}) {
    const uint32_t mw = w[0], pair = (uint32_t)w[1] + w[2];
    std::vector<std::vector<uint8_t>> ks;
    uint32_t x = 12345;
    for (int i = 0; i < 120; i++) {
      x = x * 1664525u + 1013904223u;
      const uint32_t nt = (x >> 8) % 9;
      std::vector<uint8_t> k(mw + 4, 7);
      for (uint32_t b = 0; b < nt * pair; b++) {
        x = x * 1664525u + 1013904223u;
        const uint32_t c = (x >> 16) % 4;
        k.push_back(c == 0 ? 0x00 : (c == 1 ? 0xFF : (uint8_t)((x >> 24) & 3)));
      }
      ks.push_back(k);
      if (nt < 8) {  // the same key extended by an all-zero pair
        k.insert(k.end(), pair, 0);
        ks.push_back(k);
      }
    }
    for (const auto& a : ks)
      for (const auto& b : ks) CHECK(sign(span_cmp(a, b, (int)mw)) == digit_cmp(a, b, mw, pair));
  }
  printf("findspans host checks ok\n");
  return 0;
}
