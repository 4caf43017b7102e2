// san_scanrows.cc — the argument checks, the query builder and the row test of
// tsdbhip_scan_rows (opentsdb_amd/csrc/scanrows_host.h) as a stand-alone
// program, built with -fsanitize=address,undefined by tests/test_scan_rows.py:
// every argument error in its order, the key checks over every row, the scan
// times at their edges, and sr_match against a matcher that tries every
// placement of the items (the regexp's language, without the greedy walk).
// Every array is heap-allocated at its exact size, so a read past an end is a
// sanitizer report. No device, no library.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../opentsdb_amd/csrc/scanrows_host.h"

using namespace tsdb;

#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
      return 1;                                                   \
    }                                                             \
  } while (0)

typedef std::vector<uint8_t> Bytes;

struct Query {
  Bytes tags, gbs, values;
  std::vector<uint32_t> nvalues;
  tsdbhip_scan_query q;
  void finish(uint32_t n_tags, uint32_t n_gbs) {
    memset(&q, 0, sizeof q);
    q.flags = TSDBHIP_SCAN_END_UNSET;
    q.n_tags = n_tags;
    q.n_group_bys = n_gbs;
    q.tags = tags.empty() ? nullptr : tags.data();
    q.group_bys = gbs.empty() ? nullptr : gbs.data();
    q.group_by_nvalues = nvalues.empty() ? nullptr : nvalues.data();
    q.group_by_values = values.empty() ? nullptr : values.data();
  }
};

struct Table {
  Bytes metric, bytes;
  std::vector<uint64_t> off;
  std::vector<uint32_t> o32;
  std::vector<uint64_t> o64;
  Bytes o8;
  tsdbhip_scan_desc d;
  tsdbhip_scan_sel out;
  void fill(uint8_t mw, uint8_t nw, uint8_t vw, const std::vector<Bytes>& keys) {
    metric.assign(mw, 7);
    bytes.clear();
    off.assign(1, 0);
    for (const auto& k : keys) {
      bytes.insert(bytes.end(), k.begin(), k.end());
      off.push_back(bytes.size());
    }
    memset(&d, 0, sizeof d);
    d.n_rows = (uint32_t)keys.size();
    d.metric_width = mw;
    d.name_width = nw;
    d.value_width = vw;
    d.metric = metric.data();
    d.key_off = off.data();
    d.key_bytes = bytes.data();
    d.key_nbytes = bytes.size();
    o32.assign(1, 0);
    o64.assign(1, 0);
    o8.assign(1, 0);
    memset(&out, 0, sizeof out);
    out.row_capacity = d.n_rows;
    out.key_capacity = bytes.size();
    out.row_index = o32.data();
    out.key_off = o64.data();
    out.key_bytes = o8.data();
  }
};

static Bytes key_of(uint8_t mw, uint32_t base, const std::vector<Bytes>& pairs) {
  Bytes k(mw, 7);
  for (int i = 3; i >= 0; i--) k.push_back((uint8_t)(base >> (8 * i)));
  for (const auto& p : pairs) k.insert(k.end(), p.begin(), p.end());
  return k;
}

static bool has(const char* s, const char* word) { return s && strstr(s, word); }

// every placement: item i at some pair after item i - 1's
static bool brute(const std::vector<Bytes>& pairs, size_t from, const std::vector<std::vector<Bytes>>& items, size_t i) {
  if (i == items.size()) return true;
  for (size_t p = from; p < pairs.size(); p++)
    for (const auto& alt : items[i])  // name | value, or the name alone: any value
      if (memcmp(pairs[p].data(), alt.data(), alt.size()) == 0 && brute(pairs, p + 1, items, i + 1)) return true;
  return false;
}

int main() {
  // ---- arguments, in their order ----
  std::vector<Bytes> keys;
  for (uint32_t r = 0; r < 70; r++) {
    std::vector<Bytes> pairs;
    for (uint32_t t = 0; t < r % 9; t++) pairs.push_back(Bytes{0, 0, (uint8_t)(t + 1), 0, 0, (uint8_t)r});
    keys.push_back(key_of(3, 1000 + r, pairs));
  }
  Table t;
  t.fill(3, 3, 3, keys);
  Query q;
  q.finish(0, 0);
  CHECK(sr_check_args(&t.d, &q.q, &t.out) == nullptr);
  CHECK(sr_first_error(fs_rows_of(&t.d)) == FS_NO_ERROR);
  q.tags = Bytes{0, 0, 2, 0, 0, 1, 0, 0, 1, 0, 0, 1};  // 2 then 1
  q.gbs = Bytes{0, 0, 3, 0, 0, 3};
  q.finish(9, 9);
  t.d.value_width = 9;
  CHECK(has(sr_check_args(&t.d, &q.q, &t.out), "width"));
  t.d.value_width = 3;
  CHECK(has(sr_check_args(&t.d, &q.q, &t.out), "MAX_TAGS tags"));
  q.finish(2, 9);
  CHECK(has(sr_check_args(&t.d, &q.q, &t.out), "MAX_TAGS group_bys"));
  q.finish(2, 2);
  CHECK(has(sr_check_args(&t.d, &q.q, &t.out), "tags not strictly"));
  q.tags = Bytes{0, 0, 1, 0, 0, 1, 0, 0, 3, 0, 0, 1};
  q.finish(2, 2);
  CHECK(has(sr_check_args(&t.d, &q.q, &t.out), "group_bys not strictly"));
  q.gbs = Bytes{0, 0, 2, 0, 0, 3};
  q.finish(2, 2);
  CHECK(has(sr_check_args(&t.d, &q.q, &t.out), "both"));
  q.gbs = Bytes{0, 0, 2, 0, 0, 4};
  q.nvalues = {0, 2};
  q.finish(2, 2);
  CHECK(has(sr_check_args(&t.d, &q.q, &t.out), "group_by_values is null"));
  q.values = Bytes{0, 0, 9, 0, 0, 8};
  q.finish(2, 2);
  CHECK(sr_check_args(&t.d, &q.q, &t.out) == nullptr);
  q.q.tags = nullptr;
  CHECK(has(sr_check_args(&t.d, &q.q, &t.out), "tags is null"));
  q.finish(2, 2);
  t.out.row_index = nullptr;
  CHECK(has(sr_check_args(&t.d, &q.q, &t.out), "null output"));
  t.fill(3, 3, 3, keys);
  t.d.row_status = t.o8.data();
  CHECK(has(sr_check_args(&t.d, &q.q, &t.out), "row_status"));
  t.fill(3, 3, 3, keys);
  t.d.row_qual_off = t.o64.data();
  CHECK(has(sr_check_args(&t.d, &q.q, &t.out), "four cell arrays"));
  t.fill(3, 3, 3, {});  // no rows: nothing to point at
  t.d.key_off = nullptr;
  t.d.key_bytes = nullptr;
  t.d.metric = nullptr;
  memset(&t.out, 0, sizeof t.out);
  CHECK(sr_check_args(&t.d, &q.q, &t.out) == nullptr);
  CHECK(sr_first_error(fs_rows_of(&t.d)) == FS_NO_ERROR);

  // ---- the key checks: every row, the first offender; rows of another metric are none ----
  {
    std::vector<Bytes> k2 = keys;
    k2[50][0] ^= 1;  // another metric: no error
    t.fill(3, 3, 3, k2);
    CHECK(sr_first_error(fs_rows_of(&t.d)) == FS_NO_ERROR);
    k2[69].push_back(0);
    k2[33] = Bytes(6, 7);
    t.fill(3, 3, 3, k2);
    CHECK(sr_first_error(fs_rows_of(&t.d)) == ((33ull << 8) | FS_E_SHAPE));
    k2[33] = keys[33];
    t.fill(3, 3, 3, k2);
    CHECK(sr_first_error(fs_rows_of(&t.d)) == ((69ull << 8) | FS_E_SHAPE));
    t.fill(3, 3, 3, keys);
    t.off[35] = ~0ull - 3;
    CHECK(sr_first_error(fs_rows_of(&t.d)) == ((34ull << 8) | FS_E_OFF));
    t.fill(3, 3, 3, keys);
    t.d.key_nbytes += 1;
    CHECK(sr_first_error(fs_rows_of(&t.d)) == FS_E_END);
    char buf[160];
    CHECK(fs_error((34ull << 8) | FS_E_OFF, buf, sizeof buf) == TSDBHIP_E_INVALID_ARG && strstr(buf, "row 34"));
  }

  // ---- the scan times ----
  {
    t.fill(3, 3, 3, keys);
    SrQuery s;
    std::vector<uint64_t> ids;
    Query e;
    e.finish(0, 0);
    e.q.flags = 0;
    auto times = [&](uint32_t a, uint32_t b, uint32_t iv) {
      e.q.start_time = a;
      e.q.end_time = b;
      e.q.sample_interval = iv;
      sr_build_query(&t.d, &e.q, &s, &ids);
    };
    times(0, 0, 0);
    CHECK(s.t_start == 0 && s.t_stop == 3601 && !s.filter);
    times(7200, 0, 0);
    CHECK(s.t_start == 0);
    times(7201, 0, 0);
    CHECK(s.t_start == 1);
    times(0xFFFFFFFFu, 0xFFFFFFFFu - 3601, 0);
    CHECK(s.t_start == 0xFFFFFFFFu - 7200 && s.t_stop == 0xFFFFFFFFu);
    times(0, 0xFFFFFFFFu - 3600, 0);
    CHECK(s.t_stop == 0);
    times(0, 0xFFFFFFFFu - 3600, 5);
    CHECK(s.t_stop == 5);
    times(100, 0xFFFFFFFFu, 0xFFFFFFFFu);
    CHECK(s.t_start == 0 && s.t_stop == 3599);
    e.q.flags = TSDBHIP_SCAN_END_UNSET;
    times(0, 5, 0);
    CHECK(s.t_stop == 0xFFFFFFFFu);
  }

  // ---- sr_match against every placement: widths, repeated and unsorted names, lists short and long ----
  for (auto w : std::vector<std::vector<uint8_t>>{{3, 3, 3}, {1, 1, 1}, {2, 1, 4}, {1, 8, 8}}) {
    const uint8_t mw = w[0], nw = w[1], vw = w[2];
    uint32_t x = 2463534242u, n_match = 0, n_all = 0;
    auto rnd = [&](uint32_t m) {
      x ^= x << 13, x ^= x >> 17, x ^= x << 5;
      return (x >> 8) % m;
    };
    auto id = [&](uint32_t width, uint32_t v) {  // ids 0..3 ascending, with extreme bytes; others apart from them
      static const uint8_t tab[4] = {0x00, 0x01, 0x5C, 0xFF};
      Bytes b(width, v < 4 ? tab[v] : 0x40);
      if (v >= 4) b[width - 1] = (uint8_t)v;
      return b;
    };
    for (int c = 0; c < 3000; c++) {
      std::vector<Bytes> pairs;
      for (uint32_t p = rnd(9); p > 0; p--) {
        Bytes b = id(nw, rnd(4)), v = id(vw, rnd(4));
        b.insert(b.end(), v.begin(), v.end());
        pairs.push_back(b);
      }
      Table one;
      one.fill(mw, nw, vw, {key_of(mw, 5000, pairs)});
      // items over names 0..3 in order, each a fixed tag, any value or a list
      Query u;
      std::vector<std::vector<Bytes>> items;
      uint32_t nt = 0, ng = 0;
      for (uint32_t name = 0; name < 4; name++) {
        const uint32_t kind = rnd(6);
        if (kind >= 3) continue;
        const Bytes nm = id(nw, name);
        std::vector<Bytes> alts;
        if (kind == 0) {
          Bytes v = id(vw, rnd(4));
          u.tags.insert(u.tags.end(), nm.begin(), nm.end());
          u.tags.insert(u.tags.end(), v.begin(), v.end());
          Bytes a = nm;
          a.insert(a.end(), v.begin(), v.end());
          alts.push_back(a);
          nt++;
        } else {
          u.gbs.insert(u.gbs.end(), nm.begin(), nm.end());
          const uint32_t nv = kind == 1 ? 0 : (rnd(3) == 0 ? 40 : 1 + rnd(3));  // 40: past SR_LIST_LINEAR
          u.nvalues.push_back(nv);
          for (uint32_t j = 0; j < nv; j++) {
            Bytes v = id(vw, j < 3 ? rnd(4) : 100 + rnd(100));
            u.values.insert(u.values.end(), v.begin(), v.end());
            Bytes a = nm;
            a.insert(a.end(), v.begin(), v.end());
            alts.push_back(a);
          }
          if (!nv) alts.push_back(nm);
          ng++;
        }
        items.push_back(alts);
      }
      u.finish(nt, ng);
      CHECK(sr_check_args(&one.d, &u.q, &one.out) == nullptr);
      SrQuery s;
      std::vector<uint64_t> ids;
      sr_build_query(&one.d, &u.q, &s, &ids);
      s.ids = ids.data();
      const FsRows rows = fs_rows_of(&one.d);
      CHECK(fs_check_key(rows, one.off[0], one.off[1]) == 0);
      const bool got = sr_match(one.bytes.data(), (uint32_t)one.bytes.size(), rows, s);
      CHECK(got == brute(pairs, 0, items, 0));
      n_match += got;
      n_all++;
      // the range: the base time below the start, and another metric
      Query r2 = u;
      r2.finish(nt, ng);
      r2.q.start_time = 5001 + 7200;
      sr_build_query(&one.d, &r2.q, &s, &ids);
      s.ids = ids.data();
      CHECK(!sr_match(one.bytes.data(), (uint32_t)one.bytes.size(), rows, s));
      one.metric[mw - 1] ^= 1;
      sr_build_query(&one.d, &u.q, &s, &ids);
      s.ids = ids.data();
      CHECK(!sr_match(one.bytes.data(), (uint32_t)one.bytes.size(), fs_rows_of(&one.d), s));
    }
    CHECK(n_match * 20 > n_all && n_match < n_all);  // both answers are well represented
  }
  printf("scanrows host checks ok\n");
  return 0;
}
