// k_groupby.hip — kernels of tsdbhip_groupby_plan (the grouping loop of
// TsdbQuery.groupByAndAggregate, TsdbQuery.java:310-348, and computeTags,
// SpanGroup.java:149-173, over the spans' row keys) and of
// tsdbhip_desc_gather (the spans' rows in the plan's batch order).
//
//   k_gb_keys      a lane per span: key_off / key shape / SpanCmp order checks
//                  (first offending span: one atomicMin word), the group key
//                  (Tags.getValueId per GROUP BY tag), the drop flag, and the
//                  AND / OR of every group-key byte over the grouped spans
//                  (a digit position whose AND == OR has one live bucket)
//   k_gb_count     per tile of GB_TILE sorted positions: the digit counts
//   (scan)         k_util's device-wide exclusive scan, digit-major
//   k_gb_scatter   stable scatter: rank inside a wave by ballot match, across
//                  the tile's 16 wave-rounds through LDS counts
//   k_gb_heads     head flags over the sorted group keys; (scan); k_gb_emit
//   k_gb_first     first kept position per group (one atomicMin per wave, group)
//   k_gb_masks     8-bit match mask against that span's pairs, AND-reduced per
//                  group (segmented in the wave, one atomicAnd per wave, group)
//   k_gb_finalize  a lane per group: tag count, pairs and common bits
#pragma once
#include "dev_common.h"

namespace tsdb {

constexpr uint32_t GB_THREADS = 256;
constexpr uint32_t GB_ITEMS = 4;                      // sorted positions per thread
constexpr uint32_t GB_TILE = GB_THREADS * GB_ITEMS;   // per block
constexpr uint32_t GB_WR = GB_ITEMS * (GB_THREADS / WAVE);  // wave-rounds per tile
constexpr uint32_t GB_MAX_KEY = 64;                   // TSDBHIP_MAX_TAGS * 8 bytes
constexpr uint32_t GB_KEY_WORDS = GB_MAX_KEY / 4;

// error word: (span << 8) | class, min-reduced: the first offending span
constexpr uint32_t GB_E_OFF = 1;       // key_off decreasing / past key_nbytes
constexpr uint32_t GB_E_SHAPE = 2;     // key length
constexpr uint32_t GB_E_UNSORTED = 3;  // not after its predecessor under SpanCmp
constexpr uint32_t GB_E_END = 4;       // key_off[n] != key_nbytes (span = n)

struct GbKeysArgs {
  uint32_t n, mw, nw, vw, ngb, klen;
  const uint64_t* key_off;
  const uint8_t* key;
  uint64_t key_nbytes;
  uint8_t gb[GB_MAX_KEY];  // the GROUP BY tag names, name_width bytes each
  uint8_t* gkey;           // [n * klen]
  uint8_t* drop;           // [n]
  uint8_t* ntags;          // [n]
  uint32_t* idx0;          // [n] the identity
  unsigned long long* err;
  uint32_t* andw;          // [GB_KEY_WORDS]
  uint32_t* orw;           // [GB_KEY_WORDS]
  uint32_t* n_dropped;
};

// w (1..8) bytes at p as a big-endian number
DEVI uint64_t gb_load(const uint8_t* p, uint32_t w) {
  uint64_t v = 0;
  for (uint32_t i = 0; i < w; i++) v = (v << 8) | p[i];
  return v;
}

// SpanCmp (TsdbQuery.java:602-621) of two keys of at least mw + 4 bytes
DEVI int gb_span_cmp(const uint8_t* a, uint64_t la, const uint8_t* b, uint64_t lb, uint32_t mw) {
  for (uint32_t i = 0; i < mw; i++)
    if (a[i] != b[i]) return (int)a[i] - (int)b[i];
  const uint64_t m = la < lb ? la : lb;
  for (uint64_t i = mw + 4; i < m; i++)
    if (a[i] != b[i]) return (int)a[i] - (int)b[i];
  return la < lb ? -1 : (la > lb ? 1 : 0);
}

__global__ void __launch_bounds__(256) k_gb_keys(GbKeysArgs a) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  const bool in = s < a.n;
  const uint32_t pair = a.nw + a.vw, hdr = a.mw + 4;
  bool ok = in, dropped = false;
  if (s == 0 && a.key_off[a.n] != a.key_nbytes)
    atomicMin(a.err, ((unsigned long long)a.n << 8) | GB_E_END);
  uint64_t o0 = 0, len = 0;
  uint32_t nt = 0;
  if (in) {
    o0 = a.key_off[s];
    const uint64_t o1 = a.key_off[s + 1];
    if (!(o0 <= o1 && o1 <= a.key_nbytes)) {
      atomicMin(a.err, ((unsigned long long)s << 8) | GB_E_OFF);
      ok = false;
    } else {
      len = o1 - o0;
      if (len < hdr || (len - hdr) % pair != 0 || (len - hdr) / pair > 8) {
        atomicMin(a.err, ((unsigned long long)s << 8) | GB_E_SHAPE);
        ok = false;
      } else {
        nt = (uint32_t)((len - hdr) / pair);
      }
    }
    a.idx0[s] = s;
  }
  if (ok && s > 0) {  // after its predecessor (whose own lane reports its shape)
    const uint64_t p0 = a.key_off[s - 1];
    if (p0 <= o0 && o0 - p0 >= hdr && gb_span_cmp(a.key + p0, o0 - p0, a.key + o0, len, a.mw) >= 0)
      atomicMin(a.err, ((unsigned long long)s << 8) | GB_E_UNSORTED);
  }
  if (ok) {
    // Tags.getValueId (Tags.java:213-227) per GROUP BY tag: a linear scan of
    // the key's pairs, the first match wins
    const uint8_t* tags = a.key + o0 + hdr;
    uint8_t* gk = a.gkey + (uint64_t)s * a.klen;
    for (uint32_t g = 0; g < a.ngb; g++) {
      const uint64_t want = gb_load(a.gb + g * a.nw, a.nw);
      uint32_t j = 0;
      for (; j < nt; j++)
        if (gb_load(tags + j * pair, a.nw) == want) break;
      if (j == nt) {
        dropped = true;
        break;
      }
      for (uint32_t b = 0; b < a.vw; b++) gk[g * a.vw + b] = tags[j * pair + a.nw + b];
    }
    a.drop[s] = dropped ? 1 : 0;
    a.ntags[s] = (uint8_t)nt;
  } else if (in) {
    a.drop[s] = 1;
    a.ntags[s] = 0;
  }
  const uint64_t dm = ballot(ok && dropped);
  if (lane_id() == 0 && dm) atomicAdd(a.n_dropped, (uint32_t)__popcll(dm));
  // AND / OR of the grouped spans' key bytes, a word at a time (klen is
  // uniform: the unrolled words stay in registers)
  const bool live = ok && !dropped;
  const uint8_t* gk = a.gkey + (uint64_t)s * a.klen;
#pragma unroll
  for (uint32_t w = 0; w < GB_KEY_WORDS; w++) {
    if (w * 4 >= a.klen) break;
    uint32_t v = 0;
    if (live)
      for (uint32_t b = 0; b < 4; b++)
        if (w * 4 + b < a.klen) v |= (uint32_t)gk[w * 4 + b] << (8 * b);
    uint32_t va = live ? v : ~0u, vo = live ? v : 0u;
#pragma unroll
    for (int m = 1; m < WAVE; m <<= 1) {
      va &= (uint32_t)__shfl_xor((int)va, m);
      vo |= (uint32_t)__shfl_xor((int)vo, m);
    }
    if (lane_id() == 0) {  // (an atomic only where it changes the word)
      const uint32_t ca = __hip_atomic_load(a.andw + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const uint32_t co = __hip_atomic_load(a.orw + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if ((ca & va) != ca) atomicAnd(a.andw + w, va);
      if ((co | vo) != co) atomicOr(a.orw + w, vo);
    }
  }
}

// ---- stable LSD radix sort of span indices, 8-bit digits --------------------
struct GbSortArgs {
  uint32_t n, nb;        // sorted positions, tiles
  const uint32_t* src;   // [n] span indices in the current order
  uint32_t* dst;         // [n]
  const uint8_t* dig;    // digit of span s: dig[s * stride + off]
  uint32_t stride, off;
  uint64_t* counts;      // [256 * nb] digit-major: counts[d * nb + tile]
  const uint64_t* offs;  // its exclusive scan
};

// The lanes of the wave holding digit d (valid lanes only): the lane's rank
// among them and their number.
DEVI void gb_match(uint32_t d, bool valid, uint32_t& rank, uint32_t& count, bool& leader) {
  uint64_t m = ballot(valid);
#pragma unroll
  for (int b = 0; b < 8; b++) {
    const bool bit = (d >> b) & 1u;
    const uint64_t bb = ballot(bit);
    m &= bit ? bb : ~bb;
  }
  const int lane = lane_id();
  rank = (uint32_t)__popcll(m & lanemask_lt(lane));
  count = (uint32_t)__popcll(m);
  leader = valid && rank == 0;
}

__global__ void __launch_bounds__(GB_THREADS) k_gb_count(GbSortArgs a) {
  __shared__ uint32_t s_h[256];
  const uint32_t t = threadIdx.x;
  s_h[t] = 0;
  __syncthreads();
  const uint64_t base = (uint64_t)blockIdx.x * GB_TILE;
#pragma unroll
  for (uint32_t j = 0; j < GB_ITEMS; j++) {
    const uint64_t e = base + j * GB_THREADS + t;
    const bool valid = e < a.n;
    const uint32_t d = valid ? a.dig[(uint64_t)a.src[e] * a.stride + a.off] : 0u;
    uint32_t rank, count;
    bool leader;
    gb_match(d, valid, rank, count, leader);
    if (leader) atomicAdd(&s_h[d], count);
  }
  __syncthreads();
  a.counts[(uint64_t)t * a.nb + blockIdx.x] = s_h[t];
}

__global__ void __launch_bounds__(GB_THREADS) k_gb_scatter(GbSortArgs a) {
  __shared__ uint32_t s_cnt[GB_WR][256];
  const uint32_t t = threadIdx.x, w = t / WAVE;
  for (uint32_t i = 0; i < GB_WR; i++) s_cnt[i][t] = 0;
  __syncthreads();
  const uint64_t base = (uint64_t)blockIdx.x * GB_TILE;
  uint32_t span[GB_ITEMS], dg[GB_ITEMS], rk[GB_ITEMS];
  bool vl[GB_ITEMS];
#pragma unroll
  for (uint32_t j = 0; j < GB_ITEMS; j++) {  // wave-round j * 4 + w holds positions in order
    const uint64_t e = base + j * GB_THREADS + t;
    vl[j] = e < a.n;
    span[j] = vl[j] ? a.src[e] : 0u;
    dg[j] = vl[j] ? a.dig[(uint64_t)span[j] * a.stride + a.off] : 0u;
    uint32_t count;
    bool leader;
    gb_match(dg[j], vl[j], rk[j], count, leader);
    if (leader) s_cnt[j * (GB_THREADS / WAVE) + w][dg[j]] = count;
  }
  __syncthreads();
  {  // digit t: where each wave-round's run of it starts
    uint32_t run = (uint32_t)a.offs[(uint64_t)t * a.nb + blockIdx.x];
    for (uint32_t i = 0; i < GB_WR; i++) {
      const uint32_t c = s_cnt[i][t];
      s_cnt[i][t] = run;
      run += c;
    }
  }
  __syncthreads();
#pragma unroll
  for (uint32_t j = 0; j < GB_ITEMS; j++) {
    if (!vl[j]) continue;
    const uint32_t at = s_cnt[j * (GB_THREADS / WAVE) + w][dg[j]] + rk[j];
    if (at < a.n) a.dst[at] = span[j];
  }
}

// ---- group boundaries --------------------------------------------------------
struct GbGroupArgs {
  uint32_t ng;  // grouped spans (sorted positions [0, ng))
  uint32_t klen, mw, nw, vw, tag_stride;
  const uint32_t* ord;   // [ng] span at sorted position i
  const uint8_t* gkey;
  const uint64_t* key_off;
  const uint8_t* key;
  const uint8_t* kept;   // null: all kept
  const uint8_t* ntags;
  uint64_t* heads;       // [ng]
  const uint64_t* hscan; // exclusive scan of heads
  const uint64_t* n_groups;  // its total
  uint32_t* gid;         // [ng]
  uint32_t* first;       // [ng] first kept position per group (init ~0)
  uint32_t* common;      // [ng] (init ~0)
  uint32_t* gss;         // [ng + 1]
  uint8_t* out_key;      // [ng * klen]
  uint8_t* out_ntags;    // [ng]
  uint8_t* out_tags;     // [ng * tag_stride]
  uint8_t* out_common;   // [ng]
};

__global__ void __launch_bounds__(256) k_gb_heads(GbGroupArgs a) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.ng) return;
  bool head = i == 0;
  if (!head) {
    const uint8_t* x = a.gkey + (uint64_t)a.ord[i] * a.klen;
    const uint8_t* y = a.gkey + (uint64_t)a.ord[i - 1] * a.klen;
    for (uint32_t b = 0; b < a.klen && !head; b++) head = x[b] != y[b];
  }
  a.heads[i] = head ? 1 : 0;
}

__global__ void __launch_bounds__(256) k_gb_emit(GbGroupArgs a) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.ng) return;
  const bool head = a.heads[i] != 0;
  const uint32_t g = (uint32_t)a.hscan[i] + (head ? 1u : 0u) - 1u;  // (position 0 is a head)
  a.gid[i] = g;
  if (head) {
    a.gss[g] = i;
    const uint8_t* x = a.gkey + (uint64_t)a.ord[i] * a.klen;
    for (uint32_t b = 0; b < a.klen; b++) a.out_key[(uint64_t)g * a.klen + b] = x[b];
  }
}

// The wave's segments of equal group: hm has a bit per lane that starts one
// (lane 0, a group's head, a position past the end).
DEVI uint64_t gb_seg_heads(const GbGroupArgs& a, uint32_t i, uint32_t& g) {
  const bool in = i < a.ng;
  g = in ? a.gid[i] : 0u;
  const bool head = !in || lane_id() == 0 || a.gid[i - 1] != g;
  return ballot(head);
}

__global__ void __launch_bounds__(256) k_gb_first(GbGroupArgs a) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t g;
  const uint64_t hm = gb_seg_heads(a, i, g);
  const bool kept = i < a.ng && (!a.kept || a.kept[a.ord[i]] != 0);
  const uint64_t km = ballot(kept);
  const int lane = lane_id();
  const int seg0 = 63 - __clzll(hm & lanemask_le(lane));  // (bit 0 is set)
  const uint64_t before = km & lanemask_lt(lane) & ~lanemask_lt(seg0);
  if (kept && before == 0) atomicMin(&a.first[g], i);
}

// bit j: the span's key holds pair j of the base key (name and value)
DEVI uint32_t gb_tag_mask(const GbGroupArgs& a, uint32_t sp, uint32_t base) {
  const uint32_t pair = a.nw + a.vw, hdr = a.mw + 4;
  const uint8_t* bt = a.key + a.key_off[base] + hdr;
  const uint8_t* st = a.key + a.key_off[sp] + hdr;
  const uint32_t nb = a.ntags[base], ns = a.ntags[sp];
  uint32_t m = 0;
  for (uint32_t j = 0; j < nb; j++) {
    const uint64_t name = gb_load(bt + j * pair, a.nw), value = gb_load(bt + j * pair + a.nw, a.vw);
    for (uint32_t q = 0; q < ns; q++) {
      if (gb_load(st + q * pair, a.nw) != name) continue;
      if (gb_load(st + q * pair + a.nw, a.vw) == value) m |= 1u << j;
      break;  // (the first match wins)
    }
  }
  return m;
}

__global__ void __launch_bounds__(256) k_gb_masks(GbGroupArgs a) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t g;
  const uint64_t hm = gb_seg_heads(a, i, g);
  const bool kept = i < a.ng && (!a.kept || a.kept[a.ord[i]] != 0);
  uint32_t x = 0xFFu;
  if (kept) {
    const uint32_t f = a.first[g];  // (set: this position is kept)
    if (f != i && f < a.ng) x = gb_tag_mask(a, a.ord[i], a.ord[f]);
  }
  // segmented inclusive AND scan; a segment's last lane holds its AND
  const int l = lane_id();
#pragma unroll
  for (int d = 1; d < WAVE; d <<= 1) {
    const uint32_t y = shfl_up_u32(x, d);
    const uint64_t win = l >= d ? (lanemask_le(l) & ~lanemask_le(l - d)) : 0;
    if (l >= d && (hm & win) == 0) x &= y;
  }
  const bool last = l == WAVE - 1 || ((hm >> (l + 1)) & 1ull);
  if (i < a.ng && last && x != 0xFFu) atomicAnd(&a.common[g], x);
}

__global__ void __launch_bounds__(256) k_gb_finalize(GbGroupArgs a) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t G = *a.n_groups;
  if (g == 0) a.gss[G] = a.ng;
  if (g >= G) return;
  const uint32_t f = a.first[g];
  uint8_t* out = a.out_tags + (uint64_t)g * a.tag_stride;
  uint32_t nt = 0, nbytes = 0;
  if (f < a.ng) {
    const uint32_t base = a.ord[f];
    nt = a.ntags[base];
    nbytes = nt * (a.nw + a.vw);
    const uint8_t* bt = a.key + a.key_off[base] + a.mw + 4;
    for (uint32_t b = 0; b < nbytes && b < a.tag_stride; b++) out[b] = bt[b];
  }
  for (uint32_t b = nbytes; b < a.tag_stride; b++) out[b] = 0;
  a.out_ntags[g] = (uint8_t)nt;
  a.out_common[g] = (uint8_t)(a.common[g] & ((1u << nt) - 1u));
}

// ---- tsdbhip_desc_gather -------------------------------------------------------
struct GatherArgs {
  uint32_t n;
  uint64_t n_rows;  // gathered rows (k_gather_rows)
  const uint32_t* order;
  const uint64_t* in_srs;
  const uint32_t* in_base;
  const uint32_t* in_ncells;
  const uint64_t* in_qoff;
  const uint64_t* in_voff;
  const uint32_t* in_vlen;
  uint64_t* cnt;  // [n]
  uint64_t* out_srs;  // [n + 1]
  uint32_t* out_base;
  uint32_t* out_ncells;
  uint64_t* out_qoff;
  uint64_t* out_voff;
  uint32_t* out_vlen;
};

__global__ void __launch_bounds__(256) k_gather_count(GatherArgs a) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  const uint32_t s = a.order[i];
  a.cnt[i] = a.in_srs[s + 1] - a.in_srs[s];
}

// a lane per gathered row: its span by binary search in out_srs
__global__ void __launch_bounds__(256) k_gather_rows(GatherArgs a) {
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= a.n_rows) return;
  uint32_t lo = 0, hi = a.n;  // the last i with out_srs[i] <= r
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (a.out_srs[mid] <= r) lo = mid;
    else hi = mid;
  }
  const uint64_t src = a.in_srs[a.order[lo]] + (r - a.out_srs[lo]);
  a.out_base[r] = a.in_base[src];
  a.out_ncells[r] = a.in_ncells[src];
  a.out_qoff[r] = a.in_qoff[src];
  a.out_voff[r] = a.in_voff[src];
  a.out_vlen[r] = a.in_vlen[src];
}

}  // namespace tsdb
