"""Batches for the GROUP BY shape tests (test_batch_shapes_cpu.py,
test_batch_shapes.py) and a restatement of the geometry
tsdbhip_spangroup_run_batch computes on the host, so that every case can
assert that it reaches the regime it is named for: tile groups (tpw > 1),
span chunks (n_chunks > 1, direct-only and E chunks), many groups, bitmap
words on 1024-word edges and past 256 scan blocks, the wide-range fallback,
per-group capacities and lazy errors deep in a batch.

A Case is built once and cached. Big populations are written straight into
the packing.SpanSet arrays (pack_cells): one compacted row an hour, rows
8 B / 16 B aligned as packing.pack_spans lays them out."""
import numpy as np

import oracle
from helpers import T0, U32MAX
from opentsdb_amd import packing

# how a span's cells are written: minimal-width longs (TSDB.addPoint), 8-byte
# longs (IncomingDataPoints), float32, float64
KI, K8, KF4, KF8 = 0, 1, 2, 3
MODE_INT, MODE_DBL, MODE_DUAL = 0, 1, 2  # k_reduce.hip:27
SUM, MIN, MAX, AVG, DEV = 0, 1, 2, 3, 4

# ---- constants of the batch's host geometry, copied -------------------------
TARGET_WAVES = 16384   # batch.hip:421 (reduce_geom's target, api.hip, times the group's share)
MIN_WAVES = 2048       # batch.hip:422 (reduce_geom's min_waves, api.hip, times the share)
TARGET_FLOOR = 64      # batch.hip:421 (max(64, ...))
MIN_WAVES_FLOOR = 16   # batch.hip:422 (max(16, ...))
TILE = 64              # api.hip: reduce_geom's n_tiles (grid points a tile: one wave)
CHUNK_SPANS = 256      # api.hip: reduce_geom's by_size (chunks of ~256 spans)
CHUNK_MIN_SPANS = 16   # api.hip: reduce_geom's want (no chunk below 16 spans)
RANK_BLOCK = 1024      # batch.hip:328 (bitmap words a rank block; k_group.hip:192 block_sum[w >> 10])
SCAN_BLOCKS = 256      # k_grid_scan_blocks: rank blocks a round (batch.hip:342, one block of 256 threads)
STATS_BLOCKS = 65536   # batch.hip:193,330 (blocks of k_group_stats / k_group_words; they stride beyond)
GROUP_THREADS = 256    # batch.hip:323,348 (k_group_init / k_group_T: groups a block); k_group.hip:60 stride
WIDE_BITS = 1 << 32    # batch.hip:222 (W * 32 >= 2^32: groups one by one)
WIDE_WORDS = 1 << 28   # batch.hip:222
FAST_CELLS_PER_ROW = 64  # batch.hip:253 (wide rows: the streaming decode, and k_direct_scan without downsampling)


class Case:
    """A batch: the packed spans, the group boundaries and what the builders
    know of every span (first / last timestamp, cells, kind, regular cadence)."""

    def __init__(self, name, ss, gss, counts, kinds, ts, ival, fval, regular, start, end, meta):
        self.name, self.ss, self.gss = name, ss, np.asarray(gss, np.uint32)
        self.counts, self.kinds, self.ts, self.ival, self.fval = counts, kinds, ts, ival, fval
        self.regular = regular  # per span: written on one cadence at one 4 / 8 B width (a direct candidate)
        self.start, self.end, self.meta = int(start), int(end), meta
        self.pt0 = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)  # first point of span s
        self.first = ts[self.pt0[:-1]]
        self.last = ts[self.pt0[1:] - 1]
        self.G = len(self.gss) - 1
        self._ref = {}

    def sub(self, g):
        return self.ss.shard(int(self.gss[g]), int(self.gss[g + 1]))

    def ref(self, g, agg, rate=False, ds=(0, 0), capacity=None):
        """the oracle on group g alone, computed once a query and shared"""
        k = (g, agg, rate, ds if ds[0] else (0, 0), capacity)
        if k not in self._ref:
            self._ref[k] = oracle.spangroup(self.sub(g), self.start, self.end, agg, rate, ds[0], ds[1],
                                            capacity=capacity)
        return self._ref[k]

    def span_points(self, s):
        a, b = int(self.pt0[s]), int(self.pt0[s + 1])
        return self.ts[a:b]

    def capacities(self):
        """what core.run_spanset_batch gives a group by default: its cells"""
        cum = self.pt0[self.gss.astype(np.int64)]
        return np.maximum(1, cum[1:] - cum[:-1])


def pack_cells(counts, kinds, ts, ival, fval, bad3=()):
    """SpanSet of len(counts) spans: span s has counts[s] > 0 points (ts
    ascending, flat arrays in span order) written as kinds[s] says. bad3: flat
    point indices written as 3-byte longs (flags 2: an illegal width)."""
    counts = np.asarray(counts, np.int64)
    n_spans, N = len(counts), int(counts.sum())
    assert len(ts) == N and (counts > 0).all()
    sid = np.repeat(np.arange(n_spans, dtype=np.int64), counts)
    kind = np.asarray(kinds, np.int64)[sid]
    ts = np.asarray(ts, np.int64)
    ival = np.asarray(ival, np.int64)
    flt = kind >= KF4
    iw = np.where((ival >= -128) & (ival <= 127), 1,
                  np.where((ival >= -32768) & (ival <= 32767), 2,
                           np.where((ival >= -(1 << 31)) & (ival < (1 << 31)), 4, 8)))
    w = np.where(kind == KI, iw, np.where(kind == KF4, 4, 8))
    flags = np.where(flt, 0x8 | (w - 1), w - 1)
    bad3 = np.asarray(bad3, np.int64)
    if len(bad3):
        w[bad3], flags[bad3] = 3, 2
    be = ival.astype(">i8").view(np.uint8).reshape(N, 8).copy()
    f8 = kind == KF8
    be[f8] = np.asarray(fval, np.float64)[f8].astype(">f8").view(np.uint8).reshape(-1, 8)
    f4 = kind == KF4
    be[f4, 4:] = np.asarray(fval, np.float64)[f4].astype(">f4").view(np.uint8).reshape(-1, 4)
    base = ts - ts % 3600
    newrow = np.ones(N, bool)
    newrow[1:] = (sid[1:] != sid[:-1]) | (base[1:] != base[:-1])
    rid = np.cumsum(newrow) - 1
    rfirst = np.nonzero(newrow)[0]
    rcells = np.diff(np.append(rfirst, N))
    rvlen = np.add.reduceat(w, rfirst) + (rcells > 1)
    qlen_al = (2 * rcells + packing.QUAL_ALIGN - 1) // packing.QUAL_ALIGN * packing.QUAL_ALIGN
    vlen_al = (rvlen + packing.VAL_ALIGN - 1) // packing.VAL_ALIGN * packing.VAL_ALIGN
    qoff = np.cumsum(qlen_al) - qlen_al
    voff = np.cumsum(vlen_al) - vlen_al
    qb = np.zeros(int(qlen_al.sum()) + 16, np.uint8)
    q = ((ts - base) << 4) | flags
    qp = qoff[rid] + 2 * (np.arange(N) - rfirst[rid])
    qb[qp] = (q >> 8).astype(np.uint8)
    qb[qp + 1] = (q & 0xFF).astype(np.uint8)
    wcs = np.cumsum(w) - w
    vpos = voff[rid] + wcs - wcs[rfirst][rid]
    vb = np.zeros(int(vlen_al.sum()) + 16, np.uint8)
    for width in (1, 2, 3, 4, 8):
        sel = np.nonzero(w == width)[0]
        for j in range(width):
            vb[vpos[sel] + j] = be[sel, 8 - width + j]
    srs = np.zeros(n_spans + 1, np.uint64)
    srs[1:] = np.cumsum(np.bincount(sid[rfirst], minlength=n_spans))
    return packing.SpanSet(srs, base[rfirst].astype(np.uint32), rcells.astype(np.uint32), qoff.astype(np.uint64),
                           voff.astype(np.uint64), rvlen.astype(np.uint32), qb, vb)


class Build:
    """collects groups in batch order, then packs them all at once"""

    def __init__(self):
        self.counts, self.kinds, self.ts, self.ival, self.fval, self.sizes, self.regular = [], [], [], [], [], [], []
        self.n_spans = self.n_points = self.n_groups = 0

    def _add(self, counts, kinds, ts, vals, regular):
        counts, kinds = np.asarray(counts, np.int64), np.asarray(kinds, np.int64)
        flt = np.repeat(kinds >= KF4, counts)
        vals = np.asarray(vals)
        self.counts.append(counts)
        self.kinds.append(kinds)
        self.ts.append(np.asarray(ts, np.int64))
        self.ival.append(np.where(flt, 0, vals).astype(np.int64))
        self.fval.append(np.where(flt, vals, 0).astype(np.float64))
        self.regular.append(np.broadcast_to(np.asarray(regular, bool), counts.shape).copy())
        self.n_spans += len(counts)
        self.n_points += int(counts.sum())

    def group(self, spans, regular=False):
        """one group of spans [(ts, values, kind)]; returns (group index, its
        first span's index, its first span's first flat point index)"""
        at = (self.n_groups, self.n_spans, self.n_points)
        for ts, vals, kind in spans:
            if kind >= KF4:
                self._add([len(ts)], [kind], ts, np.asarray(vals, np.float64), regular)
            else:
                self._add([len(ts)], [kind], ts, np.asarray(vals, np.int64), regular)
        self.sizes.append(np.array([len(spans)], np.int64))
        self.n_groups += 1
        return at

    def bulk(self, counts, kinds, ts, ivals, fvals, sizes=None):
        """many small groups at once: spans of counts[s] points, groups of
        sizes[g] spans (default: one span a group)"""
        counts, kinds = np.asarray(counts, np.int64), np.asarray(kinds, np.int64)
        flt = np.repeat(kinds >= KF4, counts)
        at = self.n_groups
        self._add(counts, kinds, ts, np.where(flt, fvals, np.asarray(ivals, np.float64)), False)
        self.ival[-1] = np.where(flt, 0, ivals).astype(np.int64)  # (longs beyond 2^53 keep their bits)
        sizes = np.ones(len(counts), np.int64) if sizes is None else np.asarray(sizes, np.int64)
        assert int(sizes.sum()) == len(counts)
        self.sizes.append(sizes)
        self.n_groups += len(sizes)
        return at

    def done(self, name, start=0, end=U32MAX, bad3=(), **meta):
        cat = np.concatenate
        counts, kinds, ts = cat(self.counts), cat(self.kinds), cat(self.ts)
        ival, fval = cat(self.ival), cat(self.fval)
        ss = pack_cells(counts, kinds, ts, ival, fval, bad3)
        gss = cat([[0], np.cumsum(cat(self.sizes))])
        return Case(name, ss, gss, counts, kinds, ts, ival, fval, cat(self.regular), start, end, meta)


# ---- the restatement of spangroup_run_batch's host geometry -------------------
def reduce_geom(T, nk, one_chunk, target, min_waves):
    """api.hip: reduce_geom (no spc_cap: the batch passes none): (spc, n_chunks, tpw, ntg, n_waves)"""
    n_tiles = (T + TILE - 1) // TILE
    if one_chunk or nk == 0:
        n_chunks, spc = 1, max(nk, 1)
    else:
        want = max(1, target // n_tiles)
        by_size = max((nk + CHUNK_SPANS - 1) // CHUNK_SPANS, (min_waves + n_tiles - 1) // n_tiles)
        want = min(want, by_size, max(1, nk // CHUNK_MIN_SPANS))
        n_chunks = max(1, want)
        spc = (nk + n_chunks - 1) // n_chunks
        n_chunks = (nk + spc - 1) // spc
    tpw = max(1, (n_tiles * n_chunks + target - 1) // target)
    ntg = (n_tiles + tpw - 1) // tpw
    return spc, n_chunks, tpw, ntg, ntg * n_chunks


class Geom:
    pass


def geom(case, agg=SUM, rate=False, exact=False):
    """What spangroup_run_batch computes on the host for this batch (batch.hip:
    203-222 the segmented bitmap, :390-433 the reduce geometry): per group nk,
    lo, hi, nw, wbase, mode; W, nb, wide; and rg(g, T) = the group's reduce_geom
    result for a grid of T points."""
    q = Geom()
    gss = case.gss.astype(np.int64)
    G = case.G
    kept = (case.first <= case.end) & (case.last >= case.start)  # SpanGroup.add's filter (SpanGroup.java:135-139)
    ck = np.concatenate([[0], np.cumsum(kept)])
    q.kept, q.k0 = kept, ck[gss[:-1]]
    q.nk = ck[gss[1:]] - ck[gss[:-1]]
    q.n_kept = int(kept.sum())
    nonempty = np.nonzero(gss[1:] > gss[:-1])[0]
    first = np.full(G, np.iinfo(np.int64).max)
    last = np.full(G, np.iinfo(np.int64).min)
    isf = np.zeros(G, bool)
    isi = np.zeros(G, bool)
    cells = np.zeros(G, np.int64)
    if len(nonempty):
        at = gss[:-1][nonempty]
        first[nonempty] = np.minimum.reduceat(np.where(kept, case.first, np.iinfo(np.int64).max), at)
        last[nonempty] = np.maximum.reduceat(np.where(kept, case.last, np.iinfo(np.int64).min), at)
        isf[nonempty] = np.logical_or.reduceat(kept & (case.kinds >= KF4), at)
        isi[nonempty] = np.logical_or.reduceat(kept & (case.kinds < KF4), at)
        cells[nonempty] = np.add.reduceat(np.where(kept, case.counts, 0), at)
    has = q.nk > 0
    q.lo = np.where(has, np.maximum(case.start, first), 1)
    q.hi = np.where(has, np.minimum(case.end, last), 0)
    q.nw = np.where(q.lo <= q.hi, (q.hi - q.lo + 1 + 31) // 32, 0)
    q.wbase = np.cumsum(q.nw + 1) - (q.nw + 1)
    q.W = int((q.nw + 1).sum())
    q.nb = (q.W + RANK_BLOCK - 1) // RANK_BLOCK
    q.wide = q.W * 32 >= WIDE_BITS or q.W > WIDE_WORDS
    q.n_input = cells
    q.mode = np.where(rate, MODE_DBL, np.where(~isf, MODE_INT, np.where(~isi, MODE_DBL, MODE_DUAL)))
    # wide (hourly compacted) rows: without downsampling k_direct_scan runs (decode=auto)
    q.fast = case.ss.n_rows > 0 and int(cells.sum()) // case.ss.n_rows >= FAST_CELLS_PER_ROW

    def rg(g, T):
        share = q.nk[g] / q.n_kept if q.n_kept else 1.0
        seq = exact or (agg == DEV and q.mode[g] != MODE_DBL)
        return reduce_geom(int(T), int(q.nk[g]), seq, max(TARGET_FLOOR, int(TARGET_WAVES * share)),
                           max(MIN_WAVES_FLOOR, int(MIN_WAVES * share)))

    q.rg = rg
    return q


def direct_spans(case, g, rate=False):
    """k_direct_scan + k_direct_verify_seg restated for group g (full window):
    per span of the group, whether it stays direct: written on one cadence at
    one 4 / 8 B width, and its grid points consecutive ranks of the group's
    grid (no other span's point between two of its own)."""
    s0, s1 = int(case.gss[g]), int(case.gss[g + 1])
    skip = 1 if rate else 0
    pts = [case.span_points(s)[skip:] for s in range(s0, s1)]
    grid = np.unique(np.concatenate(pts))
    out = []
    for s, p in zip(range(s0, s1), pts):
        ok = bool(case.regular[s])
        if ok and len(p):
            ok = int(np.searchsorted(grid, p[-1]) - np.searchsorted(grid, p[0])) == len(p) - 1
        out.append(ok)
    return np.array(out)


# ---- value pools ---------------------------------------------------------------
def finite(rng, n):
    """positive values a float32 holds exactly"""
    return (50.0 + 100.0 * rng.random(n)).astype(np.float32).astype(np.float64)


def wide_ints(rng, n):
    """signed, every width: half within +-1000, half within +-2^40"""
    small = rng.integers(-1000, 1001, n)
    big = rng.integers(-(1 << 40), 1 << 40, n)
    return np.where(rng.random(n) < 0.5, small, big)


def counters(rng, n):
    return np.cumsum(rng.integers(1, 1000, n)) + int(rng.integers(0, 1 << 30))


def monotone(rng, counts):
    """(longs, floats) rising inside every span of counts[s] points (flat, span
    order), so that rates are positive and a sum of them does not cancel; the
    floats are values a float32 holds exactly"""
    counts = np.asarray(counts, np.int64)
    N = int(counts.sum())
    sid = np.repeat(np.arange(len(counts)), counts)
    first = (np.cumsum(counts) - counts)[sid]
    ci = np.cumsum(rng.integers(1, 1000, N))
    cf = np.cumsum(0.5 + 9.5 * rng.random(N))
    iv = ci - ci[first] + rng.integers(0, 1 << 30, len(counts))[sid]
    fv = (50.0 + cf - cf[first]).astype(np.float32).astype(np.float64)
    return iv, fv


def jitter_ts(rng, t0, n, max_gap):
    gaps = rng.integers(1, max_gap + 1, n)
    return t0 + np.cumsum(gaps) - gaps[0]


_CACHE = {}


def cached(fn):
    def wrapper(*a):
        k = (fn.__name__,) + a
        if k not in _CACHE:
            _CACHE[k] = fn(*a)
        return _CACHE[k]
    wrapper.__name__ = fn.__name__
    return wrapper


def _vals(rng, kind, n):
    if kind == "float":
        return finite(rng, n), KF4
    if kind == "counter":
        return counters(rng, n), K8
    if kind == "fmono":
        return monotone(rng, [n])[1], KF4
    if kind == "pos":
        return rng.integers(0, 1_000_000, n), KI
    return wide_ints(rng, n), KI


def _fillers(b, rng, n, t0):
    """n groups of one one-cell span, longs and floats alternating"""
    ts = t0 + 50 * np.arange(n) + rng.integers(0, 50, n)
    kinds = np.where(np.arange(n) % 2 == 0, KI, KF4)
    return b.bulk(np.ones(n, np.int64), kinds, ts, wide_ints(rng, n), finite(rng, n))


# ---- A / G: tile groups ------------------------------------------------------
POSITIONS = ("first", "middle", "last")
LONG_KINDS = ("int", "float", "dual", "rate")
N_FILL = 1000


def _long_group(b, rng, kind, n_a, t0):
    """3 jittered spans: a covers the whole range; b has no point in the
    middle 40 % of it (its bracket is carried over the tiles there); c ends
    at 60 % (its cursor stays at len for the last tiles)"""
    ta = jitter_ts(rng, t0, n_a, 400)
    lo, hi = int(ta[0]), int(ta[-1])
    span = hi - lo
    nb1 = int(0.3 * n_a)
    tb = np.concatenate([jitter_ts(rng, lo + 7, nb1, 400), jitter_ts(rng, lo + int(0.7 * span), nb1, 400)])
    tb = tb[tb < hi]
    tc = jitter_ts(rng, lo + int(0.1 * span), int(0.5 * n_a), 400)
    tc = tc[tc < lo + int(0.6 * span)]
    kinds = {"int": ("int", "int", "int"), "float": ("float", "float", "float"), "dual": ("pos", "float", "pos"),
             "rate": ("counter", "counter", "counter")}[kind]
    spans = []
    for t, k in zip((ta, tb, tc), kinds):
        v, code = _vals(rng, k, len(t))
        spans.append((t, v, code))
    return b.group(spans)


@cached
def tile_groups(pos, kind, bad=False):
    """A: two long groups (L1: ~4800 grid points, L2: ~8500) among N_FILL
    one-cell groups, so each holds under 1/256 of the kept spans and a wave
    carries its span state over 2, and 3 or more, tiles. bad (G): a 3-byte
    long late in L1's first span, +Inf late in L2's first span."""
    rng = np.random.default_rng([11, POSITIONS.index(pos), LONG_KINDS.index(kind), int(bad)])
    b = Build()
    half = N_FILL // 2
    n1, n2 = 2300, 4100
    t1, t2 = T0 + 100_000, T0 + 2_000_000
    if pos == "first":
        L1 = _long_group(b, rng, kind, n1, t1)
        _fillers(b, rng, N_FILL, T0)
        L2 = _long_group(b, rng, kind, n2, t2)
    elif pos == "middle":
        _fillers(b, rng, half, T0)
        L1 = _long_group(b, rng, kind, n1, t1)
        L2 = _long_group(b, rng, kind, n2, t2)
        _fillers(b, rng, half, T0 + 50 * half)
    else:
        L2 = _long_group(b, rng, kind, n2, t2)
        _fillers(b, rng, N_FILL, T0)
        L1 = _long_group(b, rng, kind, n1, t1)
    bad3, meta = (), {}
    if bad:
        assert kind == "dual"  # (span a of a dual group holds longs; +Inf goes into L2's float span b)
        i1 = L1[2] + int(0.7 * n1)
        # L2's span b follows span a's n2 points: a late point of it
        i2 = L2[2] + n2 + int(0.8 * np.concatenate(b.counts)[L2[1] + 1])
        bad3 = (i1,)
        meta = dict(bad_point=i1, inf_point=i2)
    c = b.done(f"tile_groups-{pos}-{kind}{'-bad' if bad else ''}", bad3=bad3, L1=L1[0], L2=L2[0], **meta)
    return _with_inf(c, i2, bad3) if bad else c


def _with_inf(c, point, bad3):
    fval = c.fval.copy()
    fval[point] = np.inf
    ss = pack_cells(c.counts, c.kinds, c.ts, c.ival, fval, bad3)
    return Case(c.name, ss, c.gss, c.counts, c.kinds, c.ts, c.ival, fval, c.regular, c.start, c.end, c.meta)


# ---- B: span chunks ------------------------------------------------------------
CHUNK_NK = (33, 49, 97, 300, 260)         # spans a group
CHUNK_KINDS = ("int", "float", "dual", "int", "float")


def _small_jittered(rng, nk, kinds, t0, width=900):
    """nk spans of 4..10 points inside [t0, t0 + width), their values rising
    (the rate runs sum positive terms): (counts, kinds, ts, ivals, fvals)"""
    counts = rng.integers(4, 11, nk)
    ts = []
    for n in counts:
        ts.append(np.sort(rng.choice(width, int(n), replace=False)) + t0)
    ts = np.concatenate(ts)
    return (counts, kinds, ts) + monotone(rng, counts)


def _kinds_of(kind, nk):
    if kind == "int":
        return np.full(nk, KI)
    if kind == "float":
        return np.full(nk, KF4)
    return np.where(np.arange(nk) % 3 == 1, KF4, KI)


@cached
def span_chunks():
    """B: jittered groups of 33, 49 and 97 spans on grids of at most 15 tiles
    (2, 3 and 6 chunks, the last one short), an int, a float and a dual one
    side by side, then an int group of 300 and a float group of 260 spans
    (more than k_group_stats' 256 threads; 18 and 16 chunks)"""
    rng = np.random.default_rng(21)
    b = Build()
    for i, (nk, kind) in enumerate(zip(CHUNK_NK, CHUNK_KINDS)):
        counts, kinds, ts, iv, fv = _small_jittered(rng, nk, _kinds_of(kind, nk), T0 + 5000 * i)
        b.bulk(counts, kinds, ts, iv, fv, sizes=[nk])
    return b.done("span_chunks")


DIRECT_NK = (33, 49, 97, 48, 48, 48, 48, 300, 260)
DIRECT_E_SPAN = 20  # the span of a 48-span group that needs E (chunk 1 of 3)
DIRECT_BIG_E_SPAN = 150  # the span of the 300-span group that needs E (chunk 8 of 18)


def _regular(b, rng, nk, kinds, t0=T0, n=360, step=10, special=None):
    """nk one-row spans of n cells on one cadence (8-byte longs / float32:
    direct candidates). special = (span, how): "gap": that span lacks cells
    100..119 (irregular: E, the others stay direct); "shift": it is 5 s off
    phase (its points lie between everyone's: every span needs E)"""
    spans = []
    for s in range(nk):
        ts = t0 + step * np.arange(n)
        reg = True
        if special and special[0] == s:
            if special[1] == "gap":
                ts = np.delete(ts, np.arange(100, 120))
                reg = False
            else:
                ts = ts + 5
        if kinds[s] >= KF4:
            v, k = monotone(rng, [len(ts)])[1], KF4
        else:
            v, k = counters(rng, len(ts)), K8
        spans.append((ts, v, k, reg))
    counts = [len(t) for t, _, _, _ in spans]
    kk = np.array([k for _, _, k, _ in spans])
    ts = np.concatenate([t for t, _, _, _ in spans])
    flt = np.repeat(kk >= KF4, counts)
    allv = np.concatenate([v for _, v, _, _ in spans])
    at = b.bulk(counts, kk, ts, np.where(flt, 0, allv).astype(np.int64), np.where(flt, allv, 0.0), sizes=[nk])
    b.regular[-1] = np.array([r for _, _, _, r in spans])
    return at


@cached
def direct_chunks():
    """B on wide hourly rows (k_direct_scan runs): groups of 33, 49 and 97
    regular spans (int, float, both), then four 48-span groups of 3 chunks:
    all direct; span 20 irregular (chunk 1 holds an E span, chunks 0 and 2
    are direct only); all direct again; span 20 phase-shifted (every chunk E);
    then an int group of 300 spans, span 150 irregular (one E chunk among 18),
    next to a float group of 260 (16 direct-only chunks): more spans than
    k_group_stats has threads"""
    rng = np.random.default_rng(22)
    b = Build()
    _regular(b, rng, 33, _kinds_of("int", 33))
    _regular(b, rng, 49, _kinds_of("float", 49))
    _regular(b, rng, 97, _kinds_of("dual", 97))
    _regular(b, rng, 48, _kinds_of("int", 48))
    _regular(b, rng, 48, _kinds_of("int", 48), special=(DIRECT_E_SPAN, "gap"))
    _regular(b, rng, 48, _kinds_of("float", 48))
    _regular(b, rng, 48, _kinds_of("int", 48), special=(DIRECT_E_SPAN, "shift"))
    _regular(b, rng, 300, _kinds_of("int", 300), special=(DIRECT_BIG_E_SPAN, "gap"))
    _regular(b, rng, 260, _kinds_of("float", 260))
    return b.done("direct_chunks")


# ---- C: many groups ------------------------------------------------------------
def many_layout(G):
    """where the special groups of a G-group batch sit: empty groups at index
    0, two in a row in the middle and at the end (with 65 537 groups the last
    one is the 3-span group past the stride's turn, so the empty one sits just
    before the pair)"""
    mid = G // 2
    if G > STATS_BLOCKS:
        three = (STATS_BLOCKS - 1, STATS_BLOCKS)  # the last of the first stride pass, the first of the second
        empty = (0, mid, mid + 1, STATS_BLOCKS - 2)
    else:
        three = (G - 3, G - 2)
        empty = (0, mid, mid + 1, G - 1)
    n_out = max(4, G // 40)
    before = np.arange(3, 3 + n_out)              # their span lies before the window: nk = 0
    after = np.arange(mid + 5, mid + 5 + n_out)   # after it: nk = 0
    straddle = np.arange(mid - 5 - n_out // 2, mid - 5)  # a point on either side: nk = 1, T = 0
    dual = np.arange(7, G - 4, 211 if G > 1000 else 23)
    return dict(three=three, empty=empty, before=before, after=after, straddle=straddle, dual=dual)


WIN0, WIN1 = T0 + 10_000, T0 + 10_000 + 4 * 70_000


@cached
def many_groups(G):
    """C: G groups, most of one one-cell span (longs and floats alternating),
    some of an int and a float span (dual), some empty, some outside the
    window [WIN0, WIN1] or around it without a point inside, and two 3-span
    interpolating groups (for G > 65536 at the turn of k_group_stats' stride)"""
    rng = np.random.default_rng([31, G])
    lay = many_layout(G)
    role = np.zeros(G, np.int64)  # 0 plain, 1 empty, 2 dual, 3 three-span, 4 before, 5 after, 6 straddle
    role[lay["dual"]] = 2
    role[lay["before"]] = 4
    role[lay["after"]] = 5
    role[lay["straddle"]] = 6
    role[list(lay["empty"])] = 1
    role[list(lay["three"])] = 3
    sizes = np.select([role == 1, role == 2, role == 3], [0, 2, 3], 1)
    S = int(sizes.sum())
    grp = np.repeat(np.arange(G), sizes)          # group of span s
    j = np.arange(S) - (np.cumsum(sizes) - sizes)[grp]  # index of the span in its group
    r = role[grp]
    counts = np.select([r == 6, r == 3], [2, 6], 1)
    kinds = np.where(r == 2, np.where(j == 0, KI, KF4), np.where(r == 3, KI, np.where(grp % 2 == 0, KI, KF4)))
    # first timestamp of every span: the group's slot inside the window, 4 s a group
    t_first = WIN0 + 4 * (grp % 70_000) + np.where(r == 2, j, 0)
    t_first = np.where(r == 4, WIN0 - 1 - (grp % 1000), t_first)
    t_first = np.where(r == 5, WIN1 + 1 + (grp % 1000), t_first)
    t_first = np.where(r == 6, WIN0 - 1 - (grp % 7), t_first)
    t_first = np.where(r == 3, WIN0 + 1000 + 3 * j, t_first)
    pt0 = np.cumsum(counts) - counts
    N = int(counts.sum())
    sp = np.repeat(np.arange(S), counts)
    i = np.arange(N) - pt0[sp]
    step = np.where(r[sp] == 6, WIN1 - WIN0 + 20, 7)  # (a straddling span: its second point past the window)
    ts = t_first[sp] + i * step
    c = Build()
    c.bulk(counts, kinds, ts, wide_ints(rng, N), finite(rng, N), sizes=sizes)
    lay["dual"] = np.nonzero(role == 2)[0]
    return c.done(f"many_groups-{G}", start=WIN0, end=WIN1, role=role, **lay)


def plain_expect(case):
    """closed form for the plain groups (one one-cell span inside the window):
    the group emits its own point under sum, min, max and avg, and 0 under dev.
    Returns (groups, ts, is_int, bits of the value)."""
    role = case.meta["role"]
    g = np.nonzero(role == 0)[0]
    s = case.gss[g].astype(np.int64)
    p = case.pt0[s]
    isint = case.kinds[s] < KF4
    bits = np.where(isint, case.ival[p], case.fval[p].view(np.int64))
    return g, case.ts[p], isint, bits


# ---- D: bitmap words -----------------------------------------------------------
EDGE_RANGES = (1, 31, 32, 33, 64)


def _two_spans(rng, lo, hi, n, kind="int", extra=()):
    """two spans over [lo, hi]: the first holds lo, hi and `extra`, the second n points between"""
    inner = np.arange(lo + 1, hi)
    a = np.sort(rng.choice(inner, min(n, len(inner)), replace=False)) if len(inner) else np.array([], np.int64)
    bb = np.sort(rng.choice(inner, min(n, len(inner)), replace=False)) if len(inner) else np.array([], np.int64)
    ta = np.unique(np.concatenate([[lo], a, [hi], np.asarray(extra, np.int64)]))
    tb = bb if len(bb) else np.array([lo])
    out = []
    for t in (ta, tb):
        v, code = _vals(rng, kind, len(t))
        out.append((t, v, code))
    return out


MONO = {"int": "counter", "float": "fmono", "pos": "counter"}


@cached
def word_edges(mono=False):
    """D: ranges of 1, 31, 32, 33 and 64 s; a group whose pad word is the last
    word of a rank block (1023); a group of 1024 * 32 s whose pad word is the
    first word of a block; a group whose bitmap crosses a block edge with
    points on both sides. mono: rising values (the rate runs)"""
    kd = (lambda k: MONO[k]) if mono else (lambda k: k)
    rng = np.random.default_rng(41)
    b = Build()
    t = T0
    for r in EDGE_RANGES:
        b.group(_two_spans(rng, t, t + r - 1, 5, kd("int")))
        t += 100_000
    used = sum((r + 31) // 32 + 1 for r in EDGE_RANGES)
    nw = RANK_BLOCK - 1 - used
    b.group(_two_spans(rng, t, t + 32 * nw - 1, 300, kd("float")))   # words [used, 1023), pad 1023
    t += 100_000
    # the pad word that opens a rank block is word 2048, not 1024: the group before it must start at
    # word 1024 (the pad at 1023 ends block 0) and its 1024 * 32 s fill block 1 whole; a pad at 2048
    # is ranked as one at 1024 would be: the first word of a block, its block-local rank 0
    b.group(_two_spans(rng, t, t + 32 * RANK_BLOCK - 1, 300, kd("int")))  # words [1024, 2048), pad 2048
    t += 100_000
    edge = t + 32 * (3 * RANK_BLOCK - (2 * RANK_BLOCK + 1))      # the first second of word 3072
    b.group(_two_spans(rng, t, t + 32 * 2000 - 1, 1500, kd("pos"), extra=(edge - 1, edge)))  # words [2049, 4049)
    return b.done(f"word_edges-{int(mono)}")


@cached
def sparse_words(mono=False):
    """D: three sparse groups of ~3M s (93 750 words each), a few hundred
    points a group: more than 256 rank blocks, so k_grid_scan_blocks carries
    across its rounds; a 2-span interpolating group last. mono: rising values"""
    kd = (lambda k: MONO[k]) if mono else (lambda k: k)
    rng = np.random.default_rng(42)
    b = Build()
    for i, kind in enumerate(("int", "float", "pos")):
        lo = T0 + 1000 * i
        b.group(_two_spans(rng, lo, lo + 3_000_000 - 1, 150, kd(kind)))
    b.group(_two_spans(rng, T0 + 500, T0 + 5000, 40, kd("int")))
    return b.done(f"sparse_words-{int(mono)}")


# ---- E: the wide-range fallback --------------------------------------------------
def _wide(name, hi0, hi2):
    rng = np.random.default_rng(51)
    b = Build()
    for lo, hi in ((10, hi0), (None, None), (5, hi2)):
        if lo is None:
            b.group(_two_spans(rng, T0, T0 + 500, 20))
            continue
        ta = np.array([lo, lo + 100, hi - 50, hi])
        tb = np.array([lo + 50, hi - 20])
        b.group([(ta, wide_ints(rng, 4), KI), (tb, wide_ints(rng, 2), KI)])
    return b.done(name)


@cached
def wide_fallback():
    """E: two groups of a few points over 2^31 s each (their bitmaps together
    pass 2^32 bits) around a small ordinary group"""
    return _wide("wide_fallback", (1 << 31) + 100, (1 << 31) + 500)


@cached
def wide_segmented():
    """E: the largest sum of ranges that still takes the segmented path:
    W = 2^27 - 1 words, pad words included"""
    # groups 0 and 2: nw = 2^26 - 10 each; group 1 (range 501 s): nw = 16; pads: 3
    nw = (1 << 26) - 10
    assert 2 * nw + 16 + 3 == (1 << 27) - 1
    return _wide("wide_segmented", 10 + 32 * nw - 1, 5 + 32 * nw - 1)


@cached
def ordinary():
    """a small batch for the call after a wide one"""
    rng = np.random.default_rng(52)
    b = Build()
    for kind in ("int", "float", "dual"):
        counts, kinds, ts, iv, fv = _small_jittered(rng, 5, _kinds_of(kind, 5), T0)
        b.bulk(counts, kinds, ts, iv, fv, sizes=[5])
    return b.done("ordinary")


# ---- G, outside a tile group ------------------------------------------------------
DEEP_BAD, DEEP_INF = 1, 2


@cached
def deep_errors():
    """G: four 2-span groups; the second holds a 3-byte long and the third +Inf,
    each late in a range of 100 000 s: past the group's first 1024 bitmap words"""
    rng = np.random.default_rng(71)
    b = Build()
    b.group(_two_spans(rng, T0, T0 + 999, 30))
    at_bad = b.group(_two_spans(rng, T0 + 5000, T0 + 104_999, 300, "pos"))
    at_inf = b.group(_two_spans(rng, T0 + 7000, T0 + 106_999, 300, "float"))
    b.group(_two_spans(rng, T0, T0 + 999, 30, "float"))
    c = b.done("deep_errors", bad3=(at_bad[2] + 250,))
    return _with_inf(c, at_inf[2] + 240, (at_bad[2] + 250,))


# ---- F: per-group capacity -------------------------------------------------------
CAP_SHORT, CAP_EXACT = 2, 4  # the groups given capacity T - 1 and T


@cached
def capacity_groups(lazy):
    """F: 6 jittered groups; lazy: group CAP_SHORT also holds a 3-byte long
    whose error index lies below its capacity"""
    rng = np.random.default_rng(61)
    b = Build()
    at = None
    for g, kind in enumerate(("int", "float", "int", "dual", "float", "int")):
        counts, kinds, ts, iv, fv = _small_jittered(rng, 6, _kinds_of(kind, 6), T0 + 100 * g)
        if g == CAP_SHORT:
            at = b.n_points
        b.bulk(counts, kinds, ts, iv, fv, sizes=[6])
    # the second point of the group's first span: an early error index
    return b.done(f"capacity-{int(lazy)}", bad3=(at + 1,) if lazy else ())
