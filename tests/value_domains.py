"""Value pools and path-shaped groups for the value-domain tests
(test_value_domains_cpu.py, test_value_domains.py): extreme longs, negative
and boundary-width cells, signed zeros, denormals, NaN and overflowing
doubles, laid out so that a group takes one of the streaming paths (`one_row`:
one hourly row a span on one cadence) or the general path (`jittered`). Every
pool is seeded and deterministic; a Group is built once and cached."""
import struct

import numpy as np

from helpers import F, I, T0
from opentsdb_amd import packing

INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
NAN = float("nan")

INT_POOLS = ("WRAP64", "NEG", "INT32_EDGE", "WIDTHS")
FLOAT_POOLS = ("ZEROS", "DENORM", "NAN_LATER", "NAN_FIRST", "NAN_BUCKET", "HUGE")
POOLS = INT_POOLS + FLOAT_POOLS + ("BIG_MIXED",)

WRAP64_EDGES = [INT64_MIN, INT64_MIN + 1, INT64_MAX, INT64_MAX - 1, 1 << 62, -(1 << 62), -1, 0, 1,
                (1 << 53) + 1, -((1 << 53) + 1), (1 << 53) + 3, -((1 << 53) + 3)]
INT32_EDGES = [INT32_MIN, INT32_MIN + 1, INT32_MAX, 32769, -32769, 1 << 30, -(1 << 30)]
WIDTH_EDGES = [-129, -128, 127, 128, -32769, -32768, 32767, 32768, INT32_MIN - 1, INT32_MIN, INT32_MAX,
               INT32_MAX + 1]


def _f32(bits):
    return struct.unpack(">f", struct.pack(">I", bits))[0]


DENORM_F4 = [_f32(0x00000001), _f32(0x007FFFFF), _f32(0x80000001), _f32(0x00800000)]
DENORM_F8 = [5e-324, 2.2250738585072014e-308, -5e-324, -2.2250738585072014e-308]
HUGE_F8, HUGE_F4 = 1.7e308, float(np.float32(3.4e38))

# how a pool's spans are written: 8-byte longs (IncomingDataPoints), minimal-
# width longs (TSDB.addPoint), float32, float64; "mix": float32 / float64 by span
I8, IM, F4, F8 = "i8", "im", "f4", "f8"


def wrap(x):
    x &= (1 << 64) - 1
    return x - (1 << 64) if x >> 63 else x


def _seed(pool, *more):
    return [POOLS.index(pool) + 1] + [int(m) for m in more]


def _wrap64(rng, n):
    edge = rng.random(n) < 0.6
    pick = rng.integers(0, len(WRAP64_EDGES), n)
    uni = rng.integers(INT64_MIN, INT64_MAX, n, endpoint=True)
    return [WRAP64_EDGES[int(p)] if e else int(u) for e, p, u in zip(edge, pick, uni)]


def _finite(rng, n):
    """positive values a float32 holds exactly (so both widths carry the same numbers)"""
    return [float(v) for v in (50.0 + 100.0 * rng.random(n)).astype(np.float32)]


def nan_cells(n):
    """(k0, later): the cell NAN_FIRST / HUGE / NAN_BUCKET's head use, a bucket
    head for 5, 10, 30 and 60 cells a bucket at the default size and in the
    second half, and the later cells of NAN_LATER (after k0)"""
    k0 = 360 if n >= 420 else 3 * n // 5
    later = sorted({min(n - 2, k0 + 1 + int((n - k0 - 2) * f)) for f in (0.3, 0.65, 0.97)})
    return k0, later


def nan_spans(S):
    """the spans that carry NAN_LATER's NaNs: never span 0"""
    return sorted({1, S // 2, S - 1} - {0}) if S > 1 else []


def _values(pool, s, S, n, kind, rng):
    """the n values of span s of S (cell order) and how they are written"""
    if pool == "WRAP64":
        return I8, _wrap64(rng, n)
    if pool == "NEG":
        # every value of [-1000, -1]: shuffled runs of the whole range
        reps = (n + 999) // 1000
        v = np.concatenate([rng.permutation(1000) for _ in range(reps)])[:n]
        return kind or I8, [-1 - int(x) for x in v]
    if pool == "INT32_EDGE":
        edge = rng.random(n) < 0.3
        pick = rng.integers(0, len(INT32_EDGES), n)
        mag = rng.integers(32769, INT32_MAX, n, endpoint=True)
        sign = rng.integers(0, 2, n)
        return IM, [INT32_EDGES[int(p)] if e else (int(m) if sg else -int(m))
                    for e, p, m, sg in zip(edge, pick, mag, sign)]
    if pool == "WIDTHS":
        return IM, [WIDTH_EDGES[int(p)] for p in rng.integers(0, len(WIDTH_EDGES), n)]
    fk = kind if kind in (F4, F8) else (F4 if s % 2 else F8)
    if pool == "ZEROS":
        # the sign by span (all 0.0, all -0.0) and by cell (every third span, span 0 among them)
        if s % 3 == 0:
            return fk, [-0.0 if b else 0.0 for b in rng.integers(0, 2, n)]
        return fk, [0.0 if s % 3 == 1 else -0.0] * n
    if pool == "DENORM":
        table = DENORM_F4 if fk == F4 else DENORM_F8
        return fk, [table[int(p)] for p in rng.integers(0, 4, n)]
    v = _finite(rng, n)
    k0, later = nan_cells(n)
    if pool in ("NAN_LATER", "NAN_FIRST"):
        if s in nan_spans(S):
            for c in later[nan_spans(S).index(s) % len(later):]:
                v[c] = NAN
        if pool == "NAN_FIRST" and s == 0:
            v[k0] = NAN
        return fk, v
    if pool == "NAN_BUCKET":
        if S > 2 and s == 2:
            v[k0] = NAN  # the first cell of its bucket
        if s == min(5, S - 1):
            v[k0 + 61 if k0 + 61 < n else k0 + 1] = NAN  # a later cell of its bucket
        return fk, v
    if pool == "HUGE":
        if s <= S // 2:
            v[k0] = HUGE_F4 if fk == F4 else HUGE_F8
        return fk, v
    raise KeyError(pool)


class Group:
    """series: [(kind, [(ts, value)])] in span order; or (from_spans) the
    spans' KeyValue rows as they are, with no series behind them"""

    def __init__(self, pool, shape, series, spans=None, **meta):
        self.pool, self.shape, self.series, self.meta = pool, shape, series, meta
        self.spans = spans if spans is not None else [
            I(pts, minimal=False) if k == I8 else I(pts) if k == IM else F(pts, double=(k == F8)) for k, pts in series]
        self.ss = packing.pack_spans(self.spans)
        flags = {kv.qualifier[i + 1] & 0xF for rows in self.spans for kv in rows for i in range(0, len(kv.qualifier), 2)}
        # one row a span and one cell type and width: what the uniform paths' class key asks for
        self.one_class = len(flags) == 1 and all(len(rows) == 1 for rows in self.spans)
        self.is_float = any(f & 8 for f in flags) if series is None else any(k in (F4, F8) for k, _ in series)
        self.n_spans = len(self.spans)
        self.key = (pool, shape) + tuple(sorted(meta.items(), key=str))
        self._abs = None

    def abs(self):
        """the same group over |value|, longs as float64 cells (sums of them
        must not wrap): the aggregate over it bounds the sum of |terms| a
        double result is rounded against (assert_same's abs_scale)"""
        assert self.series is not None, "a group made from rows has no |value| twin"
        if self._abs is None:
            self._abs = Group(self.pool, self.shape,
                              [(k if k == F4 else F8, [(t, abs(float(v))) for t, v in pts]) for k, pts in self.series],
                              abs_of=self.key)
        return self._abs

    @classmethod
    def from_spans(cls, pool, shape, spans, **meta):
        return cls(pool, shape, None, spans=spans, **meta)

    def values(self, cell):
        """the spans' values at one cell (one_row)"""
        return [pts[cell][1] for _, pts in self.series]


_CACHE = {}


def one_row(pool, step=1, S=70, n=600, kind=None):
    """S spans of one hourly row each, n cells on one cadence from T0. The
    default size crosses the 64-lane wave and the 512-cell chunk."""
    key = ("one_row", pool, step, S, n, kind)
    if key in _CACHE:
        return _CACHE[key]
    assert step in (1, 2) and n * step <= 3600
    ts = [T0 + step * i for i in range(n)]
    series = []
    if pool == "BIG_MIXED":
        for s in range(S):
            rng = np.random.default_rng(_seed(pool, s, n, step))
            if s == S // 2:
                series.append((F8, list(zip(ts, [float(x) for x in 1e18 * rng.standard_normal(n)]))))
            else:
                series.append((I8, list(zip(ts, _wrap64(rng, n)))))
    else:
        for s in range(S):
            k, v = _values(pool, s, S, n, kind, np.random.default_rng(_seed(pool, s, n, step)))
            if pool == "WRAP64" and n > 6:
                # one grid point of Long.MIN_VALUE / Long.MAX_VALUE alternating by span: its population
                # deviation is 2^63 for two spans, and the sum of a pair wraps to -1
                v[5] = INT64_MAX if s % 2 else INT64_MIN
            series.append((k, list(zip(ts, v))))
    k0, later = nan_cells(n)
    g = Group(pool, "one_row", series, step=step, n=n, k0=k0, later=tuple(later), S=S, kind=kind)
    _CACHE[key] = g
    return g


def jittered(pool, kind=None):
    """12 spans of about 60 points with gaps from U{1..700}: the general path,
    the long lerp's wrapping product and every cell width. Span 0 starts first
    and ends last, so it is the first active span at every grid point."""
    key = ("jittered", pool, kind)
    if key in _CACHE:
        return _CACHE[key]
    S = 12
    trng = np.random.default_rng(_seed(pool, 999))
    tss = []
    for s in range(S):
        n = int(trng.integers(45, 76))
        start = T0 if s == 0 else T0 + 800 + int(trng.integers(0, 2000))
        gaps = trng.integers(1, 701, n)
        tss.append([int(t) for t in start + np.cumsum(gaps) - gaps[0]])
    last = max(t[-1] for t in tss[1:])
    while tss[0][-1] <= last + 800:
        tss[0].append(tss[0][-1] + int(trng.integers(1, 701)))
    series = []
    for s in range(S):
        n = len(tss[s])
        rng = np.random.default_rng(_seed(pool, s, 7))
        if pool == "BIG_MIXED":
            if s == 0:
                k, v = F8, [float(x) for x in 1e18 * rng.standard_normal(n)]
            else:
                k, v = I8, _wrap64(rng, n)
        else:
            k, v = _values(pool, s, S, n, kind, rng)
            if k == I8:
                k = IM  # (minimal widths: -1, 0 and 1 take a byte, the rest of WRAP64 eight)
        series.append((k, list(zip(tss[s], v))))
    g = Group(pool, "jittered", series, kind=kind)
    _CACHE[key] = g
    return g


def nan_at(cells, step=2, kind=F8, S=70, n=600):
    """one_row of finite positive floats with a NaN at each (span, cell) of `cells`"""
    key = ("nan_at", tuple(cells), step, kind, S, n)
    if key not in _CACHE:
        ts = [T0 + step * i for i in range(n)]
        series = []
        for s in range(S):
            v = _finite(np.random.default_rng(_seed("NAN_LATER", s, n, step, 5)), n)
            for sp, c in cells:
                if sp == s:
                    v[c] = NAN
            series.append((kind, list(zip(ts, v))))
        _CACHE[key] = Group("NAN_AT", "one_row", series, step=step, n=n, cells=tuple(cells), S=S, kind=kind)
    return _CACHE[key]


def cells_per_bucket(interval, step):
    """greedy downsampling over a constant cadence: ceil(interval / step) cells a bucket"""
    return (interval + step - 1) // step
