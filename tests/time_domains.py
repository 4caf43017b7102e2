"""Time pools for the time-domain tests (test_time_domains_cpu.py,
test_time_domains.py): the groups of tests/value_domains.py's shapes with
plain values (random longs in +-2^40 at 8 bytes, float64 where asked) and a
time axis laid over a boundary: 2^31 inside a row (T31), the last cell at
2^32 - 1 (TOP, TOP_ROWS), the first cell at timestamp 1 (EPOCH) or 0 (EPOCH0),
lerp brackets up to 2^32 - 2 wide (WIDE), cells at or beyond 2^32 (PAST32),
qualifier deltas past the hour (ROW_EDGE). A pool's group at base B and its
twin at T0 hold the same deltas and the same values: results shift by B - T0.
Every pool is seeded and deterministic; a group is built once and cached."""
import numpy as np

from helpers import T0, corrupt_qual
from opentsdb_amd import synth
from value_domains import F8, I8, IM, Group

B31 = 2147482800          # the hourly row that holds 2^31
P31 = 1 << 31             # = B31 + 848
TOP = 4294965600          # the last hourly row base below 2^32 (1193046 x 3600)
U32MAX = TOP + 1695       # = 2^32 - 1
P32 = 1 << 32
assert B31 % 3600 == 0 and B31 + 848 == P31 and TOP % 3600 == 0 and U32MAX == P32 - 1 and TOP + 3600 > U32MAX

# row-key base times for the scans of test_find_spans.py and test_groupby_plan.py: 0, either side of
# 2^31 (0x7FFF.. and 0x8000..) and the last hourly row below 2^32
EDGE_BASES = [0, B31 - 3600, B31 + 3600, TOP]

INTERVALS = [1, 13, 60, 1695, 1696, 3599, 3600, 3601, 4095, 4096, 65536, 1 << 24, P31 - 1]

# one_row: pool -> (row base, {step: first delta}). T31 puts 2^31 at cell 300;
# T31B in the second 512-cell chunk at step 1 (cell 520) and as far in as the
# row allows at step 2 (2^31 is 848 s into its row: cell 424 with a first delta
# of 0). TOP ends on 2^32 - 1. EPOCH starts at timestamp 1.
ONE_ROW = {
    "T31": (B31, {1: 848 - 300, 2: 848 - 600}),
    "T31B": (B31, {1: 848 - 520, 2: 0}),
    "TOP": (TOP, {1: 1096, 2: 497}),
    "EPOCH": (0, {1: 1, 2: 1}),
    "EPOCH0": (0, {1: 0, 2: 0}),  # (fails: see epoch0 below)
}
P31_CELL = {("T31", 1): 300, ("T31", 2): 300, ("T31B", 1): 520, ("T31B", 2): 424}
POOLS = ("T31", "T31B", "TOP", "EPOCH")

_CACHE = {}


def _longs(rng, n):
    return [int(v) for v in rng.integers(-(1 << 40), 1 << 40, n, endpoint=True)]


def _vals(kind, seed, n):
    rng = np.random.default_rng(seed)
    if kind == F8:
        return [float(v) for v in 1e3 * rng.standard_normal(n)]
    if kind == "i1":  # one-byte longs: a seek inside a row shifts nothing (quirk Q1)
        return [int(v) for v in rng.integers(-128, 127, n, endpoint=True)]
    return _longs(rng, n)


def _group(pool, shape, series, **meta):
    series = [(IM if k == "i1" else k, pts) for k, pts in series]
    return Group(pool, shape, series, **meta)


def one_row(pool, step=1, S=70, n=600, kind=I8, at_t0=False):
    """S spans of one hourly row each, n cells on one cadence: the pool's row
    and first delta, or (at_t0) the same deltas and values in T0's row"""
    key = ("one_row", pool, step, S, n, kind, at_t0)
    if key not in _CACHE:
        base, d0 = ONE_ROW[pool]
        d0 = d0[step]
        assert step in (1, 2) and d0 >= 0 and d0 + step * (n - 1) < 3600
        b = T0 if at_t0 else base
        ts = [b + d0 + step * i for i in range(n)]
        series = [(kind, list(zip(ts, _vals(kind, [11, s, n, step], n)))) for s in range(S)]
        _CACHE[key] = _group(pool, "one_row", series, step=step, n=n, S=S, kind=kind, base=b, d0=d0, at_t0=at_t0)
    return _CACHE[key]


def _jitter_offsets():
    """12 spans of 45..75 points with gaps from U{1..700}; span 0 starts first
    and ends last. Offsets from 0; the last offset of all is span 0's."""
    rng = np.random.default_rng([12, 999])
    offs = []
    for s in range(12):
        n = int(rng.integers(45, 76))
        start = 0 if s == 0 else 800 + int(rng.integers(0, 2000))
        gaps = rng.integers(1, 701, n)
        offs.append([int(t) for t in start + np.cumsum(gaps) - gaps[0]])
    last = max(o[-1] for o in offs[1:])
    while offs[0][-1] <= last + 800:
        offs[0].append(offs[0][-1] + int(rng.integers(1, 701)))
    return offs


def jitter_base(pool):
    """(base, d0): hour-aligned base and the delta added to every offset. TOP:
    the last point of all is 2^32 - 1. T31: 2^31 about the middle. EPOCH: the
    first point at timestamp 1."""
    offs = _jitter_offsets()
    hi = offs[0][-1]
    if pool == "TOP":
        d0 = (1695 - hi) % 3600
        return TOP - (hi + d0 - 1695), d0
    if pool in ("T31", "T31B"):
        return B31 - 3600 * ((hi // 2) // 3600), 0
    if pool == "EPOCH":
        return 0, 1
    raise KeyError(pool)


def jittered(pool, kind=IM, at_t0=False):
    """the general path: 12 spans of about 60 points, minimal-width longs (or
    float64)"""
    key = ("jittered", pool, kind, at_t0)
    if key not in _CACHE:
        base, d0 = jitter_base(pool)
        assert base % 3600 == 0
        b = T0 if at_t0 else base
        series = []
        for s, o in enumerate(_jitter_offsets()):
            series.append((kind, list(zip([b + d0 + t for t in o], _vals(kind, [13, s], len(o))))))
        _CACHE[key] = _group(pool, "jittered", series, kind=kind, base=b, d0=d0, at_t0=at_t0)
    return _CACHE[key]


def top_rows(S=70, merge=False, kind=I8, at_t0=False):
    """TOP_ROWS: spans of three hourly rows at step 10 that end in the TOP row,
    360 cells in each of the first two and 170 in the last (deltas 5..1695: the
    last cell is 2^32 - 1). merge: span S // 2 ends 495 s into its last hour, so
    that row merges into its predecessor's RowSeq (Span.java:117: last -
    base < 4096) and the group is no longer of one class."""
    key = ("top_rows", S, merge, kind, at_t0)
    if key not in _CACHE:
        b = (T0 if at_t0 else TOP - 7200)
        n = 360 + 360 + 170
        ts = [b + 5 + 10 * i for i in range(n)]
        assert at_t0 or ts[-1] == U32MAX
        series = []
        for s in range(S):
            m = 720 + 50 if merge and s == S // 2 else n  # (last cell 7200 + 495)
            series.append((kind, list(zip(ts[:m], _vals(kind, [14, s], n)[:m]))))
        _CACHE[key] = _group("TOP_ROWS", "rows3", series, step=10, n=n, S=S, kind=kind, base=b, merge=merge,
                             at_t0=at_t0)
    return _CACHE[key]


def twin(g):
    """the same deltas and values in T0's rows"""
    m = g.meta
    if g.shape == "one_row":
        return one_row(g.pool, m["step"], m["S"], m["n"], m["kind"], at_t0=True)
    if g.shape == "jittered":
        return jittered(g.pool, m["kind"], at_t0=True)
    return top_rows(m["S"], m["merge"], m["kind"], at_t0=True)


def shift(g):
    return g.meta["base"] - T0


# ---- EPOCH0: a span whose first cell is at timestamp 0 ----
def _pts(ts):
    return list(zip(ts, range(1, len(ts) + 1)))


EPOCH0_CASES = {
    "span0": [[0, 5], [3, 9]],
    "later": [[3, 9], [0, 5]],
    "only": [[0, 5]],
    "none": [[1, 5], [3, 9]],  # (the control: the epoch's neighbour)
}


def epoch0(case):
    key = ("epoch0", case)
    if key not in _CACHE:
        _CACHE[key] = _group("EPOCH0", case, [(IM, _pts(ts)) for ts in EPOCH0_CASES[case]])
    return _CACHE[key]


# ---- WIDE: lerp brackets up to 2^32 - 2 ----
WIDE_X1 = [P31, P31 + 1, U32MAX - 1, U32MAX]


def wide(x1):
    """span 0: (1, -2^50) and (x1, 2^50 + 12345); span 1: 1099 points 3600 x 997
    apart from 3600 x 997 + 5 (each in an hourly row of its own). The union grid
    spans [1, x1]: a bitmap of up to 2^32 bits."""
    key = ("wide", x1)
    if key not in _CACHE:
        a = [(1, -(1 << 50)), (x1, (1 << 50) + 12345)]
        rng = np.random.default_rng([15])
        b = list(zip([3600 * 997 * i + 5 for i in range(1, 1100)], _longs(rng, 1099)))
        assert b[-1][0] < P31 * 2
        _CACHE[key] = _group("WIDE", "wide", [(IM, a), (IM, b)], x1=x1)
    return _CACHE[key]


# ---- PAST32: cells at or beyond 2^32 ----
def past32(second):
    """a span of 60 cells in the TOP row at deltas 1799 - 30 i (the last four at
    or beyond 2^32), alone or before a second span inside the row's legal part"""
    key = ("past32", second)
    if key not in _CACHE:
        ts = [TOP + 1799 - 30 * i for i in range(59, -1, -1)]
        series = [(I8, list(zip(ts, _vals(I8, [16, 0], 60))))]
        if second:
            # (to 2^32 - 1: its grid points between span 0's cells at deltas 1679 and 1709 ask
            # span 0 for a lerp towards a cell beyond 2^32)
            ts2 = [TOP + 15 + 28 * i for i in range(61)]
            series.append((I8, list(zip(ts2, _vals(I8, [16, 1], 61)))))
        _CACHE[key] = _group("PAST32", "second" if second else "alone", series, second=second)
    return _CACHE[key]


def past32_one_row(S=70, n=600):
    """a one_row group (step 1 from TOP + 1096) whose span S // 2 runs one cell
    further: to 2^32"""
    key = ("past32_one_row", S, n)
    if key not in _CACHE:
        series = []
        for s in range(S):
            m = n + (1 if s == S // 2 else 0)
            ts = [TOP + 1096 + i for i in range(m)]
            series.append((I8, list(zip(ts, _vals(I8, [17, s], m)))))
        _CACHE[key] = _group("PAST32", "one_row", series, S=S, n=n)
    return _CACHE[key]


def past32_inner(which):
    """a cell beyond 2^32 that is not its row's last: an inner qualifier of a
    TOP row rewritten to a delta above 1695 (the row's cells are then out of
    order, and its last cell is still 2^32 - 1 or below).
    "one_row": cell 300 of span 2 of three one_row spans (the thread-per-span
    assembly), behind a span a month earlier: the union grid's bitmap is then
    more than 8 slices of 2^18 s, the layout whose slice index a timestamp
    wrapped to 32 bits would turn negative. "rows": cell 1 of the last row of
    jittered TOP's span 0 (a span of many rows: the wave walks)."""
    key = ("past32_inner", which)
    if key not in _CACHE:
        if which == "one_row":
            early = [TOP - 31 * 86400 + 600 * i for i in range(50)]
            g = _group("PAST32", "inner_one_row",
                       [(I8, list(zip(early, _vals(I8, [19, 0], 50))))] + one_row("TOP", 1, S=3).series)
            span, row, cell, delta = 2, 0, 300, 1700
        else:
            j = jittered("TOP")
            g = _group("PAST32", "inner_rows", j.series)
            span, row, cell, delta = 0, len(j.spans[0]) - 1, 1, 1800
        kv = g.spans[span][row]
        assert kv.base_time == TOP and len(kv.qualifier) // 2 >= cell + 2
        g.ss = corrupt_qual(g.ss, span, cell, lambda q: (delta << 4) | (q & 0xF), row=row)
        g.meta.update(span=span, row=row, cell=cell, delta=delta)
        _CACHE[key] = g
    return _CACHE[key]


# ---- ROW_EDGE: qualifier deltas past the hour ----
# (last delta of row 1, where row 2 starts): row 2 is the next hourly row, so it cannot start
# before delta 3600 of row 1
ROW_EDGE_CASES = [(3599, "after"), (3600, "at"), (3600, "after"), (4095, "before"), (4095, "at"), (4095, "after")]


def _row(base, deltas, seed):
    vals = _vals("i1", seed, len(deltas))
    return synth.compact_cells(base, [(base + d,) + synth.encode_long(v) for d, v in zip(deltas, vals)])


def row_edge(base, last, nxt):
    """three spans of two hourly rows. Row 1 of each: 40 cells up to delta
    `last` (RowSeq's qualifier holds 12 bits of delta; the write path never
    makes more than 3599). Row 2 (base + 3600) starts before, at or after row
    1's last cell: its own last cell decides between RowSeq.addRow (last - base
    < 4096: span 0 while its row can end at delta 495, ignored when it starts at
    or before the last cell) and a new RowSeq (spans 1 and 2: dropped when it
    does). Span 2's second row holds one cell."""
    key = ("row_edge", base, last, nxt)
    if key not in _CACHE:
        f2 = last - 3600 + {"before": -1, "at": 0, "after": 1}[nxt]
        assert f2 >= 0
        spans = []
        for s in range(3):
            d1 = sorted({last - 90 * i for i in range(40)})
            if s == 0:
                d2 = [f2 + i for i in range(max(1, min(30, 496 - f2)))]  # ends below 4096 - 3600 if it can
            elif s == 1:
                d2 = [f2 + 100 * i for i in range(30)]                # ends past it: a RowSeq of its own
            else:
                d2 = [f2 + 2000]                                      # one cell (no meta byte)
            spans.append([_row(base, d1, [18, s, 1]), _row(base + 3600, d2, [18, s, 2])])
        _CACHE[key] = Group.from_spans("ROW_EDGE", nxt, spans, base=base, last=last, first2=f2)
    return _CACHE[key]


# ---- windows ----
def windows(g):
    """(start, end) pairs over a one_row group: ends and starts on, one off and
    far off its first cell, an inside cell and its last cell, and the 2^31 /
    2^32 values whatever the group"""
    first, step, n = g.meta["base"] + g.meta["d0"], g.meta["step"], g.meta["n"]
    last = first + step * (n - 1)
    out = []
    for ts in (first, first + step * (n // 2), last):
        out += [(0, e) for e in (ts, ts - 1)]
        out += [(s, U32MAX) for s in (ts, ts + 1)]
        out += [(ts, ts), (ts + 1, ts)]
    out += [(0, e) for e in (P31 - 1, P31, U32MAX, P32, 1 << 40)]
    out += [(U32MAX, U32MAX), (U32MAX, 1 << 40), (P32, 1 << 40), (P31, P32), (first, last), (first + 1, last),
            (first, last - 1)]
    return list(dict.fromkeys(out))
