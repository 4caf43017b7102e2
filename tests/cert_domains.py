"""Cases for the direct aligned group on a descriptor that carries
TSDBHIP_DESC_QUALS_PROVEN (test_values_only_domains_cpu.py,
test_values_only_domains.py): the value, time and layout domains of
value_domains.py, time_domains.py and layouts.py, and hand-built rows on the
edges of the launch's own arithmetic, each with what the launch must say of it.

On that descriptor reg_run's CERT instantiation loads no qualifier past each
row's first word, so what keeps a row that is not the launch's from a wrong sum
is dir_fields, dir_key and the bucket test of ds_reg_direct_body
(k_ds_reg.hip:566-588, :883-894), restated here on a SpanSet and a query
(start, end, interval). A span is a member iff

  one row (span s is row s); nc >= 2; one width W in {4, 8} with
  vl - 1 == W nc; W nc < 32768; qo % 8 == 0 and vo % 16 == 0;
  with q0, q1 the row's first two qualifier words, d0 = q0 >> 4 and
  step = (q1 >> 4) - d0: q0 & 15 == W - 1; step >= 1; first = base + d0 > 0;
  first >= start; last = first + (nc - 1) step <= end and <= 2^32 - 1;
  d0 + (nc - 1) step <= 4095;
  with kk = ceil(interval / step): nb = ceil(nc / kk) <= 64 and
  nb <= cap = min(nc, (nc - 1) step // interval + 1)

and the group stands iff every span is a member and all share one
(first, nc, step, q0). `verdict` names every clause that fails.

No input has nb <= 64 and nb > cap: kk step >= interval, so
(nc - 1) step // interval >= (nc - 1) // kk = nb - 1, and nb <= nc as kk >= 1.
The clause is restated all the same, and test_values_only_domains_cpu.py
searches the small inputs for a counter-example.

Every group is seeded and deterministic, built once and cached."""
from collections import namedtuple

import numpy as np

import time_domains as td
import value_domains as vd
from helpers import T0, corrupt_qual
from opentsdb_amd import packing, synth
from value_domains import Group

U32MAX, P32 = td.U32MAX, td.P32
WAVE = 64  # a span's buckets: a lane each

SUM, MIN, MAX, AVG, DEV = range(5)
PAIRS16 = [(agg, dsa) for agg in (SUM, MIN, MAX, AVG) for dsa in (SUM, MIN, MAX, AVG)]
PAIRS4 = [(SUM, AVG), (MIN, SUM), (MAX, MIN), (AVG, MAX)]

# the clauses, in the order the kernel meets them
ONE_ROW, CELLS, WIDTH, SHORT, ALIGNED = "one row", "nc >= 2", "one width of 4 or 8", "W nc < 32768", "qo % 8, vo % 16"
FLAGS, STEP, FIRST0, START, END, U32, DELTA = ("flags == W - 1", "step >= 1", "first > 0", "first >= start",
                                               "last <= end", "last <= 2^32 - 1", "last delta <= 4095")
BUCKETS, CAP, CLASS = "nb <= 64", "nb <= cap", "one class"


# ---- the restatement ----

def _word(ss, off):
    return (int(ss.qual_bytes[off]) << 8) | int(ss.qual_bytes[off + 1])


def span_fields(ss, s):
    """(base, d0, step, nc, W, first, last) of a one-row span of one width"""
    nc, vl = int(ss.row_ncells[s]), int(ss.row_val_len[s])
    W = (vl - 1) // nc
    qo = int(ss.row_qual_off[s])
    q0, q1 = _word(ss, qo), _word(ss, qo + 2)
    d0, base = q0 >> 4, int(ss.row_base[s])
    step = (q1 >> 4) - d0
    return base, d0, step, nc, W, base + d0, base + d0 + (nc - 1) * step


def buckets(nc, step, interval):
    """(kk, nb, cap) of ds_reg_direct_body"""
    kk = -(-interval // step)
    return kk, -(-nc // kk), min(nc, (nc - 1) * step // interval + 1)


def span_refusals(ss, s, start, end, interval):
    """(the clauses span s fails, its class key or None). dir_fields' clauses
    come first: a row that fails one has no first word to speak of."""
    if int(ss.span_row_start[s]) != s or int(ss.span_row_start[s + 1]) != s + 1:
        return [ONE_ROW], None
    nc, vl = int(ss.row_ncells[s]), int(ss.row_val_len[s])
    if nc < 2:
        return [CELLS], None
    W = (vl - 1) // nc
    if vl == 0 or W not in (4, 8) or vl - 1 != W * nc:
        return [WIDTH], None
    bad = []
    if W * nc >= 32768:
        bad.append(SHORT)
    if int(ss.row_qual_off[s]) % 8 or int(ss.row_val_off[s]) % 16:
        bad.append(ALIGNED)
    if bad:
        return bad, None
    base, d0, step, nc, W, first, last = span_fields(ss, s)
    q0 = _word(ss, int(ss.row_qual_off[s]))
    for clause, ok in ((FLAGS, (q0 & 15) == W - 1), (STEP, step >= 1), (FIRST0, first > 0), (START, first >= start),
                       (END, last <= end), (U32, last <= U32MAX), (DELTA, d0 + (nc - 1) * step <= 4095)):
        if not ok:
            bad.append(clause)
    if bad:
        return bad, None
    kk, nb, cap = buckets(nc, step, interval)
    if nb > WAVE:
        bad.append(BUCKETS)
    if nb > cap:
        bad.append(CAP)
    return bad, (first, nc, step, q0)


def verdict(ss, start, end, interval):
    """{clause: [spans that fail it]}: empty iff the launch stands (the call is
    taken). CLASS: every span a member, more than one key among them."""
    assert ss.n_rows == ss.n_spans and interval > 0  # (group_direct_q, api.hip: else no launch at all)
    out, keys = {}, set()
    for s in range(ss.n_spans):
        bad, key = span_refusals(ss, s, start, end, interval)
        for clause in bad:
            out.setdefault(clause, []).append(s)
        if not bad:
            keys.add(key)
    if len(keys) > 1:
        out[CLASS] = sorted(keys)
    return out


def member(ss, start=0, end=U32MAX, interval=60):
    return not verdict(ss, start, end, interval)


# ---- items 1 and 2: the value and the time pools ----

VALUE_POOLS = ("WRAP64", "NEG", "INT32_EDGE")
VALUE_INTERVALS = {1: (60, 10), 2: (60, 19)}  # (19 at step 2: no multiple of the step; 10 cells a bucket, 60 buckets)
VALUE_RUNS = (1, 8)
TIME_POOLS = ("T31", "T31B", "TOP", "EPOCH")
STEPS = (1, 2)


def spans_of_run(run):
    return 8 * run + 3


def refused_time_groups():
    """{name: (group, end, the one clause that refuses it, the span)}: proven
    rows (test_values_only_domains_cpu.py), so tsdbhip_desc_certify flags them"""
    p = td.past32_one_row()
    return {
        "EPOCH0-1": (td.one_row("EPOCH0", 1), U32MAX, [FIRST0], None),
        "EPOCH0-2": (td.one_row("EPOCH0", 2), U32MAX, [FIRST0], None),
        # (end 2^32 - 1: both clauses on `last`; end 2^40: `last <= 2^32 - 1` decides alone)
        "PAST32": (p, U32MAX, [END, U32], 35),
        "PAST32-end-2^40": (p, 1 << 40, [U32], 35),
        # (every span to 2^32: one class, so nothing but `last <= 2^32 - 1` stands between the group and the path)
        "PAST32-every-span-end-2^40": (rows(600, 1, d0=1097, base=td.TOP), 1 << 40, [U32], None),
    }


def twin_last_cell(ss, span=None):
    """`ss` with the lowest bit of one span's last cell flipped: a cell of the
    row's last chunk, which a dropped tail would lose"""
    s = ss.n_spans // 2 if span is None else span
    _, _, _, nc, W, _, _ = span_fields(ss, s)
    vb = ss.val_bytes.copy()
    vb[int(ss.row_val_off[s]) + W * nc - 1] ^= 1
    return packing.SpanSet(ss.span_row_start, ss.row_base, ss.row_ncells, ss.row_qual_off, ss.row_val_off,
                           ss.row_val_len, ss.qual_bytes, vb)


# ---- item 3: windows ----

WINDOW_GROUPS = (("T31", 2), ("TOP", 1))
WINDOW_INTERVAL = 60
WINDOW_PAIRS = ((AVG, SUM), (MAX, MAX))


# ---- item 4: row geometry ----

_CACHE = {}
GEOMETRY_SPANS = 9


def _row(base, d0, step, nc, W, seed):
    rng = np.random.default_rng(seed)
    if W == 8:  # longs of the whole range: sums of them wrap
        vals = [int(v) for v in rng.integers(vd.INT64_MIN, vd.INT64_MAX, nc, endpoint=True)]
    else:       # 4-byte cells of either sign: beyond a short, inside an int
        mag = rng.integers(32769, vd.INT32_MAX, nc, endpoint=True)
        vals = [int(m) if sg else -int(m) - 1 for m, sg in zip(mag, rng.integers(0, 2, nc))]
    ts = [base + d0 + step * i for i in range(nc)]
    kv = synth.compact_cells(base, synth.points_int(ts, vals, minimal=(W == 4)))
    assert len(kv.value) == W * nc + (1 if nc > 1 else 0)
    return kv


def rows(nc, step, d0=0, W=8, one_cell_span=None, base=T0):
    """GEOMETRY_SPANS spans of one row of nc cells of W bytes at deltas d0,
    d0 + step, ... of the row at `base` (a row's qualifier holds deltas to
    4095: past the hour, so not series_rows'). one_cell_span: that span's row
    holds one cell (no meta byte), a proven row that is no member."""
    key = ("rows", nc, step, d0, W, one_cell_span, base)
    if key not in _CACHE:
        spans = [[_row(base, d0, step, 1 if s == one_cell_span else nc, W, [41, nc, step, d0, W, s])]
                 for s in range(GEOMETRY_SPANS)]
        _CACHE[key] = Group.from_spans("GEOMETRY", "rows", spans, nc=nc, step=step, d0=d0, W=W, one=one_cell_span,
                                       base=base)
    return _CACHE[key]


# name -> (group, intervals, the clauses that refuse it ([]: taken))
GEOMETRY = {
    "step7-last-delta-4095": (lambda: rows(586, 7), (70,), []),
    "4096x4-64-buckets": (lambda: rows(4096, 1, W=4), (64,), []),          # 8 full chunks, 16384 value bytes
    "4095x8-32760-bytes": (lambda: rows(4095, 1), (64,), []),
    "4096x8-32768-bytes": (lambda: rows(4096, 1), (100,), [SHORT]),        # test_fell_back_short_index_overflow's row
    "3600x8-the-workload": (lambda: rows(3600, 1), (60,), []),             # seven chunks and a 16-cell tail
    "1280-64-buckets": (lambda: rows(1280, 1), (20,), []),
    "1281-65-buckets": (lambda: rows(1281, 1), (20,), [BUCKETS]),
    "64-cells-a-bucket-each": (lambda: rows(64, 2), (1,), []),
    "65-cells-a-bucket-each": (lambda: rows(65, 2), (1,), [BUCKETS]),
    "step3-d0": (lambda: rows(600, 3), (60, 600), []),
    "step3-d5": (lambda: rows(600, 3, d0=5), (60, 600), []),
    "step60-d0": (lambda: rows(60, 60), (60, 600), []),
    "step60-d5": (lambda: rows(60, 60, d0=5), (60, 600), []),
    "step7-one-cell-row": (lambda: rows(586, 7, one_cell_span=4), (70,), [CELLS]),
}


# ---- item 5: layouts ----

LAYOUT_POOLS = ("WRAP64", "INT32_EDGE")
LAYOUT_RUNS = (1, 4)
PACK_SOURCES = ("compact", "mixed")


def layout_leads(name):
    return (0, 10) if name == "compact" else (0,)


# ---- item 6: ranks ----

def rank_groups():
    return [vd.one_row(p, 2) for p in VALUE_POOLS] + [td.one_row(p, 2) for p in ("T31", "TOP")]


# ---- item 7: a false promise everywhere but the direct launch ----

INERT_POOLS = ("WRAP64", "INT32_EDGE")
INERT_SPAN, INERT_CELL = 20, 300  # (cell 300 at step 2 heads a 60-s bucket: the bucket moves with it)
BATCH_CUT = [0, 9, 35, 70]

Query = namedtuple("Query", "what options agg rate interval dsa exact S", defaults=(False, 70))


def inert_group(pool, S=70):
    return vd.one_row(pool, 2, S=S)


def corrupted(ss):
    return corrupt_qual(ss, INERT_SPAN, INERT_CELL, lambda q: q + 16)


def inert_queries():
    """one-context queries: (what, options, agg, rate, interval, ds_agg, exact, S)"""
    ls, off = {"lockstep": ("always", "on")}, {"group_direct": ("off", "on")}
    qs = [Query("lockstep sum", ls, SUM, False, 0, 0), Query("lockstep max", ls, MAX, False, 0, 0),
          Query("lockstep sum rate", ls, SUM, True, 0, 0),
          Query("k_ug_dev", ls, DEV, False, 0, 0, S=100)]
    for agg, dsa in ((AVG, SUM), (MIN, MAX)):
        qs.append(Query("aligned group", off, agg, False, 60, dsa))
        qs.append(Query("aligned group exact", off, agg, False, 60, dsa, exact=True))
    for dec in ("general", "fast", "chunks", "spans", "direct"):
        o = {"decode": (dec, "auto")}
        qs += [Query(f"decode {dec}", o, SUM, False, 0, 0), Query(f"decode {dec}", o, AVG, False, 60, SUM)]
    return qs


BATCH_QUERIES = [(SUM, False, 0, 0), (MAX, True, 0, 0), (AVG, False, 60, SUM), (MIN, False, 60, MAX)]
RANK_QUERIES = [(SUM, False, 0, 0), (AVG, False, 60, SUM), (MAX, False, 60, MIN)]
