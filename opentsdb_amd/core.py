"""Host-side mirror of the reference call surface for the aggregation path.

Mirrors (names, argument meaning, error behaviour):
  Aggregators / Aggregator        src/core/Aggregators.java:22-245, Aggregator.java:24-86
  Span (addRow)                   src/core/Span.java:33-132
  SpanGroup (ctor, add, size,
    aggregatedSize, iterator,
    timestamp/isInteger/
    longValue/doubleValue(i))     src/core/SpanGroup.java:46-254
  DataPoint                       src/core/DataPoint.java:20-56
  IllegalDataException            src/core/IllegalDataException.java
  group_by_and_aggregate          TsdbQuery.groupByAndAggregate (TsdbQuery.java:294-363),
                                  SpanCmp (TsdbQuery.java:594-621),
                                  Tags.getValueId (Tags.java:213-227)
  plan_groups_device              the same grouping, and every group's tags, by
                                  tsdbhip_groupby_plan on the GPU
  SpanGroup.getTags /
    getAggregatedTags,
    compute_tags, span_in_range   SpanGroup.java:130-191

The whole SpanGroup is evaluated by libtsdbhip on the GPU on first access
(tsdbhip_spangroup_run); iteration then replays the reference's lazy
exception behaviour: points before the failing one are delivered, then the
mapped exception is raised.
"""
import ctypes as C
import numpy as np

from . import _abi
from ._lib import Context, TsdbHipError
from .packing import KeyValue, SpanSet, pack_spans


class IllegalDataException(Exception):
    """net.opentsdb.core.IllegalDataException"""


class IllegalStateException(Exception):
    """java.lang.IllegalStateException ("Got NaN or Infinity")"""


class ArrayIndexOutOfBoundsException(IndexError):
    """java.lang.ArrayIndexOutOfBoundsException"""


def _exception_for(code, msg):
    if code == _abi.E_ILLEGAL_DATA:
        return IllegalDataException(msg)
    if code == _abi.E_NAN_INF:
        return IllegalStateException(msg)
    if code == _abi.E_EMPTY_SPAN:
        return AssertionError(msg)
    if code == _abi.E_OUT_OF_BOUNDS:
        return ArrayIndexOutOfBoundsException(msg)
    return TsdbHipError(code, msg)


class Aggregator:
    """One of the five stateless aggregators; identity = op code."""

    def __init__(self, name, code):
        self._name = name
        self.code = code

    def toString(self):
        return self._name

    __str__ = toString

    def __repr__(self):
        return f"Aggregator({self._name})"


class Aggregators:
    SUM = Aggregator("sum", _abi.AGG_SUM)
    MIN = Aggregator("min", _abi.AGG_MIN)
    MAX = Aggregator("max", _abi.AGG_MAX)
    AVG = Aggregator("avg", _abi.AGG_AVG)
    DEV = Aggregator("dev", _abi.AGG_DEV)
    _BY_NAME = {"sum": SUM, "min": MIN, "max": MAX, "avg": AVG, "dev": DEV}

    @classmethod
    def get(cls, name):
        try:
            return cls._BY_NAME[name]
        except KeyError:
            raise LookupError("No such aggregator: " + name) from None

    @classmethod
    def set(cls):
        return set(cls._BY_NAME)


class DataPoint:
    __slots__ = ("_ts", "_isint", "_bits")

    def __init__(self, ts, isint, bits):
        self._ts, self._isint, self._bits = int(ts), bool(isint), int(bits)

    def timestamp(self):
        return self._ts

    def isInteger(self):
        return self._isint

    def longValue(self):
        if not self._isint:
            raise TypeError("ClassCastException: value is a double")
        return self._bits

    def doubleValue(self):
        if self._isint:
            raise TypeError("ClassCastException: value is a long")
        return float(np.int64(self._bits).view(np.float64))

    def toDouble(self):
        return float(self._bits) if self._isint else self.doubleValue()

    def __repr__(self):
        v = self._bits if self._isint else self.doubleValue()
        return f"DataPoint({self._ts}, {v!r})"


class Span:
    """The compacted rows of one time series, in scan order. The row
    acceptance rules of Span.addRow are applied by the library."""

    def __init__(self, rows=None, key=None):
        self.rows = list(rows or [])
        self.key = None if key is None else bytes(key)  # the row key (of any of its rows: the base time is ignored)

    def addRow(self, row: KeyValue):
        self.rows.append(row)


def run_spanset(ctx, spanset: SpanSet, start, end, agg, rate=False, ds_interval=0, ds_agg=0,
                exact=False, capacity=None, device_desc=None, sharded=False, span0=0, register_out=False):
    """Low-level: one tsdbhip_spangroup_run. Returns (code, ts, is_int, bits,
    n_input_points, err_index). sharded: this rank's shard of a group whose
    first span has global index span0. register_out: the result buffers
    registered (tsdbhip_host_register, as the JNI bridge registers its
    DirectByteBuffers) for the call."""
    desc = _abi.SgDesc()
    if device_desc is not None:
        C.pointer(desc)[0] = device_desc
    else:
        spanset.fill_desc(desc)
        desc.flags = 0
    desc.start_time, desc.end_time = int(start), int(end)
    desc.rate, desc.agg, desc.ds_agg = int(bool(rate)), int(agg), int(ds_agg)
    desc.ds_interval = int(ds_interval)
    if exact:
        desc.flags |= _abi.EXACT_ORDER
    if sharded:  # this rank's shard; exchange over the ctx communicator
        desc.flags |= _abi.SHARDED
        desc.span0 = int(span0)
    cap = capacity
    if cap is None:
        cap = max(1, spanset.n_cells()) if spanset is not None else 1 << 20
    ts = np.zeros(cap, np.int64)
    isi = np.zeros(cap, np.uint8)
    bits = np.zeros(cap, np.int64)
    out = _abi.SgOut()
    out.capacity = cap
    out.ts = _abi.ptr(ts, C.c_int64)
    out.is_int = _abi.ptr(isi, C.c_uint8)
    out.bits = _abi.ptr(bits, C.c_int64)
    regs = []
    try:
        if register_out:
            for a in (ts, isi, bits):
                ctx.check(ctx._lib.tsdbhip_host_register(ctx.handle, a.ctypes.data_as(C.c_void_p), a.nbytes))
                regs.append(a)
        rc = ctx._lib.tsdbhip_spangroup_run(ctx.handle, C.byref(desc), C.byref(out))
    finally:
        for a in regs:
            ctx._lib.tsdbhip_host_unregister(ctx.handle, a.ctypes.data_as(C.c_void_p))
    n = int(out.n_out)
    return rc, ts[:n], isi[:n], bits[:n], int(out.n_input_points), int(out.err_index)


def run_spanset_batch(ctx, spanset: SpanSet, group_span_start, start, end, agg, rate=False, ds_interval=0,
                      ds_agg=0, exact=False, capacities=None, device_desc=None):
    """Low-level: one tsdbhip_spangroup_run_batch over the groups
    [gss[g], gss[g+1]) of spanset. Returns (code, [per-group tuples as
    run_spanset returns them])."""
    gss = np.ascontiguousarray(group_span_start, np.uint32)
    G = len(gss) - 1
    desc = _abi.SgDesc()
    if device_desc is not None:
        C.pointer(desc)[0] = device_desc
    else:
        spanset.fill_desc(desc)
        desc.flags = 0
    desc.start_time, desc.end_time = int(start), int(end)
    desc.rate, desc.agg, desc.ds_agg = int(bool(rate)), int(agg), int(ds_agg)
    desc.ds_interval = int(ds_interval)
    if exact:
        desc.flags |= _abi.EXACT_ORDER
    if capacities is None:
        cells = np.concatenate([[0], np.cumsum(spanset.row_ncells.astype(np.int64))])
        srs = spanset.span_row_start.astype(np.int64)
        cum = cells[srs]  # cells before span s
        capacities = np.maximum(1, cum[gss[1:].astype(np.int64)] - cum[gss[:-1].astype(np.int64)])
    outs = (_abi.SgOut * max(G, 1))()
    bufs = []
    for g in range(G):
        cap = int(capacities[g])
        ts, isi, bits = np.zeros(cap, np.int64), np.zeros(cap, np.uint8), np.zeros(cap, np.int64)
        bufs.append((ts, isi, bits))
        outs[g].capacity = cap
        outs[g].ts = _abi.ptr(ts, C.c_int64)
        outs[g].is_int = _abi.ptr(isi, C.c_uint8)
        outs[g].bits = _abi.ptr(bits, C.c_int64)
    rc = ctx._lib.tsdbhip_spangroup_run_batch(ctx.handle, C.byref(desc), G, _abi.ptr(gss, C.c_uint32), outs)
    res = []
    for g in range(G):
        n = int(outs[g].n_out)
        ts, isi, bits = bufs[g]
        res.append((int(outs[g].err_code), ts[:n], isi[:n], bits[:n], int(outs[g].n_input_points),
                    int(outs[g].err_index)))
    return rc, res


class SpanGroup:
    """net.opentsdb.core.SpanGroup over libtsdbhip (SpanGroup.java:104-254)."""

    _default_ctx = None

    def __init__(self, tsdb, start_time, end_time, spans, rate, aggregator, interval=0,
                 downsampler=None, ctx=None):
        self.start_time = int(start_time)
        self.end_time = int(end_time)
        self.spans = []
        self.rate = bool(rate)
        self.aggregator = aggregator
        self.sample_interval = int(interval)
        self.downsampler = downsampler
        self._ctx = ctx
        self._result = None
        self._tsdb = tsdb
        self._tags_result = None  # (common, aggregated): from the device plan, else computed on first use
        self._widths = (3, 3, 3)  # metric, tag name, tag value UID widths of the spans' keys
        if spans is not None:
            for s in spans:
                self.add(s)

    def add(self, span):
        # SpanGroup.add's time filter (SpanGroup.java:135-139) needs the
        # assembled span; the library applies it, so every span is handed over.
        self.spans.append(span)
        self._result = None
        self._tags_result = None

    def _context(self):
        if self._ctx is None:
            if SpanGroup._default_ctx is None:
                SpanGroup._default_ctx = Context(0)
            self._ctx = SpanGroup._default_ctx
        return self._ctx

    def _run(self):
        if self._result is None:
            ss = pack_spans([s.rows for s in self.spans])
            ds = self.downsampler is not None and self.sample_interval > 0
            self._result = run_spanset(self._context(), ss, self.start_time, self.end_time,
                                       self.aggregator.code, self.rate,
                                       self.sample_interval if ds else 0,
                                       self.downsampler.code if ds else 0)
        return self._result

    def _points(self):
        rc, ts, isi, bits, _, _ = self._run()
        for i in range(len(ts)):
            yield DataPoint(ts[i], isi[i], bits[i])
        if rc:
            raise _exception_for(rc, self._context().last_error())

    def aggregatedSize(self):
        return self._run()[4]

    def _tags(self):
        """computeTags (SpanGroup.java:149-173): the device plan's result when
        group_by_and_aggregate stored one, else compute_tags over the spans'
        row keys with SpanGroup.add's time filter."""
        if self._tags_result is None:
            for s in self.spans:
                if getattr(s, "key", None) is None:
                    raise ValueError("SpanGroup.getTags: a span has no row key (Span(rows, key=...))")
            kept = [span_in_range(s, self.start_time, self.end_time) for s in self.spans]
            self._tags_result = compute_tags([s.key for s in self.spans], kept, *self._widths)
        return self._tags_result

    def _resolve(self, which, uid):
        m = getattr(self._tsdb, which, None)
        return m[uid] if m is not None else uid

    def getTags(self):
        """SpanGroup.getTags (SpanGroup.java:179-184): the tags every kept span
        carries with one value, name id -> value id (UID bytes); names and
        values as strings when the tsdb has tag_names / tag_values mappings."""
        common, _ = self._tags()
        if getattr(self._tsdb, "tag_names", None) is None or getattr(self._tsdb, "tag_values", None) is None:
            return dict(common)
        return {self._resolve("tag_names", k): self._resolve("tag_values", v) for k, v in common.items()}

    def getAggregatedTags(self):
        """SpanGroup.getAggregatedTags (SpanGroup.java:186-191): the first kept
        span's tag names that are not common, in its key's order."""
        _, agg = self._tags()
        if getattr(self._tsdb, "tag_names", None) is None:
            return list(agg)
        return [self._resolve("tag_names", k) for k in agg]

    def size(self):
        n = 0
        for _ in self._points():
            n += 1
        return n

    def iterator(self):
        return self._points()

    __iter__ = iterator

    def _get(self, i):
        if i < 0:
            raise IndexError("negative index: %d" % i)
        for j, dp in enumerate(self._points()):
            if j == i:
                return dp
        raise IndexError("index %d too large" % i)

    def timestamp(self, i):
        return self._get(i).timestamp()

    def isInteger(self, i):
        return self._get(i).isInteger()

    def longValue(self, i):
        return self._get(i).longValue()

    def doubleValue(self, i):
        return self._get(i).doubleValue()


# ---------------------------------------------------------------- GROUP BY ----
def span_cmp_key(row_key, metric_width=3):
    """Sort key equivalent to TsdbQuery.SpanCmp (TsdbQuery.java:594-621):
    metric id, then the tags, skipping the 4-byte base time; unsigned bytes,
    a shorter key first on a common prefix (Python bytes order)."""
    return bytes(row_key[:metric_width]) + bytes(row_key[metric_width + 4:])


def get_value_id(row_key, tag_id, metric_width=3, name_width=3, value_width=3):
    """Tags.getValueId (Tags.java:213-227): the value id of tag `tag_id` in
    the row key, or None."""
    pos = metric_width + 4
    while pos < len(row_key):
        if bytes(row_key[pos:pos + name_width]) == bytes(tag_id):
            pos += name_width
            return bytes(row_key[pos:pos + value_width])
        pos += name_width + value_width
    return None


def plan_groups(row_keys, group_bys, metric_width=3, name_width=3, value_width=3):
    """The grouping of TsdbQuery.groupByAndAggregate (TsdbQuery.java:294-363)
    as a plan: row_keys are the spans' row keys (any order, one per span).
    Returns (group_keys, order, group_span_start): the span indices in batch
    order (ByteMap order of the group keys, then SpanCmp order within a
    group) and the group boundaries. Spans without every group_by tag are
    dropped, as the reference does (with its log line)."""
    idx = sorted(range(len(row_keys)), key=lambda i: span_cmp_key(row_keys[i], metric_width))
    if group_bys is None:
        return [b""], idx, [0, len(idx)]
    tag_ids = sorted(bytes(t) for t in group_bys)  # group_bys is sorted by id
    groups = {}
    for i in idx:
        parts = []
        for t in tag_ids:
            v = get_value_id(row_keys[i], t, metric_width, name_width, value_width)
            if v is None:
                parts = None
                break
            parts.append(v)
        if parts is None:
            continue  # "WTF? Dropping span for row ..." (TsdbQuery.java:339-344)
        groups.setdefault(b"".join(parts), []).append(i)
    keys = sorted(groups)  # ByteMap: unsigned lexicographic
    order, gss = [], [0]
    for k in keys:
        order.extend(groups[k])
        gss.append(len(order))
    return keys, order, gss


def _parse_tags(row_key, metric_width, name_width, value_width):
    """the (name id, value id) pairs of a row key, in key order"""
    k = bytes(row_key)
    pos, pairs = metric_width + 4, []
    while pos < len(k):
        pairs.append((k[pos:pos + name_width], k[pos + name_width:pos + name_width + value_width]))
        pos += name_width + value_width
    return pairs


def compute_tags(keys, kept=None, metric_width=3, name_width=3, value_width=3):
    """SpanGroup.computeTags (SpanGroup.java:149-173) for one group, from its
    spans' row keys in group order; kept[i] false: SpanGroup.add filtered span
    i out. Returns (common: {name id: value id}, aggregated: [name id]): the
    base is the first kept span's tags; a pair is common iff every other kept
    span has that name with that value; aggregated is the base's other names
    (in key order; the reference's HashSet has none). A name only later spans
    carry is reported nowhere, as in the reference."""
    live = [k for i, k in enumerate(keys) if kept is None or kept[i]]
    if not live:
        return {}, []
    base = _parse_tags(live[0], metric_width, name_width, value_width)
    common = dict(base)
    for k in live[1:]:
        other = {}
        for nm, v in _parse_tags(k, metric_width, name_width, value_width):
            other.setdefault(nm, v)
        for nm in [nm for nm, v in common.items() if other.get(nm) != v]:
            del common[nm]
    return common, [nm for nm, _ in base if nm not in common]


def span_in_range(span, start, end):
    """SpanGroup.add's filter (SpanGroup.java:135-139): the span's first
    timestamp <= end and its last >= start, read from the first cell of its
    first row and the last cell of its last row. A span without rows counts
    as kept (its group's run reports E_EMPTY_SPAN)."""
    rows = [r for r in span.rows if len(r.qualifier) >= 2]
    if not rows:
        return True
    f, l = rows[0], rows[-1]
    first = f.base_time + (int.from_bytes(f.qualifier[0:2], "big") >> 4)
    last = l.base_time + (int.from_bytes(l.qualifier[-2:], "big") >> 4)
    return first <= end and last >= start


class GroupPlan:
    """tsdbhip_groups_out as numpy arrays (trimmed to what the call set)."""

    def __init__(self, out, order, gss, gkey, ntags, tags, common, klen, name_width, value_width):
        G, ng = int(out.n_groups), int(out.n_grouped)
        self.n_groups, self.n_grouped, self.n_dropped = G, ng, int(out.n_dropped)
        self.order = order[:ng]
        self.group_span_start = gss[:G + 1]
        self.group_keys = [gkey[g * klen:(g + 1) * klen].tobytes() for g in range(G)]
        self.group_ntags = ntags[:G]
        self.group_tags = tags[:G]
        self.group_common = common[:G]
        self._nw, self._vw = name_width, value_width

    def tags_of(self, g):
        """(common: {name id: value id}, aggregated: [name id]) of group g"""
        common, agg = {}, []
        raw, pair = self.group_tags[g].tobytes(), self._nw + self._vw
        for j in range(int(self.group_ntags[g])):
            nm, v = raw[j * pair:j * pair + self._nw], raw[j * pair + self._nw:(j + 1) * pair]
            if (int(self.group_common[g]) >> j) & 1:
                common[nm] = v
            else:
                agg.append(nm)
        return common, agg


def run_groupby_plan(ctx, key_off, key_bytes, group_bys, kept=None, metric_width=3, name_width=3, value_width=3,
                     capacity=None, device=False, n_spans=None, key_nbytes=None):
    """Low-level: one tsdbhip_groupby_plan over row keys in SpanCmp order.
    key_off / key_bytes / kept are numpy arrays, or with device=True device
    addresses (ints; n_spans and key_nbytes then given). group_bys: the tag
    name ids, sorted, or None. Returns (code, GroupPlan)."""
    d = _abi.KeysDesc()
    if device:
        n, nbytes = int(n_spans), int(key_nbytes)
        d.flags = _abi.DESC_DEVICE
        d.key_off = C.cast(C.c_void_p(int(key_off)), _abi.P64)
        d.key_bytes = C.cast(C.c_void_p(int(key_bytes)), _abi.P8)
        if kept is not None:
            d.span_kept = C.cast(C.c_void_p(int(kept)), _abi.P8)
    else:
        key_off = np.ascontiguousarray(key_off, np.uint64)
        key_bytes = np.ascontiguousarray(key_bytes, np.uint8)
        n = len(key_off) - 1 if n_spans is None else int(n_spans)
        nbytes = len(key_bytes) if key_nbytes is None else int(key_nbytes)
        d.key_off = _abi.ptr(key_off, C.c_uint64)
        d.key_bytes = _abi.ptr(key_bytes, C.c_uint8)
        if kept is not None:
            kept = np.ascontiguousarray(kept, np.uint8)
            d.span_kept = _abi.ptr(kept, C.c_uint8)
    gbs = [bytes(t) for t in (group_bys or [])]
    gb = np.frombuffer(b"".join(gbs) + b"\0", np.uint8).copy()
    d.n_spans, d.key_nbytes = n, nbytes
    d.metric_width, d.name_width, d.value_width = int(metric_width), int(name_width), int(value_width)
    d.n_group_bys = len(gbs)
    d.group_bys = _abi.ptr(gb, C.c_uint8)
    cap = max(1, n) if capacity is None else int(capacity)
    klen = len(gbs) * int(value_width) if 1 <= int(value_width) <= 8 else 0
    ts = _abi.MAX_TAGS * (max(1, min(8, int(name_width))) + max(1, min(8, int(value_width))))
    order = np.zeros(max(1, n), np.uint32)
    gss = np.zeros(cap + 1, np.uint32)
    gkey = np.zeros(max(1, cap * klen), np.uint8)
    ntags = np.zeros(cap, np.uint8)
    tags = np.zeros((cap, ts), np.uint8)
    common = np.zeros(cap, np.uint8)
    out = _abi.GroupsOut()
    out.group_capacity = cap
    out.order = _abi.ptr(order, C.c_uint32)
    out.group_span_start = _abi.ptr(gss, C.c_uint32)
    out.group_key = _abi.ptr(gkey, C.c_uint8)
    out.group_ntags = _abi.ptr(ntags, C.c_uint8)
    out.group_tags = _abi.ptr(tags, C.c_uint8)
    out.group_common = _abi.ptr(common, C.c_uint8)
    rc = ctx._lib.tsdbhip_groupby_plan(ctx.handle, C.byref(d), C.byref(out))
    if rc:  # (no array was written: only the counts, which E_CAPACITY sets for a retry)
        plan = GroupPlan.__new__(GroupPlan)
        plan.n_groups, plan.n_grouped, plan.n_dropped = int(out.n_groups), int(out.n_grouped), int(out.n_dropped)
        plan.raw = (order, gss, gkey, ntags, tags, common)  # the untouched output arrays
        return rc, plan
    return rc, GroupPlan(out, order, gss, gkey, ntags, tags, common, klen, int(name_width), int(value_width))


def plan_groups_device(ctx, row_keys, group_bys, kept=None, metric_width=3, name_width=3, value_width=3):
    """plan_groups on the GPU (tsdbhip_groupby_plan), with every group's tags:
    row_keys in any order, one per span; kept[i] false: SpanGroup.add's time
    filter drops span i from the tags (it stays in its group's batch: the
    library applies the filter to the points itself). Returns (group_keys,
    order, group_span_start, tags), the first three as plan_groups returns
    them, tags[g] = (common: {name id: value id}, aggregated: [name id])."""
    idx = sorted(range(len(row_keys)), key=lambda i: span_cmp_key(row_keys[i], metric_width))
    keys = [bytes(row_keys[i]) for i in idx]
    key_off = np.zeros(len(keys) + 1, np.uint64)
    if keys:
        key_off[1:] = np.cumsum([len(k) for k in keys])
    key_bytes = np.frombuffer(b"".join(keys), np.uint8)
    kept_a = None if kept is None else np.array([1 if kept[i] else 0 for i in idx], np.uint8)
    gbs = None if group_bys is None else sorted(bytes(t) for t in group_bys)  # group_bys is sorted by id
    rc, plan = run_groupby_plan(ctx, key_off, key_bytes, gbs, kept_a, metric_width, name_width, value_width)
    ctx.check(rc)
    order = [idx[j] for j in plan.order.tolist()]
    return (plan.group_keys, order, plan.group_span_start.tolist(),
            [plan.tags_of(g) for g in range(plan.n_groups)])


def group_by_and_aggregate(spans, group_bys, start_time, end_time, rate, aggregator, interval=0,
                           downsampler=None, ctx=None, metric_width=3, name_width=3, value_width=3,
                           device_plan=False, tsdb=None):
    """TsdbQuery.groupByAndAggregate over libtsdbhip: `spans` maps row key
    bytes -> Span (findSpans' TreeMap), `group_bys` the tag-name ids to group
    by (None: one group). Returns the SpanGroups in the reference's order,
    all evaluated by one tsdbhip_spangroup_run_batch; each raises its own
    exception lazily while iterated, like the reference's. device_plan: the
    grouping and every group's tags by tsdbhip_groupby_plan (the default: the
    host loop of plan_groups, tags computed on first use)."""
    keys = list(spans)
    if not keys:
        return []
    for k in keys:
        if getattr(spans[k], "key", None) is None:
            spans[k].key = bytes(k)
    tags = None
    if device_plan:
        if ctx is None:
            ctx = SpanGroup(None, start_time, end_time, None, rate, aggregator)._context()
        kept = [span_in_range(spans[k], start_time, end_time) for k in keys]
        gkeys, order, gss, tags = plan_groups_device(ctx, keys, group_bys, kept, metric_width, name_width,
                                                     value_width)
    else:
        gkeys, order, gss = plan_groups(keys, group_bys, metric_width, name_width, value_width)
    groups = [SpanGroup(tsdb, start_time, end_time, [spans[keys[i]] for i in order[gss[g]:gss[g + 1]]], rate,
                        aggregator, interval, downsampler, ctx) for g in range(len(gkeys))]
    if not groups:
        return []
    for g, grp in enumerate(groups):
        grp._widths = (metric_width, name_width, value_width)
        if tags is not None:
            grp._tags_result = tags[g]
    ss = pack_spans([spans[keys[i]].rows for i in order])
    ds = downsampler is not None and interval > 0
    c = groups[0]._context()
    _, res = run_spanset_batch(c, ss, gss, start_time, end_time, aggregator.code, rate,
                               interval if ds else 0, downsampler.code if ds else 0)
    for grp, r in zip(groups, res):
        grp._ctx = c
        grp._result = r
    return groups


# --------------------------------------------------------------- findSpans ----
def find_spans(rows, metric, metric_width=3, name_width=3, value_width=3):
    """TsdbQuery.findSpans (TsdbQuery.java:240-285) restated on the host:
    `rows` is a list of (row_key, KeyValue | None) in the order the scanner
    delivered them, None standing for a row tsdb.compact(row) returned null
    for. Returns {row key: Span} in SpanCmp order, the key being the full row
    key of the span's first delivered row (what TreeMap.put keeps) and the
    span's rows in delivery order, or None when no row was added (:281-283).
    A key that does not start with `metric`: IllegalDataException (:254-258)."""
    metric = bytes(metric)
    spans, nrows = {}, 0  # by SpanCmp key, in insertion order
    for i, (k, kv) in enumerate(rows):
        k = bytes(k)
        if k[:metric_width] != metric[:metric_width]:
            raise IllegalDataException(f"HBase returned a row that doesn't match our scanner: row {i} does not "
                                       f"start with {list(metric)}")
        span = spans.get(span_cmp_key(k, metric_width))
        if span is None:
            span = spans[span_cmp_key(k, metric_width)] = Span(key=k)
        if kv is not None:  # Can be null if we ignored all KVs.
            span.addRow(kv)
            nrows += 1
    if nrows == 0:
        return None
    return {spans[c].key: spans[c] for c in sorted(spans)}


class FoundSpans:
    """tsdbhip_spans_out as numpy arrays (trimmed to what the call set); on
    an error only the counts, and .raw = the untouched output arrays."""

    FIELDS = ("row_order", "span_row_start", "row_base", "row_ncells", "row_qual_off", "row_val_off",
              "row_val_len", "key_off", "key_bytes")

    def __init__(self, out, arrays, ok):
        self.n_spans, self.n_rows, self.n_skipped = int(out.n_spans), int(out.n_rows), int(out.n_skipped)
        self.key_used = int(out.key_used)
        self.raw = arrays
        if not ok:
            return
        S, R = self.n_spans, self.n_rows
        for f in self.FIELDS:
            a = arrays.get(f)
            if a is None or isinstance(a, int):
                setattr(self, f, None)
            elif f in ("span_row_start", "key_off"):
                setattr(self, f, a[:S + 1])
            elif f == "key_bytes":
                setattr(self, f, a[:self.key_used])
            else:
                setattr(self, f, a[:R])

    def keys(self):
        kb = self.key_bytes.tobytes()
        return [kb[int(self.key_off[s]):int(self.key_off[s + 1])] for s in range(self.n_spans)]


def run_find_spans(ctx, key_off, key_bytes, metric, status=None, cells=None, metric_width=3, name_width=3,
                   value_width=3, span_capacity=None, key_capacity=None, device=False, n_rows=None,
                   key_nbytes=None, outputs=None):
    """Low-level: one tsdbhip_find_spans over rows in delivery order.
    key_off / key_bytes / status and cells = (qual_off, qual_len, val_off,
    val_len) are numpy arrays, or with device=True device addresses (ints;
    n_rows and key_nbytes then given, and outputs = {field: device address} of
    the caller's output arrays, span_capacity / key_capacity their sizes).
    outputs may also pre-fill host arrays (the tests' sentinels). Returns
    (code, FoundSpans)."""
    d = _abi.ScanDesc()
    keep = []

    def inp(a, dtype, ptype):
        if a is None:
            return None
        if device:
            return C.cast(C.c_void_p(int(a)), ptype)
        a = np.ascontiguousarray(a, dtype)
        keep.append(a)
        return a.ctypes.data_as(ptype)

    if device:
        n, nbytes = int(n_rows), int(key_nbytes)
        d.flags = _abi.DESC_DEVICE
    else:
        n = (len(key_off) - 1 if key_off is not None else 0) if n_rows is None else int(n_rows)
        nbytes = (len(key_bytes) if key_bytes is not None else 0) if key_nbytes is None else int(key_nbytes)
    ko, kb, st = inp(key_off, np.uint64, _abi.P64), inp(key_bytes, np.uint8, _abi.P8), inp(status, np.uint8, _abi.P8)
    if ko is not None:
        d.key_off = ko
    if kb is not None:
        d.key_bytes = kb
    if st is not None:
        d.row_status = st
    if cells is not None:
        for f, a, dt, pt in zip(("row_qual_off", "row_qual_len", "row_val_off", "row_val_len"), cells,
                                (np.uint64, np.uint32, np.uint64, np.uint32),
                                (_abi.P64, _abi.P32, _abi.P64, _abi.P32)):
            p = inp(a, dt, pt)
            if p is not None:
                setattr(d, f, p)
    m = np.frombuffer(bytes(metric) + b"\0" * 8, np.uint8).copy()
    d.metric = _abi.ptr(m, C.c_uint8)
    d.n_rows, d.key_nbytes = n, nbytes
    d.metric_width, d.name_width, d.value_width = int(metric_width), int(name_width), int(value_width)
    scap = max(1, n) if span_capacity is None else int(span_capacity)
    kcap = max(1, nbytes) if key_capacity is None else int(key_capacity)
    out = _abi.SpansOut()
    out.span_capacity, out.key_capacity = scap, kcap
    types = {"row_order": (np.uint32, _abi.P32, max(1, n)), "span_row_start": (np.uint64, _abi.P64, scap + 1),
             "row_base": (np.uint32, _abi.P32, max(1, n)), "row_ncells": (np.uint32, _abi.P32, max(1, n)),
             "row_qual_off": (np.uint64, _abi.P64, max(1, n)), "row_val_off": (np.uint64, _abi.P64, max(1, n)),
             "row_val_len": (np.uint32, _abi.P32, max(1, n)), "key_off": (np.uint64, _abi.P64, scap + 1),
             "key_bytes": (np.uint8, _abi.P8, max(1, kcap))}
    arrays = {}
    for f, (dt, pt, size) in types.items():
        if device:
            a = (outputs or {}).get(f)
            if a is not None:
                arrays[f] = int(a)
                setattr(out, f, C.cast(C.c_void_p(int(a)), pt))
            continue
        if outputs is not None and f in outputs:
            a = outputs[f]
            if a is None:  # (a null output array, for the argument checks)
                arrays[f] = None
                continue
        elif cells is None and f in ("row_ncells", "row_qual_off", "row_val_off", "row_val_len"):
            continue
        else:
            a = np.zeros(size, dt)
        assert a.dtype == dt and a.flags.c_contiguous
        arrays[f] = a
        setattr(out, f, a.ctypes.data_as(pt))
    rc = ctx._lib.tsdbhip_find_spans(ctx.handle, C.byref(d), C.byref(out))
    return rc, FoundSpans(out, arrays, rc == 0)


def _pack_keys(rows):
    """(key_off, key_bytes, status) of find_spans' rows"""
    keys = [bytes(k) for k, _ in rows]
    key_off = np.zeros(len(keys) + 1, np.uint64)
    if keys:
        key_off[1:] = np.cumsum([len(k) for k in keys])
    key_bytes = np.frombuffer(b"".join(keys), np.uint8).copy()
    status = np.array([_abi.ROW_NONE if kv is None else _abi.ROW_SINGLE for _, kv in rows], np.uint8)
    return key_off, key_bytes, status


def _pack_scan(rows):
    """(key_off, key_bytes, status, cells, qual_bytes, val_bytes) of find_spans'
    rows, the compacted cells packed in delivery order as pack_spans lays them out"""
    key_off, key_bytes, status = _pack_keys(rows)
    ss = pack_spans([[kv if kv is not None else KeyValue(0, b"", b"") for _, kv in rows]])
    cells = (ss.row_qual_off, (ss.row_ncells * 2).astype(np.uint32), ss.row_val_off, ss.row_val_len)
    return key_off, key_bytes, status, cells, ss.qual_bytes, ss.val_bytes


def find_spans_device(ctx, rows, metric, metric_width=3, name_width=3, value_width=3):
    """find_spans on the GPU (tsdbhip_find_spans): the same dict, or None."""
    key_off, key_bytes, status = _pack_keys(rows)
    rc, fs = run_find_spans(ctx, key_off, key_bytes, metric, status, None, metric_width, name_width, value_width)
    if rc:
        raise _exception_for(rc, ctx.last_error())
    if fs.n_rows == 0:
        return None
    srs, order, out = fs.span_row_start.tolist(), fs.row_order.tolist(), {}
    for s, k in enumerate(fs.keys()):
        out[k] = Span([rows[r][1] for r in order[srs[s]:srs[s + 1]]], key=k)
    return out


def query_run(ctx, rows, metric, group_bys, start_time, end_time, rate, aggregator, interval=0, downsampler=None,
              metric_width=3, name_width=3, value_width=3, device=False, tsdb=None):
    """TsdbQuery.run (TsdbQuery.java:225-227): groupByAndAggregate(findSpans())
    over the rows of a scan (find_spans' `rows`). device: findSpans by
    tsdbhip_find_spans and the grouping by tsdbhip_groupby_plan; otherwise the
    host restatements. The SpanGroups are evaluated on the GPU either way."""
    if device:
        spans = find_spans_device(ctx, rows, metric, metric_width, name_width, value_width)
    else:
        spans = find_spans(rows, metric, metric_width, name_width, value_width)
    if spans is None:
        return []
    return group_by_and_aggregate(spans, group_bys, start_time, end_time, rate, aggregator, interval, downsampler,
                                  ctx, metric_width, name_width, value_width, device_plan=device, tsdb=tsdb)


# --------------------------------------------------------------- getScanner ----
def scan_times(start_time, end_time, interval=0):
    """(scan_start, scan_stop) of TsdbQuery.getScanner (TsdbQuery.java:378-382,
    396-425): 64-bit arithmetic, then (int). end_time None: UNSET, the stop key
    is metric | 0xFFFFFFFF."""
    ts = int(start_time) - 2 * 3600 - int(interval)
    stop = 0xFFFFFFFF if end_time is None else (int(end_time) + 3600 + 1 + int(interval)) & 0xFFFFFFFF
    return (ts if ts > 0 else 0) & 0xFFFFFFFF, stop


def _scan_items(tags, group_bys, group_by_values, name_width, value_width):
    """the checks of tsdbhip_scan_rows on a query, in its order, and the items
    of createAndSetFilter's merge (:455-488): [(name, None: any | set of ids)]"""
    tags = [(bytes(n), bytes(v)) for n, v in (tags.items() if isinstance(tags, dict) else (tags or []))]
    gbs = [bytes(g) for g in (group_bys or [])]
    if len(tags) > _abi.MAX_TAGS:
        raise ValueError("more than TSDBHIP_MAX_TAGS tags")
    if len(gbs) > _abi.MAX_TAGS:
        raise ValueError("more than TSDBHIP_MAX_TAGS group_bys")
    for n, v in tags:
        if len(n) != name_width or len(v) != value_width:
            raise ValueError("a tag of the wrong width")
    if any(len(g) != name_width for g in gbs):
        raise ValueError("a group_by of the wrong width")
    if any(a[0] >= b[0] for a, b in zip(tags, tags[1:])):
        raise ValueError("tags not strictly ascending by name")
    if any(a >= b for a, b in zip(gbs, gbs[1:])):
        raise ValueError("group_bys not strictly ascending")
    if {n for n, _ in tags} & set(gbs):
        raise ValueError("a name is both in tags and in group_bys")  # the AssertionError of :510-515
    gbv = {bytes(k): [bytes(x) for x in v] for k, v in (group_by_values or {}).items() if v}
    if any(len(x) != value_width for v in gbv.values() for x in v):
        raise ValueError("a value id of the wrong width")
    items = [(n, {v}) for n, v in tags] + [(g, set(gbv[g]) if g in gbv else None) for g in gbs]
    return tags, gbs, gbv, sorted(items, key=lambda it: it[0])


def _key_of(row):
    return bytes(row[0]) if isinstance(row, (tuple, list)) else bytes(row)


def scan_rows(rows, metric, tags=None, group_bys=None, group_by_values=None, start_time=0, end_time=None, interval=0,
              metric_width=3, name_width=3, value_width=3):
    """The rows the Scanner of TsdbQuery.getScanner delivers (TsdbQuery.java:
    368-394), restated on the host: `rows` is the table, row keys or find_spans'
    (row_key, KeyValue) pairs, of any metric in any order; tags the fixed
    (name id, value id) pairs, ascending by name; group_bys the name ids,
    ascending; group_by_values {name id: [value ids]} (absent or empty: any
    value, the tag=* of findGroupBys :192-223); end_time None: UNSET. Returns
    the indices of the selected rows, in table order: inside the start / stop
    keys and matching createAndSetFilter's regexp (:433-492), decided by walking
    the key's pairs once with an item cursor. ValueError: what
    tsdbhip_scan_rows answers TSDBHIP_E_INVALID_ARG to."""
    if not all(1 <= w <= 8 for w in (metric_width, name_width, value_width)):
        raise ValueError("a width outside 1..8")
    _, _, _, items = _scan_items(tags, group_bys, group_by_values, name_width, value_width)
    t0, t1 = scan_times(start_time, end_time, interval)
    metric = bytes(metric)[:metric_width]
    hdr, pair = metric_width + 4, name_width + value_width
    keys = [_key_of(r) for r in rows]
    for i, k in enumerate(keys):
        if len(k) < hdr or (len(k) - hdr) % pair or (len(k) - hdr) // pair > _abi.MAX_TAGS:
            raise ValueError(f"bad row key length at row {i}")
    sel = []
    for i, k in enumerate(keys):
        if k[:metric_width] != metric or not t0 <= int.from_bytes(k[metric_width:hdr], "big") < t1:
            continue
        if items:
            if len(items) > _abi.MAX_TAGS:
                continue
            cur = 0
            for pos in range(hdr, len(k), pair):
                if cur == len(items):
                    break
                name, vals = items[cur]
                if k[pos:pos + name_width] == name and (vals is None or k[pos + name_width:pos + pair] in vals):
                    cur += 1
            if cur != len(items):
                continue
        sel.append(i)
    return sel


class ScanSelection:
    """tsdbhip_scan_sel as numpy arrays (trimmed to what the call set); on an
    error only the counts, and .raw = the untouched output arrays."""

    FIELDS = ("row_index", "key_off", "key_bytes", "row_status", "row_qual_off", "row_qual_len", "row_val_off",
              "row_val_len")

    def __init__(self, out, arrays, ok):
        self.n_selected, self.key_used = int(out.n_selected), int(out.key_used)
        self.raw = arrays
        if not ok:
            return
        for f in self.FIELDS:
            a = arrays.get(f)
            if a is None or isinstance(a, int):
                setattr(self, f, None)
            elif f == "key_off":
                setattr(self, f, a[:self.n_selected + 1])
            elif f == "key_bytes":
                setattr(self, f, a[:self.key_used])
            else:
                setattr(self, f, a[:self.n_selected])

    def keys(self):
        kb = self.key_bytes.tobytes()
        return [kb[int(self.key_off[s]):int(self.key_off[s + 1])] for s in range(self.n_selected)]


def make_scan_query(tags, group_bys, group_by_values, start_time, end_time, interval, name_width=3, value_width=3):
    """(tsdbhip_scan_query, the arrays it points to): no check is made here,
    the library makes them"""
    tags = [(bytes(n), bytes(v)) for n, v in (tags.items() if isinstance(tags, dict) else (tags or []))]
    gbs = [bytes(g) for g in (group_bys or [])]
    gbv = {bytes(k): [bytes(x) for x in v] for k, v in (group_by_values or {}).items()}
    q = _abi.ScanQuery()
    q.start_time = int(start_time)
    q.end_time = 0 if end_time is None else int(end_time)
    q.sample_interval = int(interval)
    q.flags = _abi.SCAN_END_UNSET if end_time is None else 0
    q.n_tags, q.n_group_bys = len(tags), len(gbs)
    t = np.frombuffer(b"".join(n + v for n, v in tags) + b"\0", np.uint8).copy()
    g = np.frombuffer(b"".join(gbs) + b"\0", np.uint8).copy()
    nv = np.array([len(gbv.get(x, ())) for x in gbs] + [0], np.uint32)
    v = np.frombuffer(b"".join(b"".join(gbv.get(x, ())) for x in gbs) + b"\0", np.uint8).copy()
    q.tags, q.group_bys = _abi.ptr(t, C.c_uint8), _abi.ptr(g, C.c_uint8)
    q.group_by_nvalues, q.group_by_values = _abi.ptr(nv, C.c_uint32), _abi.ptr(v, C.c_uint8)
    return q, (t, g, nv, v)


def run_scan_rows(ctx, key_off, key_bytes, metric, query, status=None, cells=None, metric_width=3, name_width=3,
                  value_width=3, row_capacity=None, key_capacity=None, device=False, n_rows=None, key_nbytes=None,
                  outputs=None):
    """Low-level: one tsdbhip_scan_rows over a table. key_off / key_bytes /
    status and cells = (qual_off, qual_len, val_off, val_len) are numpy arrays,
    or with device=True device addresses (ints; n_rows and key_nbytes then
    given, and outputs = {field: device address} of the caller's output arrays,
    row_capacity / key_capacity their sizes). query: a tsdbhip_scan_query
    (make_scan_query). outputs may also pre-fill host arrays (the tests'
    sentinels). Returns (code, ScanSelection)."""
    d = _abi.ScanDesc()
    keep = []

    def inp(a, dtype, ptype):
        if a is None:
            return None
        if device:
            return C.cast(C.c_void_p(int(a)), ptype)
        a = np.ascontiguousarray(a, dtype)
        keep.append(a)
        return a.ctypes.data_as(ptype)

    if device:
        n, nbytes = int(n_rows), int(key_nbytes)
        d.flags = _abi.DESC_DEVICE
    else:
        n = (len(key_off) - 1 if key_off is not None else 0) if n_rows is None else int(n_rows)
        nbytes = (len(key_bytes) if key_bytes is not None else 0) if key_nbytes is None else int(key_nbytes)
    for f, a, dt, pt in (("key_off", key_off, np.uint64, _abi.P64), ("key_bytes", key_bytes, np.uint8, _abi.P8),
                         ("row_status", status, np.uint8, _abi.P8)):
        p = inp(a, dt, pt)
        if p is not None:
            setattr(d, f, p)
    if cells is not None:
        for f, a, dt, pt in zip(("row_qual_off", "row_qual_len", "row_val_off", "row_val_len"), cells,
                                (np.uint64, np.uint32, np.uint64, np.uint32),
                                (_abi.P64, _abi.P32, _abi.P64, _abi.P32)):
            p = inp(a, dt, pt)
            if p is not None:
                setattr(d, f, p)
    m = np.frombuffer(bytes(metric) + b"\0" * 8, np.uint8).copy()
    d.metric = _abi.ptr(m, C.c_uint8)
    d.n_rows, d.key_nbytes = n, nbytes
    d.metric_width, d.name_width, d.value_width = int(metric_width), int(name_width), int(value_width)
    rcap = max(1, n) if row_capacity is None else int(row_capacity)
    kcap = max(1, nbytes) if key_capacity is None else int(key_capacity)
    out = _abi.ScanSel()
    out.row_capacity, out.key_capacity = rcap, kcap
    types = {"row_index": (np.uint32, _abi.P32, max(1, rcap)), "key_off": (np.uint64, _abi.P64, rcap + 1),
             "key_bytes": (np.uint8, _abi.P8, max(1, kcap)), "row_status": (np.uint8, _abi.P8, max(1, rcap)),
             "row_qual_off": (np.uint64, _abi.P64, max(1, rcap)), "row_qual_len": (np.uint32, _abi.P32, max(1, rcap)),
             "row_val_off": (np.uint64, _abi.P64, max(1, rcap)), "row_val_len": (np.uint32, _abi.P32, max(1, rcap))}
    arrays = {}
    for f, (dt, pt, size) in types.items():
        if device:
            a = (outputs or {}).get(f)
            if a is not None:
                arrays[f] = int(a)
                setattr(out, f, C.cast(C.c_void_p(int(a)), pt))
            continue
        if outputs is not None and f in outputs:
            a = outputs[f]
            if a is None:  # (a null output array, for the argument checks)
                arrays[f] = None
                continue
        elif (status is None and f == "row_status") or (cells is None and f.startswith("row_") and f != "row_index"
                                                        and f != "row_status"):
            continue
        else:
            a = np.zeros(size, dt)
        assert a.dtype == dt and a.flags.c_contiguous
        arrays[f] = a
        setattr(out, f, a.ctypes.data_as(pt))
    rc = ctx._lib.tsdbhip_scan_rows(ctx.handle, C.byref(d), C.byref(query), C.byref(out))
    return rc, ScanSelection(out, arrays, rc == 0)


def scan_rows_device(ctx, rows, metric, tags=None, group_bys=None, group_by_values=None, start_time=0, end_time=None,
                     interval=0, metric_width=3, name_width=3, value_width=3):
    """scan_rows on the GPU (tsdbhip_scan_rows): the same indices."""
    keys = [_key_of(r) for r in rows]
    key_off = np.zeros(len(keys) + 1, np.uint64)
    if keys:
        key_off[1:] = np.cumsum([len(k) for k in keys])
    key_bytes = np.frombuffer(b"".join(keys), np.uint8).copy()
    q, keep = make_scan_query(tags, group_bys, group_by_values, start_time, end_time, interval, name_width, value_width)
    rc, sel = run_scan_rows(ctx, key_off, key_bytes, metric, q, None, None, metric_width, name_width, value_width)
    if rc:
        raise _exception_for(rc, ctx.last_error())
    return sel.row_index.tolist()


def tsdb_query_run(ctx, table_rows, metric, tags, group_bys, group_by_values, start_time, end_time, rate, aggregator,
                   interval=0, downsampler=None, metric_width=3, name_width=3, value_width=3, device=False,
                   tsdb=None):
    """TsdbQuery.run from the table on: the scanner (scan_rows; device:
    tsdbhip_scan_rows) over table_rows, find_spans' (row_key, KeyValue | None)
    pairs of any metric, then query_run over the rows it delivers. The
    scanner looks further than the query's times (:396-425) with the
    downsampling interval as sample_interval, as the reference sets it."""
    scan = scan_rows_device if device else scan_rows
    args = (table_rows, metric, tags, group_bys, group_by_values, start_time, end_time, interval, metric_width,
            name_width, value_width)
    sel = scan(ctx, *args) if device else scan(*args)
    rows = [table_rows[i] for i in sel]
    return query_run(ctx, rows, metric, group_bys, start_time, U32_END if end_time is None else end_time, rate,
                     aggregator, interval, downsampler, metric_width, name_width, value_width, device=device,
                     tsdb=tsdb)


U32_END = 0xFFFFFFFF


# ------------------------------------------- repacking a device descriptor ----
def pack_offsets(row_ncells, row_val_len):
    """The placement rule of packing.pack_spans and tsdbhip_desc_pack for rows
    of these lengths, in row order: (row_qual_off, row_val_off, qual_nbytes,
    val_nbytes). Row i's qualifiers lie at the sum of align8(2 ncells) of the
    rows before it, its values at the sum of align16(val_len); a buffer is
    align16(max(that sum over every row, 1)) bytes long."""
    qsz = (2 * np.asarray(row_ncells, np.uint64) + np.uint64(7)) & ~np.uint64(7)
    vsz = (np.asarray(row_val_len, np.uint64) + np.uint64(15)) & ~np.uint64(15)
    qend = np.cumsum(qsz, dtype=np.uint64)
    vend = np.cumsum(vsz, dtype=np.uint64)
    q_used = int(qend[-1]) if len(qend) else 0
    v_used = int(vend[-1]) if len(vend) else 0
    return qend - qsz, vend - vsz, (max(q_used, 1) + 15) // 16 * 16, (max(v_used, 1) + 15) // 16 * 16


def run_desc_pack(ctx, desc, order=None):
    """Low-level: one tsdbhip_desc_pack of the device-resident SgDesc `desc`
    (order: span indices, None: every span in its own order). Returns (code,
    SgDesc): the packed descriptor's arrays belong to the context until
    tsdbhip_desc_pack_free (PackedDesc frees on exit)."""
    out = _abi.SgDesc()
    if order is None:
        rc = ctx._lib.tsdbhip_desc_pack(ctx.handle, C.byref(desc), None, desc.n_spans, C.byref(out))
    else:
        o = np.ascontiguousarray(order, np.uint32)
        rc = ctx._lib.tsdbhip_desc_pack(ctx.handle, C.byref(desc), _abi.ptr(o, C.c_uint32), len(o), C.byref(out))
    return rc, out


class PackedDesc:
    """`with PackedDesc(ctx, desc, order) as d:` d is the packed SgDesc; a
    failed pack raises, the arrays are freed on exit."""

    def __init__(self, ctx, desc, order=None):
        self.ctx, self.src, self.order, self.desc = ctx, desc, order, None

    def __enter__(self):
        rc, d = run_desc_pack(self.ctx, self.src, self.order)
        if rc:
            raise _exception_for(rc, self.ctx.last_error())
        self.desc = d
        return d

    def __exit__(self, *exc):
        if self.desc is not None:
            self.ctx._lib.tsdbhip_desc_pack_free(self.ctx.handle, C.byref(self.desc))
        return False


# ------------------------------------------ the qualifier certificate ----
def row_quals_proven(q):
    """TSDBHIP_DESC_QUALS_PROVEN's statement for one row, `q` its qualifier
    bytes: the big-endian 16-bit words are q0 + c (q1 - q0) without wrap, and
    q1 - q0 is positive and a multiple of 16. A row of fewer than two cells is
    proven."""
    w = np.frombuffer(bytes(q), dtype=">u2").astype(np.int64)
    if len(w) < 2:
        return True
    q0, d = int(w[0]), int(w[1]) - int(w[0])
    if d <= 0 or d % 16 or q0 + (len(w) - 1) * d > 0xFFFF:
        return False
    return bool(np.array_equal(w, q0 + d * np.arange(len(w), dtype=np.int64)))


def quals_proven(ss, qual_nbytes=None):
    """The host restatement of tsdbhip_desc_certify over a SpanSet, row by row:
    a bool a row, True where the row is proven. tsdbhip_desc_certify counts the
    False ones and sets the flag iff there is none. A row at an odd offset or
    not inside qual_nbytes (default: the buffer's length) is unproven and
    unread."""
    qn = len(ss.qual_bytes) if qual_nbytes is None else int(qual_nbytes)
    ok = np.zeros(int(ss.n_rows), bool)
    for r in range(int(ss.n_rows)):
        qo, n = int(ss.row_qual_off[r]), int(ss.row_ncells[r])
        if qo % 2 or qo > qn or 2 * n > qn - qo:
            continue
        ok[r] = row_quals_proven(ss.qual_bytes[qo:qo + 2 * n])
    return ok


def desc_certify(ctx, desc):
    """One tsdbhip_desc_certify of the SgDesc `desc`: (code, n_unproven_rows);
    desc.flags gains or loses DESC_QUALS_PROVEN."""
    n = C.c_uint64(0)
    rc = ctx._lib.tsdbhip_desc_certify(ctx.handle, C.byref(desc), C.byref(n))
    return rc, int(n.value)


# ------------------------------------------------------------ output text ----
FMT_ASCII, FMT_GNUPLOT, FMT_CLI = 0, 1, 2


def format_points(mode, ts, is_int, bits, metric="", tags="", utc_offset=0):
    """tsdbhip_format_points: the lines GraphHandler.respondAsciiQuery
    (GraphHandler.java:785-808), Plot.dumpToFiles (Plot.java:190-204) or
    CliQuery (CliQuery.java:161-170) print for these points. Raises
    IllegalStateException on a NaN/Infinity where the reference does."""
    from ._lib import lib
    L = lib()
    ts = np.ascontiguousarray(ts, np.int64)
    isi = np.ascontiguousarray(is_int, np.uint8)
    bits = np.ascontiguousarray(bits, np.int64)
    n = len(ts)
    cap = max(64, n * (len(metric) + len(tags) + 64))
    buf = C.create_string_buffer(cap)
    rc = L.tsdbhip_format_points(mode, metric.encode(), tags.encode(), int(utc_offset), _abi.ptr(ts, C.c_int64),
                                 _abi.ptr(isi, C.c_uint8), _abi.ptr(bits, C.c_int64), n, buf, cap)
    if rc == _abi.E_NAN_INF:
        raise IllegalStateException("NaN or Infinity")
    if rc < 0:
        raise TsdbHipError(int(rc), "tsdbhip_format_points")
    return buf.raw[:rc].decode()
