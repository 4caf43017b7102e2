"""Device-side findSpans: tsdbhip_find_spans (the TreeMap<byte[], Span> under
SpanCmp that TsdbQuery.findSpans fills row by row, TsdbQuery.java:240-285,
594-621) for the rows of a scan in delivery order.

Yardstick: the reference's findSpans restated as core.find_spans, itself
checked here on the CPU against a brute-force TreeMap emulation
(functools.cmp_to_key over a literal transcription of SpanCmp.compare,
insertion in delivery order). Every comparison is on exact bytes and integers.

The GPU sizes are the smallest that cross the kernels' seams (opentsdb_amd/
csrc/k_findspans.hip, k_groupby.hip): a wave of 64 rows, the sort tile of
1024 positions, several tiles."""
import ctypes as C
import functools
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from helpers import I, T0, U32MAX, assert_same
from opentsdb_amd import _abi, compaction, core, packing, synth
from time_domains import EDGE_BASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W3 = (3, 3, 3)
WIDTHS = [(3, 3, 3), (2, 1, 4), (1, 8, 8)]
METRIC = 9
SENTINEL = 0xA5


def key(ts, tags, w=W3, metric=METRIC):
    """row key: metric | base_time(4) | (tagk tagv)*; tags as (name, value) ints or bytes"""
    b = metric.to_bytes(w[0], "big") + int(ts).to_bytes(4, "big")
    for k, v in tags:
        b += (k if isinstance(k, bytes) else k.to_bytes(w[1], "big"))
        b += (v if isinstance(v, bytes) else v.to_bytes(w[2], "big"))
    return b


def metric_of(w):
    return METRIC.to_bytes(w[0], "big")


# ------------------------------------------------------------ brute force ----
def span_cmp(a, b, metric_width):
    """SpanCmp.compare (TsdbQuery.java:602-621), literally"""
    length = min(len(a), len(b))
    i = 0
    while i < metric_width:
        if a[i] != b[i]:
            return (a[i] & 0xFF) - (b[i] & 0xFF)
        i += 1
    i += 4
    while i < length:
        if a[i] != b[i]:
            return (a[i] & 0xFF) - (b[i] & 0xFF)
        i += 1
    return len(a) - len(b)


def brute_find_spans(rows, metric, metric_width):
    """a TreeMap under SpanCmp as a list kept sorted with the comparator: get,
    put of the first key, rows appended in delivery order"""
    entries, nrows = [], 0  # [key, rows]
    for k, kv in rows:
        assert k[:metric_width] == metric
        hit = next((e for e in entries if span_cmp(e[0], k, metric_width) == 0), None)
        if hit is None:
            hit = [k, []]
            entries.append(hit)
        if kv is not None:
            hit[1].append(kv)
            nrows += 1
    if nrows == 0:
        return None
    entries.sort(key=functools.cmp_to_key(lambda x, y: span_cmp(x[0], y[0], metric_width)))
    return [(e[0], e[1]) for e in entries]


def random_series(rng, n, w, max_tags=8, alphabet=(0x00, 0xFF, 0x01, 0x80)):
    """n distinct tag parts: 0..max_tags pairs of bytes from a small alphabet
    (0x00 and 0xFF included), and for some the same key extended by all-zero
    pairs (a prefix of another key)"""
    pair, out = w[1] + w[2], set()
    tries = 0
    while len(out) < n:
        tries += 1
        assert tries < 100 * n + 1000
        nt = int(rng.integers(0, max_tags + 1))
        t = bytes(rng.choice(alphabet, nt * pair).astype(np.uint8).tolist())
        out.add(t)
        if nt < max_tags and rng.random() < 0.4 and len(out) < n:
            out.add(t + b"\0" * (pair * int(rng.integers(1, max_tags - nt + 1))))
    return sorted(out)


def scan_rows(rng, n_rows, w, hours, series=None, order="hbase"):
    """exactly n_rows rows [(key, payload)] of `hours` hour blocks, series
    missing from some hours, delivered in HBase (full key) order, shuffled or
    in reverse time; the payload is the row's number in HBase order"""
    if series is None:
        series = random_series(rng, n_rows // hours + 3, w, max_tags=4)
    cells = [(h, s) for h in range(hours) for s in range(len(series))]
    assert len(cells) >= n_rows
    pick = sorted(rng.choice(len(cells), n_rows, replace=False).tolist())
    m = metric_of(w)
    keys = sorted(m + (T0 + 3600 * cells[c][0]).to_bytes(4, "big") + series[cells[c][1]] for c in pick)
    rows = [(k, i) for i, k in enumerate(keys)]
    if order == "shuffled":
        rows = [rows[i] for i in rng.permutation(len(rows))]
    elif order == "reverse":
        rows.sort(key=lambda r: (-int.from_bytes(r[0][w[0]:w[0] + 4], "big"), r[0]))
    return rows


# EDGE_BASES: base times 0, either side of 2^31 (0x7FFF... and 0x8000...) and the last hourly row below
# 2^32: the scan order and SpanCmp compare these key bytes unsigned, and row_base carries all 32 bits


def edge_base_rows(w, order, seed=11, n_series=40):
    """one scan whose rows sit at EDGE_BASES, some series missing from some hours"""
    rng = np.random.default_rng(seed)
    series = random_series(rng, n_series, w, max_tags=4)
    m = metric_of(w)
    keys = sorted(m + b.to_bytes(4, "big") + t for b in EDGE_BASES for t in series if rng.random() < 0.8)
    assert [k[w[0]] >> 7 for k in keys] == sorted(k[w[0]] >> 7 for k in keys)  # (0x80.. and 0xFF.. bases last)
    rows = [(k, i) for i, k in enumerate(keys)]
    if order == "shuffled":
        rows = [rows[i] for i in rng.permutation(len(rows))]
    elif order == "reverse":
        rows.sort(key=lambda r: (-int.from_bytes(r[0][w[0]:w[0] + 4], "big"), r[0]))
    return rows


# ===================================================================== CPU ====
@pytest.mark.parametrize("w", WIDTHS)
@pytest.mark.parametrize("order", ["hbase", "shuffled", "reverse"])
def test_host_model_edge_base_times(w, order):
    rows = edge_base_rows(w, order)
    assert {int.from_bytes(k[w[0]:w[0] + 4], "big") for k, _ in rows} == set(EDGE_BASES)
    got = core.find_spans(rows, metric_of(w), *w)
    exp = brute_find_spans(rows, metric_of(w), w[0])
    assert [(k, s.rows) for k, s in got.items()] == exp


@pytest.mark.parametrize("w", WIDTHS)
@pytest.mark.parametrize("order", ["hbase", "shuffled", "reverse"])
def test_host_model_against_brute_force(w, order):
    rng = np.random.default_rng(sum(w) * 7 + len(order))
    for trial in range(6):
        series = random_series(rng, 40, w)
        rows = scan_rows(rng, 90, w, 3, series, order)
        # None rows: first of their span, last, alone in their span, and random ones
        none = set(rng.choice(90, 12, replace=False).tolist())
        by_span = {}
        for i, (k, _) in enumerate(rows):
            by_span.setdefault(core.span_cmp_key(k, w[0]), []).append(i)
        groups = list(by_span.values())
        none |= {groups[0][0], groups[1][-1]} | set(groups[2])
        rows = [(k, None if i in none else p) for i, (k, p) in enumerate(rows)]
        got = core.find_spans(rows, metric_of(w), *w)
        exp = brute_find_spans(rows, metric_of(w), w[0])
        assert [(k, s.rows) for k, s in got.items()] == exp
        assert [s.key for s in got.values()] == [k for k, _ in exp]
        assert any(not r for _, r in exp)  # a span without rows exists


def test_host_model_edges():
    a, b = key(T0, [(1, 1)]), key(T0 + 3600, [(1, 1)])
    # the key of the first delivered row stays, with its base time
    got = core.find_spans([(b, "x"), (a, "y")], metric_of(W3))
    assert list(got) == [b] and got[b].rows == ["x", "y"] and got[b].key == b
    # no row added: null
    assert core.find_spans([], metric_of(W3)) is None
    assert core.find_spans([(a, None), (b, None)], metric_of(W3)) is None
    # a None row creates its span and can give it its key
    c = key(T0, [(1, 2)])
    got = core.find_spans([(b, None), (c, "z"), (a, "y")], metric_of(W3))
    assert list(got) == [b, c] and got[b].rows == ["y"]
    got = core.find_spans([(c, "z"), (a, None)], metric_of(W3))
    assert list(got) == [a, c] and got[a].rows == []
    # a prefix with an all-zero extension: the shorter key first
    p, q = key(T0, [(1, 1)]), key(T0, [(1, 1), (0, 0)])
    assert list(core.find_spans([(q, 1), (p, 2)], metric_of(W3))) == [p, q]
    with pytest.raises(core.IllegalDataException):
        core.find_spans([(a, 1), (key(T0, [(1, 1)], metric=METRIC + 1), 2)], metric_of(W3))


def test_struct_layout_matches_ctypes(tmp_path):
    """sizeof / offsetof of the two new structs, from C (gcc, C11, -Werror), == _abi.py's ctypes"""
    exe = str(tmp_path / "abi_check_findspans")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "abi_check_findspans.c"), "-o", exe], check=True)
    d = json.loads(subprocess.run([exe], capture_output=True, text=True, check=True).stdout)
    assert d["abi_version"] == _abi.ABI_VERSION == 8
    assert d["has_find_spans"] == 1 and d["hot_find_spans"] == _abi.HOT_FIND_SPANS == 11
    ctypes_of = {"tsdbhip_scan_desc": _abi.ScanDesc, "tsdbhip_spans_out": _abi.SpansOut}
    assert set(d["structs"]) == set(ctypes_of)
    for name, st in ctypes_of.items():
        c = d["structs"][name]
        assert c["size"] == C.sizeof(st), name
        assert [f[0] for f in st._fields_] == list(c["fields"]), name
        for fname, ftype in st._fields_:
            off, size = c["fields"][fname]
            assert getattr(st, fname).offset == off, (name, fname)
            assert C.sizeof(ftype) == size, (name, fname)


def test_export_and_header():
    from opentsdb_amd import _lib
    assert "tsdbhip_find_spans" in _lib.EXPORTS
    hdr = open(os.path.join(ROOT, "include", "tsdbhip.h")).read()
    assert "#define TSDBHIP_ABI_VERSION 8" in hdr
    assert "#define TSDBHIP_HAS_FIND_SPANS 1" in hdr
    assert "int tsdbhip_find_spans(tsdbhip_ctx* ctx, const tsdbhip_scan_desc* scan, tsdbhip_spans_out* out);" in hdr


def test_host_checks_clean_under_asan_ubsan(tmp_path):
    """the host-side validation and the per-row check the kernels share
    (csrc/findspans_host.h) as a stand-alone program under AddressSanitizer +
    UndefinedBehaviorSanitizer; any report aborts it"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "san_findspans")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "san_findspans.cc"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "findspans host checks ok" in r.stdout


# ===================================================================== GPU ====
class Scan:
    """the arrays of a scan: keys, optional status, made-up cells (even
    offsets and lengths: only passed through)"""

    def __init__(self, rows, w, status=None, cells=True, seed=0):
        self.rows, self.w, self.n = rows, w, len(rows)
        keys = [k for k, _ in rows]
        self.key_off = np.zeros(self.n + 1, np.uint64)
        if keys:
            self.key_off[1:] = np.cumsum([len(k) for k in keys])
        self.key_bytes = np.frombuffer(b"".join(keys), np.uint8).copy()
        self.status = None if status is None else np.asarray(status, np.uint8)
        rng = np.random.default_rng(1000 + seed)
        self.cells = None
        if cells:
            self.cells = (rng.integers(0, 1 << 40, self.n).astype(np.uint64) * np.uint64(2),
                          rng.integers(0, 500, self.n).astype(np.uint32) * np.uint32(2),
                          rng.integers(0, 1 << 40, self.n).astype(np.uint64),
                          rng.integers(0, 4000, self.n).astype(np.uint32))

    def model_rows(self):
        st = self.status
        return [(k, None if st is not None and st[i] == _abi.ROW_NONE else i) for i, (k, _) in enumerate(self.rows)]

    def expected(self):
        """every output array from core.find_spans, or None"""
        spans = core.find_spans(self.model_rows(), metric_of(self.w), *self.w)
        if spans is None:
            return None
        keys = list(spans)
        order = np.array([r for s in spans.values() for r in s.rows], np.int64)
        srs = np.concatenate([[0], np.cumsum([len(s.rows) for s in spans.values()])]).astype(np.uint64)
        mw = self.w[0]
        e = {"keys": keys, "row_order": order.astype(np.uint32), "span_row_start": srs,
             "row_base": np.array([int.from_bytes(self.rows[r][0][mw:mw + 4], "big") for r in order], np.uint32),
             "key_off": np.concatenate([[0], np.cumsum([len(k) for k in keys])]).astype(np.uint64),
             "key_bytes": np.frombuffer(b"".join(keys), np.uint8)}
        if self.cells is not None:
            e["row_qual_off"] = self.cells[0][order]
            e["row_ncells"] = self.cells[1][order] // 2
            e["row_val_off"] = self.cells[2][order]
            e["row_val_len"] = self.cells[3][order]
        return e

    def live_digits(self):
        """digit positions that differ between rows: the padded tag part and the tag count"""
        mw, pair = self.w[0], self.w[1] + self.w[2]
        P = _abi.MAX_TAGS * pair
        m = np.zeros((self.n, P + 1), np.uint8)
        for i, (k, _) in enumerate(self.rows):
            t = k[mw + 4:]
            m[i, :len(t)] = np.frombuffer(t, np.uint8)
            m[i, P] = len(t) // pair
        return int((m.min(0) != m.max(0)).sum())

    def run(self, ctx, **kw):
        return core.run_find_spans(ctx, self.key_off, self.key_bytes, metric_of(self.w), self.status, self.cells,
                                   *self.w, **kw)


def assert_found(fs, exp, scan):
    if exp is None:
        assert (fs.n_spans, fs.n_rows) == (0, 0)
        return
    S, R = len(exp["keys"]), len(exp["row_order"])
    assert (fs.n_spans, fs.n_rows, fs.n_skipped) == (S, R, scan.n - R)
    assert fs.key_used == len(exp["key_bytes"])
    assert fs.keys() == exp["keys"]
    for f in ("row_order", "span_row_start", "row_base", "key_off", "key_bytes", "row_qual_off", "row_ncells",
              "row_val_off", "row_val_len"):
        if f in exp:
            np.testing.assert_array_equal(getattr(fs, f), exp[f], err_msg=f)
        else:
            assert getattr(fs, f) is None


def check(ctx, scan, **kw):
    rc, fs = scan.run(ctx, **kw)
    assert rc == 0, ctx.last_error()
    assert_found(fs, scan.expected(), scan)
    t = ctx.timing()
    assert t.hot_kernel == _abi.HOT_FIND_SPANS
    assert t.n_grid == scan.live_digits()  # dead digits cost no launch
    return fs


@functools.lru_cache(maxsize=None)
def parity_scan(n, wi, hours):
    w = WIDTHS[wi]
    return Scan(scan_rows(np.random.default_rng(n * 31 + wi), n, w, hours), w, seed=n)


@pytest.mark.gpu
@pytest.mark.parametrize("n,wi,hours", [(1, 0, 1), (2, 1, 2), (63, 2, 3), (64, 0, 4), (65, 1, 5), (1023, 2, 1),
                                        (1024, 0, 2), (1025, 1, 3), (4099, 0, 5), (4099, 2, 4)])
def test_parity_with_host_model(ctx, n, wi, hours):
    fs = check(ctx, parity_scan(n, wi, hours))
    assert fs.n_spans <= n and fs.n_rows == n
    assert ctx.timing().alg_bytes > parity_scan(n, wi, hours).key_bytes.nbytes


@pytest.mark.gpu
@pytest.mark.parametrize("wi", [0, 1, 2])
@pytest.mark.parametrize("order", ["hbase", "shuffled", "reverse"])
def test_edge_base_times(ctx, wi, order):
    """row keys whose 4-byte base time is 0, 2^31 -+ an hour and the last hour
    below 2^32 in one scan: against core.find_spans, row_base included"""
    w = WIDTHS[wi]
    rows = edge_base_rows(w, order)
    fs = check(ctx, Scan(rows, w, seed=wi))
    assert set(fs.row_base.tolist()) == set(EDGE_BASES)
    # a scan of more than one 1024-row tile
    check(ctx, Scan(edge_base_rows(w, order, seed=12, n_series=700), w, seed=wi))


@pytest.mark.gpu
def test_keys_only(ctx):
    """the four cell arrays NULL: only the order, the boundaries and the keys"""
    w = W3
    s = Scan(scan_rows(np.random.default_rng(5), 300, w, 3), w, cells=False)
    fs = check(ctx, s)
    assert fs.row_ncells is None


@pytest.mark.gpu
def test_prefix_ties_and_extremes(ctx):
    w = (1, 8, 8)
    full = bytes(range(1, 129))  # 8 tags at widths (1,8,8): a 128-byte tag part
    tagparts = [
        b"",                                        # no tags at all
        b"\x01" * 16, b"\x01" * 16 + b"\0" * 16,    # A a prefix of B, B's extra pair all zero: A first
        b"\x01" * 16 + b"\0" * 112,                 # ... up to 8 pairs
        b"\0" * 16, b"\0" * 32,                     # all-zero keys of different lengths
        b"\xff" + b"\x01" * 15,                     # 0xFF in the most significant position
        full, full[:-1] + b"\xff", full[:-1] + b"\x00",  # ... and in the least significant one
        b"\xff" * 128,
    ]
    rng = np.random.default_rng(2)
    rows = [(metric_of(w) + (T0 + 3600 * h).to_bytes(4, "big") + t, 0) for h in range(2) for t in tagparts]
    rows = [rows[i] for i in rng.permutation(len(rows))]
    fs = check(ctx, Scan(rows, w))
    got = [k[5:] for k in fs.keys()]
    assert got == sorted(tagparts)
    assert got.index(b"\x01" * 16) + 1 == got.index(b"\x01" * 16 + b"\0" * 16)
    assert got[0] == b"" and got[-1] == b"\xff" * 128
    # the same at the default widths
    rows = [(key(T0, t), 0) for t in ([], [(1, 1)], [(1, 1), (0, 0)], [(0xFFFFFF, 0xFFFFFF)], [(1, 0xFFFFFF)],
                                      [(1, 1), (0, 0), (0, 0)], [(0, 0)])]
    fs = check(ctx, Scan(rows[::-1], W3))
    assert fs.keys() == sorted((k for k, _ in rows), key=core.span_cmp_key)


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["shuffled", "reverse"])
def test_stability(ctx, order):
    w = W3
    series = random_series(np.random.default_rng(3), 300, w, max_tags=4)
    base = scan_rows(np.random.default_rng(4), 1500, w, 5, series)
    moved = scan_rows(np.random.default_rng(4), 1500, w, 5, series, order)
    assert sorted(base) == sorted(moved) and base != moved
    fa, fb = check(ctx, Scan(base, w)), check(ctx, Scan(moved, w))
    # the same spans come out (the keys differ at most in the base time of the first delivered row)
    strip = lambda ks: [core.span_cmp_key(k, w[0]) for k in ks]  # noqa: E731
    assert strip(fa.keys()) == strip(fb.keys())
    np.testing.assert_array_equal(fa.span_row_start, fb.span_row_start)
    srs = fb.span_row_start.astype(np.int64)
    multi = 0
    for s in range(fb.n_spans):
        o = fb.row_order[srs[s]:srs[s + 1]].astype(np.int64)
        assert (np.diff(o) > 0).all()
        multi += len(o) > 1
    assert multi > 100


def sentinel_outputs(n, scap, kcap):
    mk = lambda dt, size: np.frombuffer(bytes([SENTINEL]) * (size * np.dtype(dt).itemsize), dt).copy()  # noqa: E731
    return {"row_order": mk(np.uint32, n), "span_row_start": mk(np.uint64, scap + 1), "row_base": mk(np.uint32, n),
            "row_ncells": mk(np.uint32, n), "row_qual_off": mk(np.uint64, n), "row_val_off": mk(np.uint64, n),
            "row_val_len": mk(np.uint32, n), "key_off": mk(np.uint64, scap + 1), "key_bytes": mk(np.uint8, kcap)}


def assert_untouched(fs):
    for f, a in fs.raw.items():
        assert (a.view(np.uint8) == SENTINEL).all(), f


def rejected(ctx, scan, code, words=(), **kw):
    outs = sentinel_outputs(max(1, scan.n), kw.get("span_capacity", max(1, scan.n)),
                            kw.get("key_capacity", max(1, scan.key_bytes.nbytes)))
    rc, fs = scan.run(ctx, outputs=outs, **kw)
    assert rc == code, (_abi.ERR_NAMES.get(rc, rc), ctx.last_error())
    for word in words:
        assert word in ctx.last_error(), ctx.last_error()
    assert_untouched(fs)
    return fs


@pytest.mark.gpu
def test_row_status(ctx):
    w = W3
    rows = scan_rows(np.random.default_rng(6), 700, w, 4)
    by_span = {}
    for i, (k, _) in enumerate(rows):
        by_span.setdefault(core.span_cmp_key(k, w[0]), []).append(i)
    groups = [g for g in by_span.values() if len(g) >= 2]
    st = np.full(700, _abi.ROW_SINGLE, np.uint8)
    st[np.random.default_rng(7).choice(700, 40, replace=False)] = _abi.ROW_NONE
    st[[1, 2]] = [_abi.ROW_TRIVIAL, _abi.ROW_COMPLEX]
    st[groups[0][0]] = _abi.ROW_NONE   # a span whose first row is NONE keeps that row's key
    st[groups[1][1:]] = _abi.ROW_SINGLE
    st[groups[2]] = _abi.ROW_NONE      # a span of only NONE rows
    scan = Scan(rows, w, st)
    fs = check(ctx, scan)
    n_none = int((st == _abi.ROW_NONE).sum())
    assert fs.n_skipped == n_none and fs.n_rows == 700 - n_none
    keys = fs.keys()
    assert rows[groups[0][0]][0] in keys
    s = keys.index(rows[groups[2][0]][0])
    assert fs.span_row_start[s] == fs.span_row_start[s + 1]
    # all rows NONE: OK, nothing found
    rc, fs = Scan(rows, w, np.zeros(700, np.uint8)).run(ctx)
    assert rc == 0 and (fs.n_spans, fs.n_rows, fs.n_skipped) == (0, 0, 700)
    # ERROR at row i, a foreign metric at row j: the lower row wins, in both arrangements
    for i, j in [(100, 500), (500, 100)]:
        st2 = st.copy()
        st2[i] = _abi.ROW_ERROR
        bad = list(rows)
        bad[j] = (key(T0, [(1, 1)], metric=METRIC + 1), 0)
        rejected(ctx, Scan(bad, w, st2), _abi.E_ILLEGAL_DATA, ["row %d" % min(i, j), "metric" if j < i else "ROW_ERROR"])
    # on one row the metric wins
    st2 = st.copy()
    st2[300] = _abi.ROW_OOB
    bad = list(rows)
    bad[300] = (key(T0, [(1, 1)], metric=METRIC + 1), 0)
    rejected(ctx, Scan(bad, w, st2), _abi.E_ILLEGAL_DATA, ["row 300", "metric"])
    rejected(ctx, Scan(rows, w, st2), _abi.E_OUT_OF_BOUNDS, ["row 300"])
    st2[300] = 9
    rejected(ctx, Scan(rows, w, st2), _abi.E_INVALID_ARG, ["row 300"])
    with pytest.raises(core.IllegalDataException):
        core.find_spans_device(ctx, bad, metric_of(w))
    with pytest.raises(core.IllegalDataException):
        core.find_spans(bad, metric_of(w))


@pytest.mark.gpu
def test_capacity(ctx):
    scan = parity_scan(1025, 1, 3)
    exp = scan.expected()
    S, K = len(exp["keys"]), len(exp["key_bytes"])
    for kw in ({"span_capacity": S - 1}, {"key_capacity": K - 1}):
        fs = rejected(ctx, scan, _abi.E_CAPACITY, **kw)
        assert (fs.n_spans, fs.n_rows, fs.n_skipped, fs.key_used) == (S, 1025, 0, K)
        # the retry with the reported sizes
        rc, again = scan.run(ctx, span_capacity=fs.n_spans, key_capacity=fs.key_used)
        assert rc == 0, ctx.last_error()
        assert_found(again, exp, scan)


def to_device(ctx, a):
    import torch
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    view = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(a.dtype)
    t = torch.from_numpy(a.view(view) if view else a).to(torch.device("cuda", ctx.device))
    return t


def run_device(ctx, scan, key_off=None, key_nbytes=None, n_rows=None, null=(), span_capacity=None,
               key_capacity=None, w=None, cells="scan", key_bytes=None, fill=0):
    """the scan as torch device tensors, outputs on the device; returns
    (code, FoundSpans of host copies, the device tensors)"""
    import torch
    dev = torch.device("cuda", ctx.device)
    n = scan.n if n_rows is None else n_rows
    kb = scan.key_bytes if key_bytes is None else key_bytes
    cells = scan.cells if cells == "scan" else cells
    t_in = {"key_off": to_device(ctx, scan.key_off if key_off is None else key_off),
            "key_bytes": to_device(ctx, kb if len(kb) else np.zeros(1, np.uint8)),
            "status": to_device(ctx, scan.status)}
    t_cells = None if cells is None else [to_device(ctx, c) for c in cells]
    scap = max(1, n) if span_capacity is None else span_capacity
    kcap = max(1, len(kb)) if key_capacity is None else key_capacity
    sizes = {"row_order": (torch.int32, n), "span_row_start": (torch.int64, scap + 1), "row_base": (torch.int32, n),
             "row_ncells": (torch.int32, n), "row_qual_off": (torch.int64, n), "row_val_off": (torch.int64, n),
             "row_val_len": (torch.int32, n), "key_off": (torch.int64, scap + 1), "key_bytes": (torch.uint8, kcap)}
    esz = {torch.int32: 4, torch.int64: 8, torch.uint8: 1}
    t_out = {f: torch.full((max(1, size) * esz[dt],), fill, dtype=torch.uint8, device=dev).view(dt)
             for f, (dt, size) in sizes.items()}  # (every byte = fill)
    torch.cuda.synchronize(dev)
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    rc, fs = core.run_find_spans(
        ctx, None if "key_off" in null else ptr(t_in["key_off"]), ptr(t_in["key_bytes"]), metric_of(scan.w),
        ptr(t_in["status"]), None if t_cells is None else [ptr(c) for c in t_cells], *(w or scan.w),
        span_capacity=scap, key_capacity=kcap, device=True, n_rows=n,
        key_nbytes=len(kb) if key_nbytes is None else key_nbytes,
        outputs={f: t.data_ptr() for f, t in t_out.items()})
    torch.cuda.synchronize(dev)
    host = {}
    for f, t in t_out.items():
        a = t.cpu().numpy()
        host[f] = a.view({np.dtype(np.int64): np.uint64, np.dtype(np.int32): np.uint32}.get(a.dtype, a.dtype))
    return rc, core.FoundSpans(_abi.SpansOut(n_spans=fs.n_spans, n_rows=fs.n_rows, n_skipped=fs.n_skipped,
                                             key_used=fs.key_used), host, rc == 0), (t_in, t_cells, t_out)


def invalid_cases(scan):
    """(label, kwargs for the changed call) of every invalid argument; scan: 300 rows at (3,3,3)"""
    w, rows = scan.w, scan.rows

    def with_rows(r, **kw):
        return dict(scan=Scan(r, w, scan.status, seed=0), **kw)

    short = list(rows)
    short[77] = (rows[77][0][:w[0] + 3], 0)
    extra = list(rows)
    extra[78] = (rows[78][0] + b"\0", 0)
    nine = list(rows)
    nine[79] = (key(T0, [(k, 1) for k in range(1, 10)]), 0)
    dec = scan.key_off.copy()
    dec[100] = dec[101] + 1
    qlen = scan.cells[1].copy()
    qlen[5] += 1
    qoff = scan.cells[0].copy()
    qoff[6] += 1
    c_len = (scan.cells[0], qlen, scan.cells[2], scan.cells[3])
    c_off = (qoff, scan.cells[1], scan.cells[2], scan.cells[3])
    return [("width 0", dict(w=(0, 3, 3)), ["width"]), ("width 9", dict(w=(3, 3, 9)), ["width"]),
            ("short key", with_rows(short), ["row 77"]), ("tag part + 1", with_rows(extra), ["row 78"]),
            ("9 pairs", with_rows(nine), ["row 79"]), ("key_off decreasing", dict(key_off=dec), ["row"]),
            ("key_off end", dict(key_nbytes=scan.key_bytes.nbytes + 4,
                                 key_bytes=np.concatenate([scan.key_bytes, np.zeros(4, np.uint8)])), ["key_off"]),
            ("odd qual_len", dict(cells=c_len), ["row 5"]), ("odd qual_off", dict(cells=c_off), ["row 6"]),
            ("null key_off", dict(null=("key_off",)), ["key_off"])]


@functools.lru_cache(maxsize=None)
def invalid_scan():
    st = np.full(300, _abi.ROW_SINGLE, np.uint8)
    st[[7, 8]] = _abi.ROW_NONE
    return Scan(scan_rows(np.random.default_rng(8), 300, W3, 3), W3, st)


@pytest.mark.gpu
def test_invalid_arguments_host(ctx):
    scan = invalid_scan()
    assert scan.run(ctx)[0] == 0
    for label, kw, words in invalid_cases(scan):
        s = kw.pop("scan", scan)
        outs = sentinel_outputs(300, 300, s.key_bytes.nbytes + 8)
        args = dict(key_off=s.key_off, key_bytes=kw.get("key_bytes", s.key_bytes), status=s.status,
                    cells=kw.get("cells", s.cells))
        if "key_off" in kw:
            args["key_off"] = kw["key_off"]
        if "null" in kw:
            args["key_off"] = None
        w = kw.get("w", s.w)
        rc, fs = core.run_find_spans(ctx, args["key_off"], args["key_bytes"], metric_of(s.w), args["status"],
                                     args["cells"], *w, outputs=outs, n_rows=300,
                                     key_nbytes=kw.get("key_nbytes"), span_capacity=300,
                                     key_capacity=s.key_bytes.nbytes + 8)
        assert rc == _abi.E_INVALID_ARG, (label, _abi.ERR_NAMES.get(rc, rc), ctx.last_error())
        for word in words:
            assert word in ctx.last_error(), (label, ctx.last_error())
        assert_untouched(fs)
    # an odd length and an odd offset on a NONE row are accepted
    qlen, qoff = scan.cells[1].copy(), scan.cells[0].copy()
    qlen[7] += 1
    qoff[8] += 1
    s2 = Scan(scan.rows, scan.w, scan.status)
    s2.cells = (qoff, qlen, scan.cells[2], scan.cells[3])
    check(ctx, s2)
    # no rows: OK
    rc, fs = Scan([], W3).run(ctx)
    assert rc == 0 and (fs.n_spans, fs.n_rows, fs.n_skipped) == (0, 0, 0)


@pytest.mark.gpu
def test_invalid_arguments_device(ctx):
    """the same checks run by the first kernel for a scan already in HBM"""
    scan = invalid_scan()
    rc, fs, _ = run_device(ctx, scan)
    assert rc == 0, ctx.last_error()
    assert_found(fs, scan.expected(), scan)
    for label, kw, words in invalid_cases(scan):
        s = kw.pop("scan", scan)
        rc, fs, _ = run_device(ctx, s, fill=SENTINEL, **kw)
        assert rc == _abi.E_INVALID_ARG, (label, _abi.ERR_NAMES.get(rc, rc), ctx.last_error())
        for word in words:
            assert word in ctx.last_error(), (label, ctx.last_error())
        assert_untouched(fs)
    off3 = scan.key_off.copy()
    off3[200] = scan.key_bytes.nbytes + 1000  # past the key bytes: never read
    rc, fs, _ = run_device(ctx, scan, key_off=off3, fill=SENTINEL)
    assert rc == _abi.E_INVALID_ARG and "row 199" in ctx.last_error()
    assert_untouched(fs)
    qlen, qoff = scan.cells[1].copy(), scan.cells[0].copy()
    qlen[7] += 1
    qoff[8] += 1
    rc, fs, _ = run_device(ctx, scan, cells=(qoff, qlen, scan.cells[2], scan.cells[3]))
    assert rc == 0, ctx.last_error()
    rc, fs, _ = run_device(ctx, Scan([], W3), n_rows=0)
    assert rc == 0 and (fs.n_spans, fs.n_rows) == (0, 0)
    # errors and capacity on the device leave the device arrays alone too
    st = scan.status.copy()
    st[150] = _abi.ROW_OOB
    rc, fs, _ = run_device(ctx, Scan(scan.rows, scan.w, st), fill=SENTINEL)
    assert rc == _abi.E_OUT_OF_BOUNDS and "row 150" in ctx.last_error()
    assert_untouched(fs)
    S = len(scan.expected()["keys"])
    rc, fs, _ = run_device(ctx, scan, span_capacity=S - 1, fill=SENTINEL)
    assert rc == _abi.E_CAPACITY and fs.n_spans == S
    assert_untouched(fs)


@pytest.mark.gpu
def test_device_resident(ctx):
    scan = parity_scan(4099, 0, 5)
    rc, fs, _ = run_device(ctx, scan)
    assert rc == 0, ctx.last_error()
    assert ctx.timing().h2d_bytes == 0
    assert_found(fs, scan.expected(), scan)
    rc, host = scan.run(ctx)
    assert rc == 0 and ctx.timing().h2d_bytes > 0
    for f in core.FoundSpans.FIELDS:
        np.testing.assert_array_equal(getattr(fs, f), getattr(host, f), err_msg=f)


# ---------------------------------------------------------------- the chain ----
def int_scan(n_rows, hours, seed, n_hosts=6, n_dcs=3):
    """rows [(key, KeyValue)] of integer series, tags host (name 1), dc (name
    2) and a unique id (name 3), in HBase order; a few points an hour"""
    rng = np.random.default_rng(seed)
    n_series = n_rows // hours + 3
    series = [[(1, 0x10 + int(rng.integers(0, n_hosts))), (2, int(rng.integers(0, n_dcs))), (3, s)]
              for s in range(n_series)]
    cells = [(h, s) for h in range(hours) for s in range(n_series)]
    pick = sorted(rng.choice(len(cells), n_rows, replace=False).tolist())
    rows = []
    for c in pick:
        h, s = cells[c]
        base = T0 + 3600 * h
        pts = [(base + 20 * i + s % 17, int(rng.integers(-1000, 1000))) for i in range(int(rng.integers(1, 5)))]
        kvs = I(pts)
        assert len(kvs) == 1
        rows.append((key(base, series[s]), kvs[0]))
    rows.sort(key=lambda r: r[0])
    return rows


@functools.lru_cache(maxsize=None)
def chain_rows():
    return int_scan(1025, 3, 12)


def results_of(groups):
    return [g._run() for g in groups]


def same_result(a, b):
    assert a[0] == b[0] == 0
    for x, y in zip(a[1:4], b[1:4]):
        np.testing.assert_array_equal(x, y)
    assert a[4] == b[4]


@pytest.mark.gpu
def test_chain_from_keys(ctx):
    """find_spans -> groupby_plan -> desc_gather -> spangroup_run_batch, all
    device-resident; only the plan comes back to the host in between"""
    import oracle
    rows = chain_rows()
    key_off, key_bytes, status, cells, qual, val = core._pack_scan(rows)
    scan = Scan(rows, W3, status)
    scan.cells = cells
    rc, fs, (t_in, t_cells, t_out) = run_device(ctx, scan)
    assert rc == 0, ctx.last_error()
    model = core.find_spans(rows, metric_of(W3))
    assert fs.keys() == list(model)
    gbs = [(1).to_bytes(3, "big"), (2).to_bytes(3, "big")]
    rc, plan = core.run_groupby_plan(ctx, t_out["key_off"].data_ptr(), t_out["key_bytes"].data_ptr(), gbs,
                                     device=True, n_spans=fs.n_spans, key_nbytes=fs.key_used)
    assert rc == 0, ctx.last_error()  # (no E_UNSORTED: the keys come out in SpanCmp order)
    gk, order, gss = core.plan_groups(list(model), gbs)
    assert plan.group_keys == gk and plan.order.tolist() == order and plan.group_span_start.tolist() == gss
    assert plan.n_groups > 4
    t_qual, t_val = to_device(ctx, qual), to_device(ctx, val)
    d = _abi.SgDesc()
    d.flags = _abi.DESC_DEVICE
    d.n_spans, d.n_rows = fs.n_spans, fs.n_rows
    for f, pt in (("span_row_start", _abi.P64), ("row_base", _abi.P32), ("row_ncells", _abi.P32),
                  ("row_qual_off", _abi.P64), ("row_val_off", _abi.P64), ("row_val_len", _abi.P32)):
        setattr(d, f, C.cast(C.c_void_p(t_out[f].data_ptr()), pt))
    d.qual_bytes, d.qual_nbytes = C.cast(C.c_void_p(t_qual.data_ptr()), _abi.P8), len(qual)
    d.val_bytes, d.val_nbytes = C.cast(C.c_void_p(t_val.data_ptr()), _abi.P8), len(val)
    g = _abi.SgDesc()
    o = np.ascontiguousarray(plan.order, np.uint32)
    ctx.check(ctx._lib.tsdbhip_desc_gather(ctx.handle, C.byref(d), _abi.ptr(o, C.c_uint32), len(o), C.byref(g)))
    try:
        ncells = np.array([len(kv.qualifier) // 2 for _, kv in rows], np.int64)
        span_cells = [int(sum(len(r.qualifier) // 2 for r in model[k].rows)) for k in model]
        caps = [max(1, sum(span_cells[i] for i in order[gss[q]:gss[q + 1]])) for q in range(len(gk))]
        assert sum(caps) == ncells.sum()
        for agg, ds in ((core.Aggregators.SUM, None), (core.Aggregators.AVG, (60, core.Aggregators.AVG))):
            rc, res = core.run_spanset_batch(ctx, None, plan.group_span_start, 0, U32MAX, agg.code, False,
                                             ds[0] if ds else 0, ds[1].code if ds else 0, capacities=caps,
                                             device_desc=g)
            assert rc == 0, ctx.last_error()
            host = core.group_by_and_aggregate(dict(model), gbs, 0, U32MAX, False, agg, ds[0] if ds else 0,
                                               ds[1] if ds else None, ctx=ctx)
            assert len(host) == len(res)
            for a, b in zip(res, results_of(host)):
                same_result(a, b)
        members = [model[list(model)[i]].rows for i in order[gss[1]:gss[2]]]
        rc, res = core.run_spanset_batch(ctx, None, plan.group_span_start, 0, U32MAX, 0, False, 0, 0,
                                         capacities=caps, device_desc=g)
        assert_same(res[1], oracle.spangroup(packing.pack_spans(members), 0, U32MAX, 0))
    finally:
        ctx._lib.tsdbhip_desc_gather_free(ctx.handle, C.byref(g))


@pytest.mark.gpu
def test_chain_from_raw_rows(ctx):
    """compact_rows -> find_spans -> a SpanGroup. Every qualifier here has an
    even length, and the one junk row holds two junk KVs whose odd qualifier
    lengths (1 + 3) add up to an even number, so every row's compacted
    qualifier offset is even, as tsdbhip_sg_desc requires."""
    rng = np.random.default_rng(14)
    n_series, hours = 50, 4
    tags = [[(1, s % 5), (2, s)] for s in range(n_series)]
    raw, keys, points = [], [], {s: [] for s in range(n_series)}
    junk_at = None
    for h in range(hours):
        for s in range(n_series):
            base = T0 + 3600 * h
            if h == 1 and s == 20:  # a row of only junk in the middle of span 20
                junk_at = len(raw)
                raw.append([(b"\x01", b"x"), (b"\x01\x02\x03", b"yz")])
                keys.append(key(base, tags[s]))
                continue
            ts = sorted(rng.choice(3600, int(rng.integers(2, 6)), replace=False).tolist())
            pts = synth.points_int([base + t for t in ts], rng.integers(-500, 500, len(ts)).tolist())
            points[s] += pts
            raw.append([(((t - base) << 4 | fl).to_bytes(2, "big"), vb) for t, fl, vb in pts])
            keys.append(key(base, tags[s]))
    assert len(raw) == 200
    batch = compaction.pack_rows(raw)
    res = compaction.compact_rows(ctx, batch)
    assert res.status[junk_at] == _abi.ROW_NONE and (res.status != _abi.ROW_NONE).sum() == 199
    assert (res.qual_off[res.status != _abi.ROW_NONE] % 2 == 0).all()
    scan = Scan([(k, 0) for k in keys], W3, res.status, cells=False)
    scan.cells = (res.qual_off, res.qual_len, res.val_off, res.val_len)
    rc, fs = scan.run(ctx)
    assert rc == 0, ctx.last_error()
    assert (fs.n_spans, fs.n_rows, fs.n_skipped) == (n_series, 199, 1)
    ss = packing.SpanSet(fs.span_row_start, fs.row_base, fs.row_ncells, fs.row_qual_off, fs.row_val_off,
                         fs.row_val_len, res.qual, res.val)
    order = sorted(range(n_series), key=lambda s: core.span_cmp_key(key(T0, tags[s])))
    ref = packing.pack_spans([synth.series_rows(points[s]) for s in order])
    assert ss.n_rows == ref.n_rows == 199
    for agg, ds in ((0, (0, 0)), (_abi.AGG_AVG, (60, _abi.AGG_AVG))):
        got = core.run_spanset(ctx, ss, 0, U32MAX, agg, False, ds[0], ds[1])
        exp = core.run_spanset(ctx, ref, 0, U32MAX, agg, False, ds[0], ds[1])
        same_result(got, exp)
        assert len(got[1]) > 100


@pytest.mark.gpu
def test_query_run_device(ctx):
    rows = chain_rows()
    gbs = [(1).to_bytes(3, "big"), (2).to_bytes(3, "big")]
    for agg, ds in ((core.Aggregators.SUM, None), (core.Aggregators.AVG, (60, core.Aggregators.AVG))):
        args = (rows, metric_of(W3), gbs, 0, U32MAX, False, agg, ds[0] if ds else 0, ds[1] if ds else None)
        dev = core.query_run(ctx, *args, device=True)
        host = core.query_run(ctx, *args, device=False)
        assert len(dev) == len(host) > 4
        for a, b in zip(dev, host):
            same_result(a._run(), b._run())
            assert a.getTags() == b.getTags() and a.getAggregatedTags() == b.getAggregatedTags()
            assert [s.key for s in a.spans] == [s.key for s in b.spans]
    assert core.query_run(ctx, [(rows[0][0], None)], metric_of(W3), gbs, 0, U32MAX, False, core.Aggregators.SUM,
                          device=True) == []
