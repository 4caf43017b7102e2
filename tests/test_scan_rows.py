"""tsdbhip_scan_rows: the rows TsdbQuery.getScanner's Scanner delivers (the
start / stop keys and createAndSetFilter's key regexp, TsdbQuery.java:368-492).

CPU: the host restatement core.scan_rows against the literal regexp and the
literal key compare; the scan times; the argument errors; the struct layouts
from C; the shared host checks under the host sanitizers. GPU: the C-ABI call
on host and device tables with both key loaders, exact against core.scan_rows,
at the sizes, offsets and lengths where the match kernel changes path; the
errors; and a whole query from a compacted table on."""
import ctypes as C
import functools
import json
import os
import re
import shutil
import subprocess
import types

import numpy as np
import pytest

from helpers import T0, U32MAX, assert_same
from opentsdb_amd import _abi, compaction, core, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W3 = (3, 3, 3)
W188 = (1, 8, 8)
METRIC = 9
SENTINEL = 0xA5
REGION = 4096  # k_scanrows.hip SR_REGION: a wave's LDS bytes
ALPHABET = bytes([0x00, 0x01, 0x0A, 0x0D, ord("\\"), ord("E"), ord("|"), ord("."), 0xFF])


def metric_of(w, metric=METRIC):
    return metric.to_bytes(w[0], "big")


def key(ts, tags, w=W3, metric=METRIC):
    b = (metric if isinstance(metric, bytes) else metric.to_bytes(w[0], "big")) + int(ts).to_bytes(4, "big")
    for k, v in tags:
        b += (k if isinstance(k, bytes) else k.to_bytes(w[1], "big"))
        b += (v if isinstance(v, bytes) else v.to_bytes(w[2], "big"))
    return b


# ------------------------------------------------------- the literal scanner ----
def filter_regexp(w, tags, group_bys, group_by_values):
    """the pattern createAndSetFilter builds (TsdbQuery.java:433-492), re.escape for \\Q...\\E"""
    mw, nw, vw = w
    pair = nw + vw
    pat = b"^.{%d}" % (mw + 4)
    tags, gbs = list(tags), list(group_bys)
    while tags or gbs:
        pat += b"(?:.{%d})*" % pair
        if tags and (not gbs or tags[0][0] < gbs[0]):  # isTagNext
            n, v = tags.pop(0)
            pat += re.escape(n) + re.escape(v)
        else:
            g = gbs.pop(0)
            ids = (group_by_values or {}).get(g)
            pat += re.escape(g)
            pat += b".{%d}" % vw if not ids else b"(?:" + b"|".join(re.escape(x) for x in ids) + b")"
    pat += b"(?:.{%d})*$" % pair
    return re.compile(pat, re.S)


def literal_scan(keys, w, metric, tags, group_bys, group_by_values, start, end, interval):
    """the Scanner, literally: start_key <= key < stop_key on the full key
    bytes (bytes compare: unsigned, the shorter first), then the regexp"""
    t0, t1 = core.scan_times(start, end, interval)
    lo, hi = metric + t0.to_bytes(4, "big"), metric + t1.to_bytes(4, "big")
    rx = filter_regexp(w, tags, group_bys, group_by_values) if (tags or group_bys) else None
    return [i for i, k in enumerate(keys) if lo <= k < hi and (rx is None or rx.search(k))]


def rand_id(rng, n):
    return bytes(ALPHABET[int(x)] for x in rng.integers(0, len(ALPHABET), n))


def random_case(rng, w, big_list=False):
    """(keys, query): keys with 0..8 pairs of repeated, unsorted names over the
    alphabet; the query mostly drawn from the first key, so that it matches
    about as often as not"""
    mw, nw, vw = w
    metric = rand_id(rng, mw)
    near = metric[:-1] + bytes([(metric[-1] + 1) & 0xFF])  # a byte-wise neighbour
    names = [rand_id(rng, nw) for _ in range(3)]
    keys = []
    for j in range(5):
        nt = int(rng.integers(0, 9))
        pairs = [(names[int(rng.integers(0, 3))] if rng.random() < 0.8 else rand_id(rng, nw), rand_id(rng, vw))
                 for _ in range(nt)]
        if j and rng.random() < 0.5:  # a variation of the first key
            pairs = list(keys_pairs0)
            if pairs and rng.random() < 0.5:
                pairs.pop(int(rng.integers(0, len(pairs))))
            if len(pairs) < 8 and rng.random() < 0.5:
                pairs.insert(int(rng.integers(0, len(pairs) + 1)), (rand_id(rng, nw), rand_id(rng, vw)))
        if j == 0:
            keys_pairs0 = pairs
        m = metric if rng.random() < 0.85 else (near if rng.random() < 0.5 else rand_id(rng, mw))
        keys.append(key(T0 + 3600 * int(rng.integers(0, 4)), pairs, w, m))
    # items: a strictly ascending choice of the first key's names, in key order
    items, last = [], None
    for n, v in keys_pairs0:
        if (last is None or n > last) and rng.random() < 0.6:
            items.append((n, v))
            last = n
    if rng.random() < 0.15:
        items = sorted({rand_id(rng, nw): rand_id(rng, vw) for _ in range(int(rng.integers(1, 4)))}.items())
    tags, gbs, gbv = [], [], {}
    for n, v in items:
        kind = int(rng.integers(0, 4))
        v = v if rng.random() < 0.85 else rand_id(rng, vw)
        if kind == 0:
            tags.append((n, v))
        else:
            gbs.append(n)
            if kind >= 2:
                nv = 1024 if big_list else (1 if kind == 2 else 2)
                ids = [rand_id(rng, vw) for _ in range(nv)]
                ids[int(rng.integers(0, nv))] = v
                gbv[n] = ids
    start = T0 + int(rng.integers(0, 4 * 3600)) if rng.random() < 0.5 else 0
    end = None if rng.random() < 0.5 else T0 + int(rng.integers(0, 4 * 3600))
    q = dict(tags=tags, group_bys=gbs, group_by_values=gbv, start_time=start, end_time=end,
             interval=int(rng.integers(0, 2)) * 3600)
    return metric, keys, q


CPU_WIDTHS = [(3, 3, 3), (1, 1, 1), (2, 1, 2), (1, 2, 1), (1, 8, 8)]


@pytest.mark.parametrize("w", CPU_WIDTHS, ids=str)
def test_host_model_against_literal_regexp(w):
    rng = np.random.default_rng(sum(w) * 101 + w[0])
    n_keys = n_sel = 0
    seen = {"list1": 0, "list2": 0, "list1024": 0, "filter": 0, "other_metric": 0}
    for case in range(1500):
        metric, keys, q = random_case(rng, w, big_list=case % 60 == 0)
        got = core.scan_rows(keys, metric, q["tags"], q["group_bys"], q["group_by_values"], q["start_time"],
                             q["end_time"], q["interval"], *w)
        exp = literal_scan(keys, w, metric, q["tags"], q["group_bys"], q["group_by_values"], q["start_time"],
                           q["end_time"], q["interval"])
        assert got == exp, (case, keys, q)
        n_keys += len(keys)
        n_sel += len(got)
        for ids in q["group_by_values"].values():
            seen["list%d" % len(ids)] += 1
        seen["filter"] += bool(q["tags"] or q["group_bys"])
        seen["other_metric"] += sum(k[:w[0]] != metric for k in keys)
    assert all(seen.values()), seen
    assert 0.1 <= n_sel / n_keys <= 0.9, (n_sel, n_keys)


def test_filter_walk_edges():
    n1, n2, n3 = [(i).to_bytes(3, "big") for i in (1, 2, 3)]
    v = lambda i: i.to_bytes(3, "big")  # noqa: E731
    scan = lambda pairs, **q: core.scan_rows([key(T0, pairs)], metric_of(W3), **q) == [0]  # noqa: E731
    # a repeated name: the pair with the accepted value counts, wherever it stands
    assert scan([(1, 5), (1, 6)], tags=[(n1, v(6))])
    assert scan([(1, 6), (1, 5)], tags=[(n1, v(6))])
    # the items in name order, the pairs in any: 2 before 1 in the key does not match 1 then 2
    assert scan([(1, 5), (2, 6)], tags=[(n1, v(5)), (n2, v(6))])
    assert not scan([(2, 6), (1, 5)], tags=[(n1, v(5)), (n2, v(6))])
    assert scan([(2, 6), (1, 5), (2, 6)], tags=[(n1, v(5))], group_bys=[n2])
    # any value, a list, a list with duplicates
    assert scan([(3, 9)], group_bys=[n3])
    assert not scan([(2, 9)], group_bys=[n3])
    assert scan([(3, 9)], group_bys=[n3], group_by_values={n3: [v(8), v(9), v(9)]})
    assert not scan([(3, 7)], group_bys=[n3], group_by_values={n3: [v(8), v(9)]})
    # no filter: a key without tags is delivered; with one it is not
    assert scan([])
    assert not scan([], group_bys=[n3])
    # nine items: a valid query that matches nothing
    names = [(i).to_bytes(3, "big") for i in range(1, 10)]
    assert not scan([(i, 1) for i in range(1, 9)], tags=[(n, v(1)) for n in names[:4]], group_bys=names[4:])
    assert scan([(i, 1) for i in range(1, 9)], tags=[(n, v(1)) for n in names[:4]], group_bys=names[4:8])


def test_scan_times():
    m = metric_of(W3)
    sel = lambda bases, **q: core.scan_rows([key(b, [(1, 1)]) for b in bases], m, **q)  # noqa: E731
    lit = lambda bases, **q: literal_scan([key(b, [(1, 1)]) for b in bases], W3, m, [], [], {},  # noqa: E731
                                          q.get("start_time", 0), q.get("end_time"), q.get("interval", 0))
    both = lambda bases, **q: (sel(bases, **q), lit(bases, **q))  # noqa: E731
    # the start clamps at 0
    assert core.scan_times(0, 0) == (0, 3601) and core.scan_times(7199, 0)[0] == 0
    assert core.scan_times(7200, 0)[0] == 0 and core.scan_times(7201, 0)[0] == 1
    assert both([0, 1, 3600, 3601], start_time=0, end_time=0) == ([0, 1, 2], [0, 1, 2])
    assert both([0, 1, 2], start_time=7201, end_time=U32MAX - 4000) == ([1, 2], [1, 2])
    # an unsigned compare on either side of 2^31
    h = 1 << 31
    assert both([h - 3600, h - 1, h, h + 3600], start_time=h - 1 + 7200, end_time=h) == ([1, 2, 3], [1, 2, 3])
    assert both([h - 1, h, h + 1], start_time=0, end_time=h - 3601) == ([0], [0])
    # the wrap: end + 3601 + interval at 2^32 - 1, 2^32, 2^32 + 5
    top = (1 << 32) - 1
    assert core.scan_times(0, top - 3601) == (0, top)
    assert both([0, top - 1, top], start_time=0, end_time=top - 3601) == ([0, 1], [0, 1])
    assert core.scan_times(0, top - 3600) == (0, 0) and core.scan_times(0, top - 3600 + 5) == (0, 5)
    assert both([0, 4, 5, top], start_time=0, end_time=top - 3600) == ([], [])
    assert both([0, 4, 5, top], start_time=0, end_time=top - 3600 + 5) == ([0, 1], [0, 1])
    assert both([T0], start_time=T0, end_time=top - 3600 + 5) == ([], [])  # a stop below the start
    assert core.scan_times(0, top - 3700, 100) == (0, 0)  # the interval wraps it too
    # UNSET: up to but not including 0xFFFFFFFF
    assert both([top - 1, top], start_time=0, end_time=None) == ([0], [0])
    # the sample interval moves both bounds across a row boundary
    bases = [T0 - 3 * 3600, T0 - 2 * 3600, T0, T0 + 3600, T0 + 2 * 3600]
    assert both(bases, start_time=T0, end_time=T0 - 1) == ([1, 2], [1, 2])
    assert both(bases, start_time=T0, end_time=T0 - 1, interval=3600) == ([0, 1, 2, 3], [0, 1, 2, 3])


def test_argument_errors_and_their_order():
    m, k = metric_of(W3), [key(T0, [(1, 1)])]
    n = [(i).to_bytes(3, "big") for i in range(1, 11)]
    v = (1).to_bytes(3, "big")

    def err(**q):
        with pytest.raises(ValueError) as e:
            core.scan_rows(q.pop("rows", k), m, **q)
        return str(e.value)

    assert "width" in err(metric_width=0) and "width" in err(value_width=9)
    assert "MAX_TAGS tags" in err(tags=[(x, v) for x in n[:9]])
    assert "MAX_TAGS group_bys" in err(group_bys=n[:9])
    assert "tags not strictly ascending" in err(tags=[(n[1], v), (n[0], v)])
    assert "tags not strictly ascending" in err(tags=[(n[0], v), (n[0], v)])
    assert "group_bys not strictly ascending" in err(group_bys=[n[1], n[1]])
    assert "both in tags and in group_bys" in err(tags=[(n[0], v), (n[2], v)], group_bys=[n[1], n[2]])
    # the order: a width, the counts (tags first), the tags' order, the group_bys', the shared name, the rows
    assert "width" in err(name_width=0, tags=[(x, v) for x in n[:9]])
    assert "MAX_TAGS tags" in err(tags=[(x, v) for x in reversed(n[:9])], group_bys=n[:9])
    assert "MAX_TAGS group_bys" in err(tags=[(n[1], v), (n[0], v)], group_bys=n[:9])
    assert "tags not" in err(tags=[(n[1], v), (n[0], v)], group_bys=[n[1], n[0]])
    assert "group_bys not" in err(tags=[(n[0], v)], group_bys=[n[1], n[0]])
    assert "both" in err(tags=[(n[0], v)], group_bys=[n[0]], rows=[b"\0"])
    assert "row 1" in err(rows=[k[0], k[0] + b"\0", k[0][:5]])
    assert "row 0" in err(rows=[key(T0, [(i, 1) for i in range(9)])])


def test_struct_layout_matches_ctypes(tmp_path):
    """sizeof / offsetof of the two new structs, from C (gcc, C11, -Werror), == _abi.py's ctypes"""
    exe = str(tmp_path / "abi_check_scanrows")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "abi_check_scanrows.c"), "-o", exe], check=True)
    d = json.loads(subprocess.run([exe], capture_output=True, text=True, check=True).stdout)
    assert d["abi_version"] == _abi.ABI_VERSION == 8
    assert d["has_scan_rows"] == 1 and d["hot_scan_rows"] == _abi.HOT_SCAN_ROWS == 12
    assert d["scan_end_unset"] == _abi.SCAN_END_UNSET and d["max_tags"] == _abi.MAX_TAGS
    assert _abi.HOT_NAMES[_abi.HOT_SCAN_ROWS] == "k_sr_match"
    ctypes_of = {"tsdbhip_scan_query": _abi.ScanQuery, "tsdbhip_scan_sel": _abi.ScanSel}
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
    assert "tsdbhip_scan_rows" in _lib.EXPORTS
    hdr = open(os.path.join(ROOT, "include", "tsdbhip.h")).read()
    assert "#define TSDBHIP_ABI_VERSION 8" in hdr
    assert "#define TSDBHIP_HAS_SCAN_ROWS 1" in hdr
    assert "int tsdbhip_scan_rows(tsdbhip_ctx* ctx, const tsdbhip_scan_desc* table" in hdr


def test_host_checks_clean_under_asan_ubsan(tmp_path):
    """the argument checks, the query builder and the row test the kernels
    share (csrc/scanrows_host.h) as a stand-alone program under
    AddressSanitizer + UndefinedBehaviorSanitizer; any report aborts it"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "san_scanrows")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "san_scanrows.cc"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "scanrows host checks ok" in r.stdout


# ===================================================================== GPU ====
FIELDS = {"row_index": np.uint32, "key_off": np.uint64, "key_bytes": np.uint8, "row_status": np.uint8,
          "row_qual_off": np.uint64, "row_qual_len": np.uint32, "row_val_off": np.uint64, "row_val_len": np.uint32}


class Table:
    """a table: keys, optional status and made-up cells (only gathered)"""

    def __init__(self, keys, w=W3, status=True, cells=True, seed=0):
        self.keys, self.w, self.n = keys, w, len(keys)
        self.key_off = np.zeros(self.n + 1, np.uint64)
        if keys:
            self.key_off[1:] = np.cumsum([len(k) for k in keys])
        self.key_bytes = np.frombuffer(b"".join(keys), np.uint8).copy()
        rng = np.random.default_rng(77 + seed)
        self.status = rng.integers(0, 6, self.n).astype(np.uint8) if status else None  # (unread: any value)
        self.cells = None
        if cells:
            self.cells = (rng.integers(0, 1 << 40, self.n).astype(np.uint64), rng.integers(0, 999, self.n).astype(np.uint32),
                          rng.integers(0, 1 << 40, self.n).astype(np.uint64), rng.integers(0, 4000, self.n).astype(np.uint32))

    def expected(self, q):
        idx = np.array(core.scan_rows(self.keys, metric_of(self.w), *q_args(q), *self.w), np.int64)
        ks = [self.keys[i] for i in idx]
        e = {"row_index": idx.astype(np.uint32), "key_bytes": np.frombuffer(b"".join(ks), np.uint8),
             "key_off": np.concatenate([[0], np.cumsum([len(k) for k in ks])]).astype(np.uint64)}
        if self.status is not None:
            e["row_status"] = self.status[idx]
        if self.cells is not None:
            for f, a in zip(("row_qual_off", "row_qual_len", "row_val_off", "row_val_len"), self.cells):
                e[f] = a[idx]
        return e


def q_args(q):
    return (q.get("tags"), q.get("group_bys"), q.get("group_by_values"), q.get("start_time", 0), q.get("end_time"),
            q.get("interval", 0))


def query_of(q, w):
    return core.make_scan_query(*q_args(q), w[1], w[2])


def run_host(ctx, t, q, key_off=None, row_capacity=None, key_capacity=None):
    rcap = max(1, t.n) if row_capacity is None else row_capacity
    kcap = max(1, len(t.key_bytes)) if key_capacity is None else key_capacity
    sizes = {"key_off": rcap + 1, "key_bytes": max(1, kcap)}
    outs = {f: np.full(sizes.get(f, max(1, rcap)), SENTINEL, np.uint8).repeat(np.dtype(dt).itemsize).view(dt)
            for f, dt in FIELDS.items()}
    sq, keep = query_of(q, t.w)
    rc, sel = core.run_scan_rows(ctx, t.key_off if key_off is None else key_off, t.key_bytes, metric_of(t.w), sq,
                                 t.status, t.cells, *t.w, row_capacity=rcap, key_capacity=kcap, outputs=outs)
    return rc, sel


def run_device(ctx, t, q, key_off=None, row_capacity=None, key_capacity=None, shift=0):
    """the table as torch device tensors, each allocated at its exact size
    (the key bytes `shift` bytes into theirs), outputs on the device filled
    with the sentinel; returns (code, ScanSelection of host copies)"""
    import torch
    dev = torch.device("cuda", ctx.device)

    def up(a, lead=0):
        a = np.ascontiguousarray(a)
        x = torch.empty(max(1, a.nbytes + lead), dtype=torch.uint8, device=dev)
        x[lead:lead + a.nbytes] = torch.from_numpy(a.view(np.uint8).reshape(-1))
        return x

    rcap = max(1, t.n) if row_capacity is None else row_capacity
    kcap = max(1, len(t.key_bytes)) if key_capacity is None else key_capacity
    ko, kb = up(t.key_off if key_off is None else key_off), up(t.key_bytes, shift)
    st = None if t.status is None else up(t.status)
    cells = None if t.cells is None else [up(c) for c in t.cells]
    sizes = {"key_off": rcap + 1, "key_bytes": max(1, kcap)}
    t_out = {f: torch.full((sizes.get(f, max(1, rcap)) * np.dtype(dt).itemsize,), SENTINEL, dtype=torch.uint8, device=dev)
             for f, dt in FIELDS.items()}
    torch.cuda.synchronize(dev)
    sq, keep = query_of(q, t.w)
    rc, sel = core.run_scan_rows(ctx, ko.data_ptr(), kb.data_ptr() + shift, metric_of(t.w), sq,
                                 None if st is None else st.data_ptr(),
                                 None if cells is None else [c.data_ptr() for c in cells], *t.w, row_capacity=rcap,
                                 key_capacity=kcap, device=True, n_rows=t.n, key_nbytes=len(t.key_bytes),
                                 outputs={f: x.data_ptr() for f, x in t_out.items()})
    torch.cuda.synchronize(dev)
    host = {f: x.cpu().numpy().view(FIELDS[f]) for f, x in t_out.items()}
    return rc, core.ScanSelection(_abi.ScanSel(n_selected=sel.n_selected, key_used=sel.key_used), host, rc == 0)


def assert_selection(sel, exp, t):
    S = len(exp["row_index"])
    assert (sel.n_selected, sel.key_used) == (S, len(exp["key_bytes"]))
    if S == 0:
        assert int(sel.raw["key_off"][0]) == 0
        return
    for f in FIELDS:
        if f in exp:
            np.testing.assert_array_equal(getattr(sel, f), exp[f], err_msg=f)
            # nothing past what the call owns
            tail = sel.raw[f][len(exp[f]):]
            assert (tail.view(np.uint8) == SENTINEL).all(), f
        else:
            assert (sel.raw[f].view(np.uint8) == SENTINEL).all(), f


def assert_untouched(sel):
    for f in FIELDS:
        assert (sel.raw[f].view(np.uint8) == SENTINEL).all(), f


def check(ctx, t, q, **kw):
    """host and device tables, exact against core.scan_rows"""
    exp = t.expected(q)
    for run in (run_host, run_device):
        args = {k: v for k, v in kw.items() if run is run_device or k != "shift"}  # (a host table is staged: no shift)
        rc, sel = run(ctx, t, q, **args)
        assert rc == 0, ctx.last_error()
        assert_selection(sel, exp, t)
        tm = ctx.timing()
        assert tm.hot_kernel == _abi.HOT_SCAN_ROWS
        assert tm.alg_bytes > len(t.key_bytes)
    return exp


@pytest.fixture(params=["lanes", "lds"])
def loader(request, ctx):
    ctx.set_option("scan_rows_load", request.param)
    yield request.param
    ctx.set_option("scan_rows_load", "auto")


MARK, OTHER = 7, 8


def marked_keys(n, selected, w=W3, seed=0):
    """n keys of 1..5 pairs; tag 1 = MARK on the rows of `selected`, OTHER on the rest"""
    rng = np.random.default_rng(n * 7 + seed)
    selected = set(selected)
    keys = []
    for i in range(n):
        extra = sorted(rng.choice(np.arange(2, 8), int(rng.integers(0, 5)), replace=False).tolist())
        keys.append(key(T0 + 3600 * int(rng.integers(0, 3)),
                        [(1, MARK if i in selected else OTHER)] + [(e, int(rng.integers(0, 99))) for e in extra], w))
    return keys


@functools.lru_cache(maxsize=None)
def marked_table(n, which):
    sel = {"all": range(n), "none": [], "first": [0], "last": [n - 1], "every65": range(0, n, 65)}[which]
    return Table(marked_keys(n, sel), seed=n)


Q_MARK = dict(tags=[((1).to_bytes(3, "big"), MARK.to_bytes(3, "big"))])
SIZES = [1, 63, 64, 65, 256, 257, 1025, 3 * 1024 + 1]


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_sizes_and_selectivity(ctx, loader, n):
    for which in ("all", "none", "first", "last", "every65"):
        t = marked_table(n, which)
        exp = check(ctx, t, Q_MARK)
        want = {"all": n, "none": 0, "first": 1, "last": 1, "every65": (n + 64) // 65}[which]
        assert len(exp["row_index"]) == want
    check(ctx, marked_table(n, "none"), {})  # no filter: every row


@pytest.mark.gpu
def test_grid_stride(ctx, loader):
    """one block of 4 waves: a wave takes rows 64 w + 256 j; 600 rows are three rounds, the last one partial"""
    ctx.set_option("scan_rows_blocks", "1")
    try:
        check(ctx, marked_table(600, "every65"), Q_MARK)
        check(ctx, marked_table(257, "last"), Q_MARK)
    finally:
        ctx.set_option("scan_rows_blocks", "auto")
    with pytest.raises(Exception):
        ctx.set_option("scan_rows_blocks", "0")
    with pytest.raises(Exception):
        ctx.set_option("scan_rows_load", "regs")


@functools.lru_cache(maxsize=None)
def mixed_table(w, n=700):
    """rows of two metrics and a neighbour, four hours, repeated and unsorted names, 0..8 pairs"""
    rng = np.random.default_rng(sum(w) + n)
    nw, vw = w[1], w[2]
    nm = lambda i: int(i).to_bytes(nw, "big")  # noqa: E731
    vl = lambda i: int(i).to_bytes(vw, "big")  # noqa: E731
    keys = []
    for i in range(n):
        pairs = [(nm(rng.integers(1, 5)), vl(rng.integers(0, 6))) for _ in range(int(rng.integers(0, 9)))]
        m = METRIC + int(rng.choice([0, 0, 0, 1, 100]))
        keys.append(key(T0 + 3600 * int(rng.integers(0, 4)), pairs, w, m))
    return Table(keys, w, seed=n)


@pytest.mark.gpu
@pytest.mark.parametrize("w", [(3, 3, 3), (1, 1, 1), (2, 1, 4), (1, 8, 8)], ids=str)
def test_queries(ctx, loader, w):
    t = mixed_table(w)
    nw, vw = w[1], w[2]
    nm = lambda i: int(i).to_bytes(nw, "big")  # noqa: E731
    vl = lambda i: int(i).to_bytes(vw, "big")  # noqa: E731
    many = [vl(i) for i in [5, 2] + list(range(249, 51, -1))] * 6  # 1200 ids, duplicates, unsorted
    qs = [dict(group_bys=[nm(2)]),
          dict(tags=[(nm(1), vl(3))]),
          dict(tags=[(nm(1), vl(3))], group_bys=[nm(2), nm(3)], group_by_values={nm(3): [vl(i) for i in range(4)] + [vl(i) for i in range(100, 116)]}),
          dict(group_bys=[nm(2)], group_by_values={nm(2): [vl(5)]}),
          dict(group_bys=[nm(1), nm(2)], group_by_values={nm(1): [vl(5), vl(9)], nm(2): many}),
          dict(group_bys=[nm(3)], group_by_values={nm(3): many[:17]}, start_time=T0 + 3 * 3600),
          dict(start_time=T0 + 2 * 3600 + 1, end_time=T0 + 2 * 3600 - 2),
          dict(start_time=T0, end_time=T0, interval=3600),
          dict(start_time=T0, end_time=U32MAX - 3600),  # the wrap
          dict(tags=[(nm(i), vl(1)) for i in range(1, 6)], group_bys=[nm(i) for i in range(6, 10)])]  # nine items
    counts = [len(check(ctx, t, q)["row_index"]) for q in qs]
    assert all(c > 0 for c in counts[:8]) and counts[8:] == [0, 0], counts
    assert counts[6] < t.n / 2


def wave_of(total, w=W188):
    """64 keys at (1,8,8), 5 + 16 t bytes each with t in 0..8, `total` bytes in all, some of 8 tags"""
    T, rem = divmod(total - 64 * 5, 16)
    assert rem == 0 and 8 <= T <= 512
    ts = [8] * (T // 8) + ([T % 8] if T % 8 else [])
    ts += [0] * (64 - len(ts))
    rng = np.random.default_rng(total)
    rng.shuffle(ts)
    return [key(T0, [(j + 1, MARK if (i + j) % 3 == 0 else OTHER) for j in range(t)], w) for i, t in enumerate(ts)]


Q_MARK188 = dict(group_bys=[(2).to_bytes(8, "big")], group_by_values={(2).to_bytes(8, "big"): [MARK.to_bytes(8, "big")]})


@pytest.mark.gpu
@pytest.mark.parametrize("total,shift", [(REGION, 0), (REGION - 16, 15), (REGION, 1), (REGION - 16, 0),
                                         (REGION + 16, 0), (64 * 133, 0)])
def test_lds_region_seam(ctx, loader, total, shift):
    """the second wave's 64 keys, from the 16-byte line of their first byte on,
    take exactly the region (4096 + 0), one byte less (4080 + 15), one more
    (4096 + 1: the lane loads take that wave), and 16 less / more; the first
    wave's keys are a multiple of 16 bytes, so the device address of the
    second wave's first byte is `shift` mod 16"""
    keys = wave_of(64 * 21) + wave_of(total) + wave_of(64 * 37)[:40]
    t = Table(keys, W188, seed=total + shift)
    assert int(t.key_off[64]) % 16 == 0 and int(t.key_off[128] - t.key_off[64]) == total
    exp = check(ctx, t, Q_MARK188, shift=shift)
    assert 0 < len(exp["row_index"]) < t.n


@pytest.mark.gpu
@pytest.mark.parametrize("shift", [0, 1, 15])
def test_key_offsets_mod_16(ctx, loader, shift):
    """the first key of every wave at any offset mod 16; the table's last key
    ends at key_nbytes, 1 mod 16, in a device buffer of exactly that size"""
    keys = marked_keys(300, range(0, 300, 3), seed=shift) + marked_keys(1, [0])
    while sum(len(k) for k in keys) % 16 != 1:
        keys += marked_keys(1, [0], seed=len(keys))
    t = Table(keys, seed=shift)
    assert len(t.key_bytes) % 16 == 1 and {int(o) % 16 for o in t.key_off[::64]} >= {0}
    exp = check(ctx, t, Q_MARK, shift=shift)
    assert exp["row_index"][-1] == t.n - 1


@pytest.mark.gpu
def test_bad_rows_report_the_first_and_write_nothing(ctx, loader):
    base = marked_keys(300, range(300))
    for at in (0, 299, 64 + 29):
        for what in ("short", "extra", "nine", "off"):
            keys = list(base)
            ko = None
            if what == "short":
                keys[at] = keys[at][:6]
            elif what == "extra":
                keys[at] = keys[at] + b"\0"
            elif what == "nine":
                keys[at] = key(T0, [(i, 1) for i in range(1, 10)])
            if at != 299:  # a later offender does not count
                keys[299] = keys[299] + b"\1\2"
            t = Table(keys)
            if what == "off":
                ko = t.key_off.copy()
                if at == 299:
                    ko[299] = ko[300] + 1
                    at_exp = (298, 299)
                else:
                    ko[at + 1] = 1 << 50
                    at_exp = (at,)
            else:
                at_exp = (at,)
            for run in (run_host, run_device):
                rc, sel = run(ctx, t, Q_MARK, key_off=ko)
                assert rc == _abi.E_INVALID_ARG, (what, at)
                assert any(f"row {a}" in ctx.last_error() for a in at_exp), (ctx.last_error(), what, at)
                assert (sel.n_selected, sel.key_used) == (0, 0)
                assert_untouched(sel)
    # key_off not ending at key_nbytes: before any row
    t = Table(base)
    ko = t.key_off.copy()
    ko[300] -= 1
    for run in (run_host, run_device):
        rc, sel = run(ctx, t, Q_MARK, key_off=ko)
        assert rc == _abi.E_INVALID_ARG and "key_off does not end" in ctx.last_error()
        assert_untouched(sel)


@pytest.mark.gpu
def test_capacity(ctx, loader):
    t = marked_table(257, "every65")
    exp = t.expected(Q_MARK)
    S, K = len(exp["row_index"]), len(exp["key_bytes"])
    for run in (run_host, run_device):
        for kw in (dict(row_capacity=S - 1, key_capacity=K), dict(row_capacity=S, key_capacity=K - 1)):
            rc, sel = run(ctx, t, Q_MARK, **kw)
            assert rc == _abi.E_CAPACITY, ctx.last_error()
            assert (sel.n_selected, sel.key_used) == (S, K)
            assert_untouched(sel)
        rc, sel = run(ctx, t, Q_MARK, row_capacity=S, key_capacity=K)  # exactly enough
        assert rc == 0, ctx.last_error()
        assert_selection(sel, exp, t)


@pytest.mark.gpu
def test_optional_arrays_and_arguments(ctx, loader):
    keys = marked_keys(130, range(0, 130, 2))
    for status, cells in ((False, False), (True, False), (False, True)):
        check(ctx, Table(keys, status=status, cells=cells), Q_MARK)
    t = Table(keys)
    rc, sel = run_host(ctx, Table([]), Q_MARK)
    assert rc == 0 and (sel.n_selected, sel.key_used) == (0, 0) and int(sel.raw["key_off"][0]) == 0
    n = [(i).to_bytes(3, "big") for i in range(1, 11)]
    v = (1).to_bytes(3, "big")
    bad = [(dict(tags=[(x, v) for x in n[:9]]), "tags"), (dict(group_bys=n[:9]), "group_bys"),
           (dict(tags=[(n[1], v), (n[0], v)]), "ascending"), (dict(group_bys=[n[1], n[1]]), "ascending"),
           (dict(tags=[(n[0], v)], group_bys=[n[0]]), "both")]
    for q, word in bad:
        for run in (run_host, run_device):
            rc, sel = run(ctx, t, q)
            assert rc == _abi.E_INVALID_ARG and word in ctx.last_error(), (q, ctx.last_error())
            assert_untouched(sel)
        with pytest.raises(ValueError):
            core.scan_rows(keys, metric_of(W3), *q_args(q))
    assert core.scan_rows_device(ctx, keys, metric_of(W3), *q_args(Q_MARK)) == list(range(0, 130, 2))


# ------------------------------------------------------------ end to end ----
@pytest.mark.gpu
def test_query_from_a_compacted_table(ctx):
    """compact_rows, then core.tsdb_query_run(device=True): scan_rows ->
    find_spans -> groupby_plan -> desc_gather -> run_batch, for dc=x,
    host=a|b|c, rack=*, downsampled sum, against query_run(device=False) over
    the rows the literal scanner selects; every group bit-exact"""
    rng = np.random.default_rng(21)
    DC, HOST, RACK = 1, 2, 3
    n_series, hours = 40, 3
    series = [[(DC, s % 2), (HOST, s % 5), (RACK, s % 3), (4, s)] for s in range(n_series)]
    series[7] = [(HOST, 1), (RACK, 2)]  # no dc
    series[8] = [(DC, 0), (HOST, 2)]    # no rack
    raw, keys = [], []
    for h in range(hours):
        for metric in (METRIC, METRIC + 1):
            for s in range(n_series):
                base = T0 + 3600 * h
                ts = sorted(rng.choice(3600, int(rng.integers(2, 7)), replace=False).tolist())
                pts = synth.points_int([base + x for x in ts], rng.integers(-500, 500, len(ts)).tolist())
                raw.append([(((x - base) << 4 | fl).to_bytes(2, "big"), vb) for x, fl, vb in pts])
                keys.append(key(base, series[s], W3, metric))
    res = compaction.compact_rows(ctx, compaction.pack_rows(raw))
    assert (res.status != _abi.ROW_NONE).all()
    table = [(k, core.KeyValue(int.from_bytes(k[3:7], "big"), *res.row(r)[1:])) for r, k in enumerate(keys)]
    b3 = lambda i: int(i).to_bytes(3, "big")  # noqa: E731
    tags, gbs, gbv = [(b3(DC), b3(0))], [b3(HOST), b3(RACK)], {b3(HOST): [b3(0), b3(1), b3(2)]}
    m = metric_of(W3)
    args = (T0 + 600, T0 + 3 * 3600, False, core.Aggregators.SUM, 300, core.Aggregators.SUM)
    got = core.tsdb_query_run(ctx, table, m, tags, gbs, gbv, *args, device=True)
    sel = literal_scan(keys, W3, m, tags, gbs, gbv, args[0], args[1], 300)
    assert 0 < len(sel) < len(keys) / 4
    assert sel == core.scan_rows(keys, m, tags, gbs, gbv, args[0], args[1], 300)
    exp = core.query_run(ctx, [table[i] for i in sel], m, gbs, *args, device=False)
    assert len(got) == len(exp) == 3 * 3
    for a, b in zip(got, exp):
        rc, ts, isi, bits, n_in, _ = b._run()
        assert rc == 0 and len(ts) > 3
        assert_same(a._run(), types.SimpleNamespace(code=rc, ts=ts, is_int=isi, bits=bits, n_input_points=n_in),
                    exact_double=True)
        assert [s.key for s in a.spans] == [s.key for s in b.spans]
        assert a.getTags() == b.getTags()
        # hosts 3 and 4 are in the table under dc 0 and nowhere in the answer
        assert all(core.get_value_id(s.key, b3(HOST), 3, 3, 3) in gbv[b3(HOST)] for s in a.spans)
