"""tsdbhip_desc_certify (k_desccert.hip): the count of unproven rows and the
flag TSDBHIP_DESC_QUALS_PROVEN against core.quals_proven, the host restatement
that tests/test_desc_certify_cpu.py holds to hand-built rows.

Every case row lies between proven neighbours, and the kernel is asked about
the whole table and about each case with its two neighbours alone (a view of
three rows of the same device arrays), so a miscounted row shows as that row.
The sources are uploaded as tests/test_desc_pack.py uploads them: qual_nbytes
ends at the last row and 64 bytes of 0xFF follow."""
import ctypes as C

import numpy as np
import pytest

import cert_cases as cc
import layouts
import test_layouts as tl
from layouts import relayout
from opentsdb_amd import _abi, core, packing, synth
from test_find_spans import to_device

pytestmark = pytest.mark.gpu
QP = _abi.DESC_QUALS_PROVEN


def upload(ctx, ss, lead=0):
    """`ss` as a device descriptor: nbytes end at the last row, the allocations
    go on for 64 bytes of 0xFF. lead: that many 0xFF bytes before the buffers'
    first byte, every offset moved up by it. Returns (desc, tensors)."""
    qn, vn = layouts.extents(ss)
    pad = np.full(lead, 0xFF, np.uint8)
    tail = np.full(64, 0xFF, np.uint8)
    host = {
        "span_row_start": ss.span_row_start, "row_base": ss.row_base, "row_ncells": ss.row_ncells,
        "row_qual_off": ss.row_qual_off + np.uint64(lead), "row_val_off": ss.row_val_off + np.uint64(lead),
        "row_val_len": ss.row_val_len,
        "qual_bytes": np.concatenate([pad, ss.qual_bytes[:qn], tail]),
        "val_bytes": np.concatenate([pad, ss.val_bytes[:vn], tail]),
    }
    t = {f: to_device(ctx, a) for f, a in host.items()}
    d = _abi.SgDesc()
    d.flags = _abi.DESC_DEVICE
    d.n_spans, d.n_rows = ss.n_spans, ss.n_rows
    for f, pt in tl.DESC_FIELDS:
        setattr(d, f, C.cast(C.c_void_p(t[f].data_ptr()), pt))
    d.qual_bytes = C.cast(C.c_void_p(t["qual_bytes"].data_ptr()), _abi.P8)
    d.val_bytes = C.cast(C.c_void_p(t["val_bytes"].data_ptr()), _abi.P8)
    d.qual_nbytes, d.val_nbytes = qn + lead, vn + lead
    return d, t


def rows_view(d, r0, n):
    """rows [r0, r0 + n) of the device descriptor `d` as a descriptor of their
    own (one span a row, as cert_cases.table builds them): the same arrays"""
    e = _abi.SgDesc()
    C.pointer(e)[0] = d
    e.n_spans = e.n_rows = n
    for f, pt in tl.DESC_FIELDS:
        w = C.sizeof(pt._type_)
        setattr(e, f, C.cast(C.c_void_p(C.cast(getattr(d, f), C.c_void_p).value + w * r0), pt))
    return e


def certify(ctx, d):
    rc, n = core.desc_certify(ctx, d)
    assert rc == 0, ctx.last_error()
    assert bool(d.flags & QP) == (n == 0)
    assert d.flags & _abi.DESC_DEVICE
    return n


# ---- 1. the cases, each between proven neighbours ----

SIZES = [2, 7, 8, 9, 63, 511, 512, 513, 1300]


def seams(n):
    """the first word (cells 0 and 1), a lane seam (cells 7 and 8), a chunk seam
    (cells 511 and 512), the last cell"""
    return sorted({c for c in (0, 1, 7, 8, 511, 512, n - 1) if c < n})


def case_rows():
    """[(name, words)]: the hand rows, then rows of SIZES cells on step 2 with
    one qualifier changed (delta + 1, float flag) at each seam"""
    rows = [(name, w) for name, w, _ in cc.hand_rows()]
    for n in SIZES:
        base = cc.quals(n, 3, 2)
        rows.append((f"{n} cells", base))
        for c in seams(n):
            rows.append((f"{n} cells, delta+1 at {c}", cc.changed(base, c, cc.DELTA["delta+1"])))
            rows.append((f"{n} cells, float-flag at {c}", cc.changed(base, c, cc.FLAGS["float-flag"])))
    return rows


CASES = case_rows()
# neighbour, case, neighbour, case, ..., neighbour: the neighbours of every size
NEIGHBOURS = [cc.quals(n, 1, 3) for n in (1, 2, 9, 64, 513, 1300)]


def case_table():
    rows = []
    for i, (_, w) in enumerate(CASES):
        rows += [NEIGHBOURS[i % len(NEIGHBOURS)], w]
    rows.append(NEIGHBOURS[len(CASES) % len(NEIGHBOURS)])
    return cc.table(rows)


CASE_SS = case_table()
_UP = {}


def source(ctx, name, lead=0):
    """the case table on a layout of layouts.NAMES, uploaded once"""
    k = (name, lead)
    if k not in _UP:
        ss = relayout(CASE_SS, name, seed=3)
        _UP[k] = (ss, *upload(ctx, ss, lead))
    return _UP[k]


def test_the_cases_hold_both_verdicts():
    ok = core.quals_proven(CASE_SS)
    assert ok[0::2].all()  # (the neighbours)
    assert ok[1::2].any() and not ok[1::2].all()
    # a change of cell 1 of a two-cell row only changes its step: still proven
    assert ok[1 + 2 * [n for n, _ in CASES].index("2 cells, delta+1 at 1")]


# the packer's layout; even qualifier offsets that are no multiple of 8; a shuffled row order with every even
# residue; back to back (tsdbhip_rows_out's placement)
@pytest.mark.parametrize("name,lead", [("packed", 0), ("q2", 0), ("q6", 6), ("mixed", 0), ("shuffled", 2), ("compact", 0),
                                       ("compact", 10)])
def test_count_and_flag(ctx, name, lead):
    ss, d, _ = source(ctx, name, lead)
    want = core.quals_proven(ss)
    assert certify(ctx, d) == int((~want).sum()) > 0 and not d.flags & QP
    tm = ctx.timing()
    assert tm.hot_kernel == _abi.HOT_DESC_CERTIFY and _abi.HOT_NAMES[tm.hot_kernel] == "k_desc_certify"
    for i, (cname, _) in enumerate(CASES):
        v = rows_view(d, 2 * i, 3)
        # (the view starts with the wrong flag: the call sets one that holds and clears one that does not)
        v.flags = _abi.DESC_DEVICE | (0 if want[2 * i + 1] else QP)
        assert certify(ctx, v) == (0 if want[2 * i + 1] else 1), f"{name} lead {lead}: {cname}"


def test_proven_table(ctx):
    rows = [w for (_, w), ok in zip(CASES, core.quals_proven(CASE_SS)[1::2]) if ok] + NEIGHBOURS
    for name in ("packed", "mixed"):
        d, _ = upload(ctx, relayout(cc.table(rows), name, seed=4))
        assert certify(ctx, d) == 0 and d.flags & QP
        assert core.desc_certify(ctx, d) == (0, 0) and d.flags & QP  # (a second proof)


def test_null_count_and_empty_table(ctx):
    ss, d, _ = source(ctx, "packed")
    e = rows_view(d, 0, 1)
    assert ctx._lib.tsdbhip_desc_certify(ctx.handle, C.byref(e), None) == 0 and e.flags & QP
    r = int(np.nonzero(~core.quals_proven(ss))[0][0])  # (an unproven row and its neighbours)
    e = rows_view(d, r - 1, 3)
    e.flags |= QP
    assert ctx._lib.tsdbhip_desc_certify(ctx.handle, C.byref(e), None) == 0 and not e.flags & QP
    e.n_spans = e.n_rows = 0
    assert core.desc_certify(ctx, e) == (0, 0) and e.flags & QP


# ---- 2. rows outside the buffer ----

def test_overrun_is_unproven_and_unread(ctx):
    """the row that ends the buffer: (a) three cells longer than it is, the
    overrun in the 64 bytes of 0xFF behind qual_nbytes; (b) qual_nbytes two
    bytes short of its end. Either way it counts, once, and (b) shows that the
    verdict is the bounds check's: the row's bytes are a proven row's."""
    rows = [cc.quals(40, 1, 2), cc.quals(1), cc.quals(700, 0, 5), cc.quals(512, 2, 1)]
    ss = cc.table(rows)
    assert core.quals_proven(ss).all()
    d, t = upload(ctx, ss)
    assert certify(ctx, d) == 0
    e = rows_view(d, 0, 4)
    e.qual_nbytes -= 2
    assert certify(ctx, e) == 1 == int((~core.quals_proven(ss, e.qual_nbytes)).sum())
    nc = ss.row_ncells.copy()
    nc[3] += 3
    long = packing.SpanSet(ss.span_row_start, ss.row_base, nc, ss.row_qual_off, ss.row_val_off, ss.row_val_len,
                           ss.qual_bytes, ss.val_bytes)
    t2 = to_device(ctx, nc)
    e = rows_view(d, 0, 4)
    e.row_ncells = C.cast(C.c_void_p(t2.data_ptr()), _abi.P32)
    assert certify(ctx, e) == 1 == int((~core.quals_proven(long, d.qual_nbytes)).sum())
    # an offset beyond the buffer, and an odd one (a one-cell row, proven anywhere else)
    off = ss.row_qual_off.copy()
    off[0] = np.uint64(1 << 40)
    off[1] += np.uint64(1)
    t3 = to_device(ctx, off)
    e = rows_view(d, 0, 4)
    e.row_qual_off = C.cast(C.c_void_p(t3.data_ptr()), _abi.P64)
    assert certify(ctx, e) == 2


# ---- 3. arguments ----

def test_host_descriptor(ctx):
    host = _abi.SgDesc()
    CASE_SS.fill_desc(host)
    host.flags = QP
    n = C.c_uint64(77)
    assert ctx._lib.tsdbhip_desc_certify(ctx.handle, C.byref(host), C.byref(n)) == _abi.E_INVALID_ARG
    assert "tsdbhip_desc_certify" in ctx.last_error()
    assert host.flags == QP and n.value == 77
    assert ctx._lib.tsdbhip_desc_certify(ctx.handle, None, None) == _abi.E_INVALID_ARG


# ---- 4. the producers ----

def test_synth_generate_sets_the_flag(ctx):
    for kind, n_points, step in ((_abi.SYN_INT64_COUNTER, 700, 1), (_abi.SYN_FLOAT32, 700, 10)):
        d = _abi.SgDesc()
        p = _abi.SynthParams(seed=7, n_spans=64, n_points=n_points, t0=synth.T0, step=step, kind=kind, span0=0)
        ctx.check(ctx._lib.tsdbhip_synth_generate(ctx.handle, C.byref(p), C.byref(d)))
        try:
            assert d.flags & QP and d.flags & _abi.DESC_DEVICE
            assert core.desc_certify(ctx, d) == (0, 0) and d.flags & QP
        finally:
            ctx._lib.tsdbhip_synth_free(ctx.handle, C.byref(d))


def test_desc_pack_proves_its_output(ctx):
    good = relayout(cc.table([cc.quals(n, 1, 3) for n in (1, 2, 9, 64, 513, 1300)]), "mixed", seed=6)
    bad = relayout(cc.table([cc.quals(9), cc.changed(cc.quals(600, 0, 2), 300, cc.DELTA["delta+1"]), cc.quals(64)]),
                   "mixed", seed=6)
    dg, _ = upload(ctx, good)
    db, _ = upload(ctx, bad)
    with core.PackedDesc(ctx, dg) as out:  # an unflagged proven table
        assert out.flags & QP and not dg.flags & QP
        assert ctx.timing().hot_kernel == _abi.HOT_DESC_PACK  # (the call's timing stays the copy's)
    with core.PackedDesc(ctx, db) as out:  # one bad row
        assert not out.flags & QP
    with core.PackedDesc(ctx, db, [2, 0]) as out:  # ... left out of the order
        assert out.flags & QP
    db.flags |= QP  # a flagged input: the promise is handed on, not proven again
    with core.PackedDesc(ctx, db) as out:
        assert out.flags & QP
        assert core.desc_certify(ctx, out) == (0, 1) and not out.flags & QP


def test_desc_gather_keeps_the_flag(ctx):
    ss, d, _ = source(ctx, "packed")
    order = np.asarray([2, 0], np.uint32)
    for flag in (QP, 0):
        e = rows_view(d, 0, 3)
        e.flags |= flag
        g = _abi.SgDesc()
        ctx.check(ctx._lib.tsdbhip_desc_gather(ctx.handle, C.byref(e), _abi.ptr(order, C.c_uint32), 2, C.byref(g)))
        try:
            assert (g.flags & QP) == flag
            assert core.desc_certify(ctx, g) == (0, 0) and g.flags & QP  # (rows 2 and 0: the neighbours)
        finally:
            ctx._lib.tsdbhip_desc_gather_free(ctx.handle, C.byref(g))
