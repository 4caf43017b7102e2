"""tsdbhip_desc_pack: device rows repacked to packing.pack_spans' layout.

The defining property is checked byte for byte: for a device descriptor on
any layout of tests/layouts.py and any order of its spans, the eight arrays of
the packed descriptor are what pack_spans returns for the same rows, the 64
bytes behind each byte buffer are zero, and the source is unchanged. The
sources are uploaded as test_layouts.device_desc uploads them: qual_nbytes /
val_nbytes end at the last row and 64 bytes of 0xFF follow, so a byte taken
from outside a row shows as a non-zero gap, a NaN or a -1.

Then what the call is for: the chain of test_chain_at_kernel_path_size, which
runs on the general path from tsdbhip_compact_rows' placement, takes the
uniform, lockstep and direct aligned-group kernels once it is packed."""
import ctypes as C
import threading

import numpy as np
import pytest

import layouts
import test_layouts as tl
import value_domains as vd
from helpers import U32MAX, with_option
from layouts import NAMES, relayout
from opentsdb_amd import _abi, compaction, core, packing, synth
from test_find_spans import W3, Scan, key, to_device

pytestmark = pytest.mark.gpu

SUM, MIN, MAX, AVG, DEV = 0, 1, 2, 3, 4
LOADS = ["unaligned", "shift"]


@pytest.fixture(params=LOADS)
def load(request):
    yield from with_option(request, "desc_pack_load", request.param, "auto")


# ---- uploading, packing, downloading ----

def upload(ctx, ss, lead=0, ptr_shift=0):
    """`ss` as a device descriptor: nbytes end at the last row, the allocations
    go on for 64 bytes of 0xFF. lead: that many 0xFF bytes before the buffers'
    first byte, every offset moved up by it (a first row at offset `lead`).
    ptr_shift: the descriptor's byte pointers that far into the allocations and
    the offsets back down by it (a first row at offset lead - ptr_shift of a
    buffer that does not begin on a dword). Returns (desc, tensors, host copies
    of what was uploaded)."""
    qn, vn = layouts.extents(ss)
    pad = np.full(lead, 0xFF, np.uint8)
    tail = np.full(64, 0xFF, np.uint8)
    host = {
        "span_row_start": ss.span_row_start, "row_base": ss.row_base, "row_ncells": ss.row_ncells,
        "row_qual_off": ss.row_qual_off + np.uint64(lead - ptr_shift),
        "row_val_off": ss.row_val_off + np.uint64(lead - ptr_shift), "row_val_len": ss.row_val_len,
        "qual_bytes": np.concatenate([pad, ss.qual_bytes[:qn], tail]),
        "val_bytes": np.concatenate([pad, ss.val_bytes[:vn], tail]),
    }
    t = {f: to_device(ctx, a) for f, a in host.items()}
    d = _abi.SgDesc()
    d.flags = _abi.DESC_DEVICE
    d.n_spans, d.n_rows = ss.n_spans, ss.n_rows
    for f, pt in tl.DESC_FIELDS:
        setattr(d, f, C.cast(C.c_void_p(t[f].data_ptr()), pt))
    d.qual_bytes = C.cast(C.c_void_p(t["qual_bytes"].data_ptr() + ptr_shift), _abi.P8)
    d.val_bytes = C.cast(C.c_void_p(t["val_bytes"].data_ptr() + ptr_shift), _abi.P8)
    d.qual_nbytes, d.val_nbytes = qn + lead - ptr_shift, vn + lead - ptr_shift
    return d, t, host


def download(ctx, d, slack=0):
    """the eight arrays of a device descriptor; the byte buffers to nbytes + slack"""
    e = _abi.SgDesc()
    C.pointer(e)[0] = d
    e.qual_nbytes, e.val_nbytes = d.qual_nbytes + slack, d.val_nbytes + slack
    R = int(d.n_rows)
    a = dict(span_row_start=np.zeros(d.n_spans + 1, np.uint64), row_base=np.zeros(R, np.uint32),
             row_ncells=np.zeros(R, np.uint32), row_qual_off=np.zeros(R, np.uint64), row_val_off=np.zeros(R, np.uint64),
             row_val_len=np.zeros(R, np.uint32), qual_bytes=np.zeros(e.qual_nbytes, np.uint8),
             val_bytes=np.zeros(e.val_nbytes, np.uint8))
    ctx.check(ctx._lib.tsdbhip_desc_download(ctx.handle, C.byref(e), *[v.ctypes.data_as(C.c_void_p) for v in a.values()]))
    return a


def assert_unchanged(t, host):
    for f, a in host.items():
        np.testing.assert_array_equal(t[f].cpu().numpy().view(a.dtype), a, err_msg=f"the source's {f} changed")


def assert_packed(ctx, out, spans, what):
    """the packed descriptor `out` against pack_spans of the same spans"""
    ref = packing.pack_spans(spans)
    assert (out.n_spans, out.n_rows, out.span0) == (ref.n_spans, ref.n_rows, 0), what
    assert out.flags & _abi.DESC_DEVICE
    assert (out.qual_nbytes, out.val_nbytes) == (len(ref.qual_bytes), len(ref.val_bytes)), what
    got = download(ctx, out, 64)
    for f in ("span_row_start", "row_base", "row_ncells", "row_qual_off", "row_val_off", "row_val_len"):
        np.testing.assert_array_equal(got[f], getattr(ref, f), err_msg=f"{what}: {f}")
    for f in ("qual_bytes", "val_bytes"):
        exp = np.concatenate([getattr(ref, f), np.zeros(64, np.uint8)])
        bad = np.nonzero(got[f] != exp)[0]
        assert not len(bad), f"{what}: {f} differs at {len(bad)} bytes, first at {int(bad[0])} of {len(exp)}: " \
                             f"{int(got[f][bad[0]]):#x}, wanted {int(exp[bad[0]]):#x}"


# ---- 1. bytes ----

# value lengths at the instruction (1 KB), piece (4 KB) and several-piece edges; a row's qualifiers are 2 n bytes
# with n = ceil(len / 8): 1026, 2050 and 8194 B are the same edges of the 8-byte qualifier units (512 B, 2 KB)
EDGE_LENS = [17, 0, 1, 15, 16, 1023, 1024, 1025, 4095, 4096, 4097, 8193, 32769]
# (cells, value bytes) around the small-row limit (both aligned extents at most 64 B: a lane copies the row;
# else it is a row of pieces): both extents at the limit, one past it on either side, one far past it
SMALL_EDGES = [(32, 64), (32, 49), (33, 16), (2, 65), (29, 64), (33, 65), (1, 4096), (600, 8)]
SPAN_ROWS = [0, 1, 2, 70, 0, 3]  # rows a span


def edge_group():
    """spans of 0, 1, 2 and 70 rows; the rows' lengths are EDGE_LENS, then
    SMALL_EDGES, then small random ones (on both sides of the small-row limit),
    the last row 29 value bytes (its last unit is partly the row's, partly what
    follows the buffer)"""
    rng = np.random.default_rng(41)
    R = sum(SPAN_ROWS)
    lens = [((vl + 7) // 8, vl) for vl in EDGE_LENS] + SMALL_EDGES
    lens += [((int(x) + 7) // 8, int(x)) for x in rng.integers(0, 100, R - len(lens) - 1)] + [(4, 29)]
    rows = [packing.KeyValue(int(rng.integers(0, 1 << 32)), rng.bytes(2 * n), rng.bytes(vl)) for n, vl in lens]
    spans, r = [], 0
    for k in SPAN_ROWS:
        spans.append(rows[r:r + k])
        r += k
    return spans


EDGE_SPANS = edge_group()
EDGE_SS = packing.pack_spans(EDGE_SPANS)
ORDERS = {
    "identity": None,
    "permutation": [3, 0, 5, 2, 1, 4],
    "reversed_subset": [5, 3, 2, 0],
    "repeated": [2, 3, 1, 3, 4, 2],
}
_UP = {}


def edge_source(ctx, name):
    """the edge group on a layout of layouts.NAMES, or on `compact` with its
    first row at offset 1 (off1) or at offset 0 of buffers that begin 3 bytes
    into a dword (ptr3)"""
    if name not in _UP:
        if name == "off1":
            _UP[name] = upload(ctx, relayout(EDGE_SS, "compact", seed=5), lead=1)
        elif name == "ptr3":
            _UP[name] = upload(ctx, relayout(EDGE_SS, "compact", seed=5), lead=3, ptr_shift=3)
        else:
            _UP[name] = upload(ctx, relayout(EDGE_SS, name, seed=5))
    return _UP[name]


def test_edge_sources_cover_the_residues():
    """compact, mixed and vodd together: every value residue mod 16, qualifier
    residues 0..6; the first row of `compact` at offset 0, its last row ending
    at nbytes; off1 has odd qualifier offsets"""
    vres, qres = set(), set()
    for name in ("compact", "mixed", "vodd"):
        ss = relayout(EDGE_SS, name, seed=5)
        vres |= {int(x) % 16 for x, n in zip(ss.row_val_off, ss.row_val_len) if n}
        qres |= {int(x) % 8 for x, n in zip(ss.row_qual_off, ss.row_ncells) if n}
    assert vres == set(range(16)) and qres >= {0, 2, 4, 6}
    ss = relayout(EDGE_SS, "compact", seed=5)
    assert int(ss.row_val_off[0]) == 0 and int(ss.row_qual_off[0]) == 0 and int(ss.row_val_len[0]) == 17
    qn, vn = layouts.extents(ss)
    assert int(ss.row_val_off[-1]) + int(ss.row_val_len[-1]) == vn and int(ss.row_val_len[-1]) == 29
    assert int(ss.row_qual_off[-1]) + 2 * int(ss.row_ncells[-1]) == qn


@pytest.mark.parametrize("name", [n for n in NAMES if n != "packed"] + ["off1", "ptr3"])
def test_bytes(ctx, load, name):
    d, t, host = edge_source(ctx, name)
    for oname, order in ORDERS.items():
        with core.PackedDesc(ctx, d, order) as out:
            spans = [EDGE_SPANS[s] for s in (order if order is not None else range(len(EDGE_SPANS)))]
            assert_packed(ctx, out, spans, f"{name} {oname} {load}")
            tm = ctx.timing()
            assert tm.hot_kernel == _abi.HOT_DESC_PACK and tm.alg_bytes > out.qual_nbytes + out.val_nbytes
    assert_unchanged(t, host)


# ---- 2. the metadata agrees with tsdbhip_desc_gather ----

@pytest.mark.parametrize("oname", [o for o in ORDERS if o != "identity"])
def test_gather_agreement(ctx, oname):
    d, _, _ = edge_source(ctx, "mixed")
    order = np.asarray(ORDERS[oname], np.uint32)
    g = _abi.SgDesc()
    ctx.check(ctx._lib.tsdbhip_desc_gather(ctx.handle, C.byref(d), _abi.ptr(order, C.c_uint32), len(order), C.byref(g)))
    try:
        with core.PackedDesc(ctx, d, order) as out:
            assert (out.n_spans, out.n_rows) == (g.n_spans, g.n_rows)
            a, b = download(ctx, out), download(ctx, g)
            for f in ("span_row_start", "row_base", "row_ncells", "row_val_len"):
                np.testing.assert_array_equal(a[f], b[f], err_msg=f)
    finally:
        ctx._lib.tsdbhip_desc_gather_free(ctx.handle, C.byref(g))


# ---- 3. the point of it: the chain reaches the streaming kernels ----

@pytest.fixture
def lockstep_always(request):
    yield from with_option(request, "lockstep", "always", "on")


@pytest.fixture
def group_direct_always(request):
    yield from with_option(request, "group_direct", "always", "on")


def test_chain_reaches_the_streaming_paths(ctx, lockstep_always, group_direct_always):
    """test_layouts.test_chain_at_kernel_path_size's chain (70 spans of one
    hourly row of 600 eight-byte cells through compact_rows and find_spans,
    values at 4801 r), uploaded and packed: the calls that chain makes with
    every streaming bit clear now set them, with no fallback bit, and the
    results (all integers) equal the oracle's bit for bit"""
    S, n = 70, 600
    g = vd.one_row("WRAP64", 2, S=S, n=n)
    tags = [[(1, s % 5), (2, s)] for s in range(S)]
    order = sorted(range(S), key=lambda s: core.span_cmp_key(key(synth.T0, tags[s])))
    base = g.spans[0][0].base_time
    raw, keys = [], []
    for i, s in enumerate(order):
        (kv,) = g.spans[i]
        raw.append([(kv.qualifier[2 * c:2 * c + 2], kv.value[8 * c:8 * c + 8]) for c in range(n)])
        keys.append(key(base, tags[s]))
    res = compaction.compact_rows(ctx, compaction.pack_rows(raw))
    np.testing.assert_array_equal(res.val_off, 4801 * np.arange(S, dtype=np.uint64))
    scan = Scan([(k, 0) for k in keys], W3, res.status, cells=False)
    scan.cells = (res.qual_off, res.qual_len, res.val_off, res.val_len)
    rc, fs = scan.run(ctx)
    assert rc == 0, ctx.last_error()
    qb = np.concatenate([res.qual, np.full(64, 0xFF, np.uint8)])
    vb = np.concatenate([res.val, np.full(64, 0xFF, np.uint8)])
    ss = packing.SpanSet(fs.span_row_start, fs.row_base, fs.row_ncells, fs.row_qual_off, fs.row_val_off,
                         fs.row_val_len, qb, vb)
    assert not layouts.rows_proposable(ss) and not layouts.rows_streamable(ss)
    d, _, _ = upload(ctx, ss)
    lg = tl.Laid.__new__(tl.Laid)
    lg.g, lg.name, lg.ss, lg.stream, lg.prop = g, "packed chain", g.ss, True, True
    fallbacks = tl.UFB | tl.DR | tl.GDF | tl.AR
    with core.PackedDesc(ctx, d) as out:
        assert_packed(ctx, out, g.spans, "chain")
        assert tl.ref(g, SUM).is_int.all() and tl.ref(g, AVG, False, 60, AVG).is_int.all()
        tl.expect(tl.check(ctx, lg, SUM, desc=out), tl.UNI | tl.LS, fallbacks | tl.GD, "packed chain sum")
        for ld, lines in (("lines_nt", tl.GDL), ("rows", 0)):
            ctx.set_option("group_direct_load", ld)
            try:
                p = tl.check(ctx, lg, AVG, False, 60, AVG, desc=out)
            finally:
                ctx.set_option("group_direct_load", "auto")
            # (the packer flags what it makes: the launch runs without the qualifier stream)
            tl.expect(p, tl.GD | tl.AG | tl.UNI | lines | _abi.PATH_QUALS_PROVEN, fallbacks | (tl.GDL ^ lines),
                      f"packed chain avg 60 {ld}")


# ---- 4. the batch over a packed descriptor ----

@pytest.mark.parametrize("name", ["compact", "mixed"])
@pytest.mark.parametrize("pool,kind", [("WRAP64", None), ("NAN_LATER", vd.F8)], ids=["WRAP64", "NAN_LATER"])
def test_pack_batch(ctx, pool, kind, name):
    """test_device_gather_batch with the pack in the gather's place"""
    g = vd.one_row(pool, 2, kind=kind)
    d = tl.device_desc(ctx, tl.laid(g, name))
    order = np.random.default_rng(8).permutation(g.n_spans).astype(np.uint32)
    with core.PackedDesc(ctx, d, order) as out:
        assert out.n_spans == g.n_spans and out.n_rows == g.ss.n_rows
        spans_of = lambda lo, hi: packing.pack_spans([g.spans[int(s)] for s in order[lo:hi]])  # noqa: E731
        tl.batch_case(ctx, g, None, tl.BATCH_CUT, False, device_desc=out, span_of=spans_of, what=f"packed {name}")


# ---- 5. offsets beyond 2^32 ----

def peek(ctx, d, qo, qlen, vo, vlen):
    """qual_bytes[qo, qo + qlen) and val_bytes[vo, vo + vlen) of a device descriptor"""
    e = _abi.SgDesc()
    C.pointer(e)[0] = d
    e.n_spans = e.n_rows = 0
    e.qual_bytes = C.cast(C.c_void_p(C.cast(d.qual_bytes, C.c_void_p).value + qo), _abi.P8)
    e.val_bytes = C.cast(C.c_void_p(C.cast(d.val_bytes, C.c_void_p).value + vo), _abi.P8)
    e.qual_nbytes, e.val_nbytes = qlen, vlen
    a = download(ctx, e)
    return a["qual_bytes"], a["val_bytes"]


@pytest.mark.timeout(60)  # (0.3 s on its first run: generating, packing and two queries over 5.4 GB; the limit is for a loaded box)
def test_beyond_4_gib(ctx):
    """150,000 spans of one row of 3600 eight-byte points: 4.32 GB of values, so
    the last rows' new offsets, the scans behind them and the copy's addresses
    need their 64 bits"""
    S, n = 150_000, 3600
    d = _abi.SgDesc()
    p = _abi.SynthParams(seed=5, n_spans=S, n_points=n, t0=synth.T0, step=1, kind=_abi.SYN_INT64_COUNTER, span0=0)
    ctx.check(ctx._lib.tsdbhip_synth_generate(ctx.handle, C.byref(p), C.byref(d)))
    try:
        assert d.val_nbytes > 1 << 32
        with core.PackedDesc(ctx, d) as out:
            assert (out.n_spans, out.n_rows) == (S, S)
            R = S
            meta = [np.zeros(R + 1, np.uint64), np.zeros(R, np.uint32), np.zeros(R, np.uint32), np.zeros(R, np.uint64),
                    np.zeros(R, np.uint64), np.zeros(R, np.uint32)]
            for desc, arrs in ((out, meta), (d, None)):
                e = _abi.SgDesc()
                C.pointer(e)[0] = desc
                e.qual_nbytes = e.val_nbytes = 16  # (the byte buffers are looked at row by row below)
                a = arrs or [np.zeros_like(x) for x in meta]
                qb, vb = np.zeros(16, np.uint8), np.zeros(16, np.uint8)
                ctx.check(ctx._lib.tsdbhip_desc_download(ctx.handle, C.byref(e),
                                                         *[x.ctypes.data_as(C.c_void_p) for x in a + [qb, vb]]))
                if arrs is None:
                    src = a
            qoff, voff, qn, vn = core.pack_offsets(meta[2], meta[5])
            np.testing.assert_array_equal(meta[3], qoff)
            np.testing.assert_array_equal(meta[4], voff)
            assert (out.qual_nbytes, out.val_nbytes) == (qn, vn) and int(voff[-1]) > 1 << 32
            np.testing.assert_array_equal(meta[2], src[2])
            np.testing.assert_array_equal(meta[5], src[5])
            for r in (R - 3, R - 2, R - 1):
                ql, vl = 2 * int(meta[2][r]), int(meta[5][r])
                gq, gv = peek(ctx, out, int(qoff[r]), ql, int(voff[r]), vl)
                sq, sv = peek(ctx, d, int(src[3][r]), ql, int(src[4][r]), vl)
                assert ql == 2 * n and vl == 8 * n + 1
                np.testing.assert_array_equal(gq, sq, err_msg=f"row {r} qualifiers")
                np.testing.assert_array_equal(gv, sv, err_msg=f"row {r} values")
            a = core.run_spanset(ctx, None, 0, U32MAX, SUM, False, 60, SUM, device_desc=out, capacity=4096)
            b = core.run_spanset(ctx, None, 0, U32MAX, SUM, False, 60, SUM, device_desc=d, capacity=4096)
            assert a[0] == b[0] == 0 and len(a[1]) == 60 and a[4] == b[4] == S * n
            for x, y in zip(a[1:4], b[1:4]):
                np.testing.assert_array_equal(x, y)
    finally:
        ctx._lib.tsdbhip_synth_free(ctx.handle, C.byref(d))


# ---- 6. errors and lifetime ----

def pack_raw(ctx, d, order, n, out):
    arr = None if order is None else np.ascontiguousarray(order, np.uint32)
    return ctx._lib.tsdbhip_desc_pack(ctx.handle, C.byref(d), None if arr is None else _abi.ptr(arr, C.c_uint32), n,
                                      C.byref(out))


def sentinel():
    out = _abi.SgDesc()
    C.memset(C.byref(out), 0x5A, C.sizeof(out))
    return out, bytes(out)


def test_argument_errors(ctx):
    d, _, _ = edge_source(ctx, "compact")
    S = d.n_spans
    host = _abi.SgDesc()
    EDGE_SS.fill_desc(host)
    host.flags = 0
    sharded = _abi.SgDesc()
    C.pointer(sharded)[0] = d
    sharded.flags |= _abi.SHARDED
    for what, src, order, n in (("a host descriptor", host, None, S), ("TSDBHIP_SHARDED", sharded, None, S),
                                ("order[1] out of range", d, [0, S, 1], 3), ("order[1] far out of range", d, [0, U32MAX], 2),
                                ("a null order with n != n_spans", d, None, S - 1),
                                ("a null order with n = 0", d, None, 0)):
        out, before = sentinel()
        assert pack_raw(ctx, src, order, n, out) == _abi.E_INVALID_ARG, what
        assert "tsdbhip_desc_pack" in ctx.last_error(), what
        assert bytes(out) == before, what
    assert ctx._lib.tsdbhip_desc_pack(ctx.handle, C.byref(d), None, S, C.byref(d)) == _abi.E_INVALID_ARG  # in == out
    assert d.n_spans == S


@pytest.mark.parametrize("which", ["values", "qualifiers"])
def test_row_out_of_bounds(ctx, load, which):
    """the row that ends the source buffer, one byte past a shortened nbytes, in
    the middle of the order: the message names its gathered index"""
    d, t, host = edge_source(ctx, "compact")
    e = _abi.SgDesc()
    C.pointer(e)[0] = d
    if which == "values":
        e.val_nbytes -= 1
    else:
        e.qual_nbytes -= 1
    # the last row of span 5 is the source's last; spans 1 and 2 (3 rows) come first, then span 5's 3 rows
    order = [1, 2, 5, 3, 5]
    bad_row = 1 + 2 + 2
    out, before = sentinel()
    assert pack_raw(ctx, e, order, len(order), out) == _abi.E_INVALID_ARG
    assert f"gathered row {bad_row} " in ctx.last_error(), ctx.last_error()
    assert bytes(out) == before
    assert_unchanged(t, host)
    out2 = _abi.SgDesc()
    assert pack_raw(ctx, d, order, len(order), out2) == 0, ctx.last_error()  # (the full buffer: fine)
    ctx._lib.tsdbhip_desc_pack_free(ctx.handle, C.byref(out2))


def test_empty_order_and_free(ctx):
    d, _, _ = edge_source(ctx, "compact")
    out = _abi.SgDesc()
    assert pack_raw(ctx, d, [0], 0, out) == 0, ctx.last_error()
    assert (out.n_spans, out.n_rows, out.qual_nbytes, out.val_nbytes) == (0, 0, 16, 16)
    assert_packed(ctx, out, [], "n = 0")
    assert download(ctx, out)["span_row_start"].tolist() == [0]
    for _ in range(2):  # (a second free is harmless)
        assert ctx._lib.tsdbhip_desc_pack_free(ctx.handle, C.byref(out)) == 0
        for f in ("span_row_start", "row_base", "row_ncells", "row_qual_off", "row_val_off", "row_val_len", "qual_bytes",
                  "val_bytes"):
            assert not getattr(out, f), f
        assert (out.qual_nbytes, out.val_nbytes) == (0, 0)
    # packing over a live packed descriptor replaces it
    assert pack_raw(ctx, d, [3], 1, out) == 0 and pack_raw(ctx, d, [1, 2], 2, out) == 0
    assert_packed(ctx, out, [EDGE_SPANS[1], EDGE_SPANS[2]], "packed twice")
    ctx._lib.tsdbhip_desc_pack_free(ctx.handle, C.byref(out))


def test_packed_outlives_its_source(ctx):
    d = _abi.SgDesc()
    p = _abi.SynthParams(seed=7, n_spans=64, n_points=700, t0=synth.T0, step=1, kind=_abi.SYN_INT64_COUNTER, span0=0)
    ctx.check(ctx._lib.tsdbhip_synth_generate(ctx.handle, C.byref(p), C.byref(d)))
    try:
        want = core.run_spanset(ctx, None, 0, U32MAX, SUM, False, 60, AVG, device_desc=d, capacity=4096)
        order = np.arange(64, dtype=np.uint32)[::-1].copy()
        with core.PackedDesc(ctx, d, order) as out:
            ctx._lib.tsdbhip_synth_free(ctx.handle, C.byref(d))
            junk = to_device(ctx, np.full(1 << 20, 0xFF, np.uint8))  # (what the freed source may be reused for)
            got = core.run_spanset(ctx, None, 0, U32MAX, SUM, False, 60, AVG, device_desc=out, capacity=4096)
            del junk
        assert got[0] == want[0] == 0 and got[4] == want[4] == 64 * 700
        for x, y in zip(got[1:4], want[1:4]):
            np.testing.assert_array_equal(x, y)
    finally:
        ctx._lib.tsdbhip_synth_free(ctx.handle, C.byref(d))


def test_four_threads_on_one_context(ctx):
    d, t, host = edge_source(ctx, "mixed")
    orders = [o for o in ORDERS.values()]
    outs = [_abi.SgDesc() for _ in orders]
    rcs = [None] * len(orders)

    def work(i):
        for _ in range(3):
            rcs[i] = pack_raw(ctx, d, orders[i], d.n_spans if orders[i] is None else len(orders[i]), outs[i])
            if rcs[i]:
                return

    ths = [threading.Thread(target=work, args=(i,)) for i in range(len(orders))]
    for th in ths:
        th.start()
    for th in ths:
        th.join()
    try:
        assert rcs == [0] * len(orders), ctx.last_error()
        for i, order in enumerate(orders):
            spans = [EDGE_SPANS[s] for s in (order if order is not None else range(len(EDGE_SPANS)))]
            assert_packed(ctx, outs[i], spans, f"thread {i}")
    finally:
        for o in outs:
            ctx._lib.tsdbhip_desc_pack_free(ctx.handle, C.byref(o))
    assert_unchanged(t, host)
