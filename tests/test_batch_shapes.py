"""tsdbhip_spangroup_run_batch at the shapes where its segmented kernels
switch (tests/batch_shapes.py): tile groups (a wave carries cursors and cached
brackets over 2 and 3 tiles), span chunks (partials of 2 to 18 chunks, a short
last one, direct-only chunks next to chunks with E spans), 257 and 65 537
groups (block strides, binary searches over offsets that empty groups share),
bitmap words on rank-block edges and past 256 rank blocks, the wide-range
fallback, per-group capacities and lazy errors deep in a batch.

Every group is compared with the oracle on that group alone: integers,
timestamps, isInteger, aggregatedSize, codes and error indices exactly, doubles
at 1e-9 relative (bit-exact with EXACT_ORDER); one-cell groups, by the
thousand, against their closed form (which test_batch_shapes_cpu.py holds to
the oracle). test_batch_shapes_cpu.py asserts through a restatement of the
batch's host geometry that each case reaches the regime it is named for."""
import ctypes as C

import numpy as np
import pytest

import batch_shapes as bs
from helpers import assert_same
from opentsdb_amd import _abi, core
from opentsdb_amd._lib import Context

pytestmark = pytest.mark.gpu

AGGS = [0, 1, 2, 3, 4]
DS = [(0, 0), (60, 3)]
HOT_REDUCE_DIRECT = 5  # TSDBHIP_HOT_REDUCE_DIRECT (include/tsdbhip.h)


def run(ctx, c, agg, rate=False, ds=(0, 0), exact=False, capacities=None):
    rc, res = core.run_spanset_batch(ctx, c.ss, c.gss, c.start, c.end, agg, rate, ds[0], ds[1], exact=exact,
                                     capacities=c.capacities() if capacities is None else capacities)
    if rc in (_abi.E_HIP, _abi.E_RCCL):  # a device fault: nothing more runs on this GPU
        pytest.exit(f"{c.name} agg={agg} rate={rate} ds={ds} exact={exact}: {ctx.last_error()}", returncode=3)
    return rc, res


def assert_segmented(ctx, c, res, n_grid=None):
    """The batch just run took its own segmented pipeline, not the group-by-
    group rerun (which any error raised at group construction falls back to,
    and which leaves the last group's timing): tsdbhip_timing.n_grid is the
    grid of all groups together. n_grid: that sum, where every group is free
    of errors; None, with lazy errors in the batch (a failing group's grid is
    at least the points it delivered): at least the delivered points, which is
    more than the last group alone has."""
    got = ctx.timing().n_grid
    if n_grid is not None:
        assert got == n_grid, f"{c.name}: n_grid {got}, the groups' grids together {n_grid}"
        return
    delivered = sum(len(r[1]) for r in res)
    last = len(res[-1][1])
    assert got >= delivered > last, f"{c.name}: n_grid {got}, delivered {delivered}, last group {last}"


def grid_points(c, groups, agg, rate=False, ds=(0, 0)):
    """the grid points of error-free groups together (the oracle's n_out)"""
    return sum(len(c.ref(int(g), agg, rate, ds).ts) for g in groups)


def check_groups(c, res, groups, agg, rate=False, ds=(0, 0), exact=False):
    """the listed groups against the oracle; returns the first failing code among them"""
    first = 0
    for g in groups:
        g = int(g)
        o = c.ref(g, agg, rate, ds)
        try:
            assert_same(res[g], o, exact_double=exact)
            assert res[g][5] == o.err_index, f"err_index gpu={res[g][5]} oracle={o.err_index}"
        except AssertionError as e:
            raise AssertionError(f"{c.name} group {g} agg={agg} rate={rate} ds={ds} exact={exact}: {e}") from None
        first = first or o.code
    return first


def check_closed_form(c, res, groups, ts, isint, bits, n_input=1):
    """groups that emit one known point each (or, ts None, nothing), vectorised"""
    groups = [int(g) for g in groups]
    assert all(res[g][0] == 0 for g in groups), "a code"
    assert all(res[g][5] == -1 for g in groups), "an error index"
    assert all(res[g][4] == n_input for g in groups), "aggregatedSize"
    n = np.array([len(res[g][1]) for g in groups])
    if ts is None:
        assert (n == 0).all()
        return
    bad = np.nonzero(n != 1)[0]
    assert not len(bad), f"{c.name}: group {groups[bad[0]]} emitted {n[bad[0]]} points"
    for k, want in ((1, ts), (2, isint), (3, bits)):
        got = np.concatenate([res[g][k] for g in groups])
        ne = np.nonzero(got != want)[0]
        assert not len(ne), f"{c.name}: group {groups[ne[0]]} field {k}: gpu={got[ne[0]]} expected={want[ne[0]]}"


# ---- A: tile groups ----
def filler_expect(c, fill, agg):
    p = c.pt0[c.gss[fill].astype(np.int64)]
    isint = c.kinds[c.gss[fill].astype(np.int64)] < bs.KF4
    bits = np.where(isint, c.ival[p], c.fval[p].view(np.int64))
    return c.ts[p], isint.astype(np.uint8), np.zeros_like(bits) if agg == 4 else bits


@pytest.mark.parametrize("kind", bs.LONG_KINDS)
@pytest.mark.parametrize("pos", bs.POSITIONS)
def test_tile_groups(ctx, pos, kind):
    """two 3-span groups of ~4800 and ~8500 grid points (tpw 2 and 3) first,
    in the middle and last among 1000 one-cell groups"""
    c = bs.tile_groups(pos, kind)
    rate = kind == "rate"
    long = (c.meta["L1"], c.meta["L2"])
    fill = np.array([g for g in range(c.G) if g not in long])
    for ds in DS:
        for agg in AGGS:
            for exact in (False, True):
                rc, res = run(ctx, c, agg, rate, ds, exact)
                assert rc == 0
                assert_segmented(ctx, c, res, grid_points(c, long, agg, rate, ds) + (0 if rate else len(fill)))
                check_groups(c, res, long, agg, rate, ds, exact)
                if rate:  # a span of one point has no rate
                    check_closed_form(c, res, fill, None, None, None)
                else:
                    check_closed_form(c, res, fill, *filler_expect(c, fill, agg))


# ---- G: lazy errors deep in a batch ----
@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("agg", [0, 3])
def test_deep_lazy_errors(ctx, agg, exact):
    """a 3-byte long in one tile group and +Inf in the next, neither the
    batch's first group, each past its group's first 1024 bitmap words and in a
    tile beyond a wave's first tpw: err_index and n_out as the oracle's,
    every other group untouched"""
    c = bs.tile_groups("middle", "dual", True)
    long = (c.meta["L1"], c.meta["L2"])
    fill = np.array([g for g in range(c.G) if g not in long])
    rc, res = run(ctx, c, agg, exact=exact)
    assert_segmented(ctx, c, res)
    assert check_groups(c, res, long, agg, exact=exact) == rc == _abi.E_ILLEGAL_DATA
    assert [res[g][0] for g in long] == [_abi.E_ILLEGAL_DATA, _abi.E_NAN_INF]
    check_closed_form(c, res, fill, *filler_expect(c, fill, agg))


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("agg", [0, 3])
def test_deep_lazy_errors_plain(ctx, agg, exact):
    """the same two errors in 2-span groups of 100 000 s (no tile group):
    past the group's first 1024 bitmap words, in the batch's second and third
    group"""
    c = bs.deep_errors()
    rc, res = run(ctx, c, agg, exact=exact)
    assert_segmented(ctx, c, res)
    assert check_groups(c, res, range(c.G), agg, exact=exact) == rc == _abi.E_ILLEGAL_DATA
    assert [r[0] for r in res] == [0, _abi.E_ILLEGAL_DATA, _abi.E_NAN_INF, 0]


# ---- B: span chunks ----
@pytest.mark.parametrize("rate", [False, True])
@pytest.mark.parametrize("agg", AGGS)
def test_span_chunks(ctx, agg, rate):
    """groups of 33, 49, 97, 300 and 260 jittered spans: 2, 3, 6, 18 and 16 chunks"""
    c = bs.span_chunks()
    for ds in DS:
        for exact in (False, True):
            rc, res = run(ctx, c, agg, rate, ds, exact)
            assert_segmented(ctx, c, res, grid_points(c, range(c.G), agg, rate, ds))
            assert rc == 0 == check_groups(c, res, range(c.G), agg, rate, ds, exact)


@pytest.mark.parametrize("rate", [False, True])
@pytest.mark.parametrize("agg", AGGS)
def test_direct_chunks(ctx, agg, rate):
    """the same on wide hourly rows, where spans on one cadence skip E: groups
    whose chunks are all direct-only, direct-only around one chunk with an E
    span, and all E; 300 and 260 spans in 18 and 16 chunks, one of them E"""
    c = bs.direct_chunks()
    for exact in (False, True):
        rc, res = run(ctx, c, agg, rate, exact=exact)
        assert_segmented(ctx, c, res, grid_points(c, range(c.G), agg, rate))
        assert rc == 0 == check_groups(c, res, range(c.G), agg, rate, exact=exact)
        assert ctx.timing().hot_kernel == HOT_REDUCE_DIRECT  # k_direct_scan ran


# ---- C: many groups ----
@pytest.mark.parametrize("G,aggs", [(257, AGGS), (65537, [0, 4])])
def test_many_groups(ctx, G, aggs):
    c = bs.many_groups(G)
    role = c.meta["role"]
    plain, ts, isint, bits = bs.plain_expect(c)
    sample = np.random.default_rng(7).choice(plain, min(1000, len(plain)), replace=False)
    special = np.nonzero(role != 0)[0]
    outside = np.nonzero((role == 4) | (role == 5) | (role == 1))[0]
    caps = c.capacities()
    for agg in aggs:
        for exact in (False, True) if G < 1000 else (False,):
            rc, res = run(ctx, c, agg, exact=exact, capacities=caps)
            assert rc == 0
            assert_segmented(ctx, c, res, len(plain) + grid_points(c, special, agg))
            check_closed_form(c, res, plain, ts, isint.astype(np.uint8), np.zeros_like(bits) if agg == 4 else bits)
            check_closed_form(c, res, outside, None, None, None, n_input=0)
            check_closed_form(c, res, np.nonzero(role == 6)[0], None, None, None, n_input=2)
            assert check_groups(c, res, special, agg, exact=exact) == 0
            assert check_groups(c, res, sample, agg, exact=exact) == 0


# ---- D: bitmap words ----
@pytest.mark.parametrize("rate", [False, True])
@pytest.mark.parametrize("name", ["word_edges", "sparse_words"])
def test_bitmap_words(ctx, name, rate):
    c = getattr(bs, name)(rate)  # (rising values under rate: a sum of rates has positive terms)
    for agg in AGGS:
        for exact in (False, True):
            rc, res = run(ctx, c, agg, rate, exact=exact)
            assert_segmented(ctx, c, res, grid_points(c, range(c.G), agg, rate))
            assert rc == 0 == check_groups(c, res, range(c.G), agg, rate, exact=exact)


# ---- E: the wide-range fallback ----
@pytest.fixture
def own_ctx():
    """a context of the test's own: the wide grids grow its scratch for good"""
    c = Context(0)
    yield c
    c.close()


def test_wide_range_fallback(own_ctx):
    c = bs.wide_fallback()
    for agg in (0, 3):
        rc, res = run(own_ctx, c, agg)
        assert rc == 0 == check_groups(c, res, range(c.G), agg)
        # group by group: the call's timing is its last group's (the segmented path reports the batch's grid)
        assert own_ctx.timing().n_grid == len(c.ref(c.G - 1, agg).ts) < grid_points(c, range(c.G), agg)
    o = bs.ordinary()  # the next, ordinary batch on the same context
    for agg in AGGS:
        rc, res = run(own_ctx, o, agg)
        assert rc == 0 == check_groups(o, res, range(o.G), agg)
        assert_segmented(own_ctx, o, res, grid_points(o, range(o.G), agg))


def test_widest_segmented(own_ctx):
    """W = 2^27 - 1 words: the last batch before the fallback"""
    c = bs.wide_segmented()
    rc, res = run(own_ctx, c, 0)
    assert rc == 0 == check_groups(c, res, range(c.G), 0)
    assert_segmented(own_ctx, c, res, grid_points(c, range(c.G), 0))


# ---- F: per-group capacity ----
SENTINEL = 0x5A


def _bufs(cap):
    return (np.full(8 * cap, SENTINEL, np.uint8).view(np.int64), np.full(cap, SENTINEL, np.uint8),
            np.full(8 * cap, SENTINEL, np.uint8).view(np.int64))


def _desc(c, ss, agg):
    d = _abi.SgDesc()
    ss.fill_desc(d)
    d.flags = 0
    d.start_time, d.end_time, d.agg = c.start, c.end, agg
    return d


def _point(out, bufs):
    out.capacity = len(bufs[0])
    out.ts, out.is_int, out.bits = _abi.ptr(bufs[0], C.c_int64), _abi.ptr(bufs[1], C.c_uint8), _abi.ptr(bufs[2], C.c_int64)


def _fields(out):
    return int(out.err_code), int(out.n_out), int(out.n_input_points), int(out.err_index)


def raw_batch(ctx, c, agg, caps):
    """the batch into sentinel-filled buffers: (rc, [fields], [buffers])"""
    gss = np.ascontiguousarray(c.gss, np.uint32)
    outs = (_abi.SgOut * c.G)()
    bufs = [_bufs(int(k)) for k in caps]
    for g in range(c.G):
        _point(outs[g], bufs[g])
    d = _desc(c, c.ss, agg)
    rc = ctx._lib.tsdbhip_spangroup_run_batch(ctx.handle, C.byref(d), c.G, _abi.ptr(gss, C.c_uint32), outs)
    return rc, [_fields(outs[g]) for g in range(c.G)], bufs, int(ctx.timing().n_grid)


def raw_lone(ctx, c, g, agg, cap):
    ss = c.sub(g)
    out, bufs = _abi.SgOut(), _bufs(cap)
    _point(out, bufs)
    d = _desc(c, ss, agg)
    rc = ctx._lib.tsdbhip_spangroup_run(ctx.handle, C.byref(d), C.byref(out))
    return rc, _fields(out), bufs


@pytest.mark.parametrize("lazy", [False, True])
@pytest.mark.parametrize("agg", AGGS)
def test_group_capacity(ctx, agg, lazy):
    """one group with room for T - 1 points, another for exactly T: the first
    alone reports E_CAPACITY, every field and buffer as a lone
    tsdbhip_spangroup_run with that capacity leaves them; lazy: its error
    index lies below the capacity, so the lazy error is reported instead"""
    c = bs.capacity_groups(lazy)
    T = len(bs.capacity_groups(False).ref(bs.CAP_SHORT, agg).ts)
    caps = c.capacities().copy()
    caps[bs.CAP_SHORT] = T - 1
    caps[bs.CAP_EXACT] = len(c.ref(bs.CAP_EXACT, agg).ts)
    rc, fields, bufs, n_grid = raw_batch(ctx, c, agg, caps)
    # the segmented pipeline, not the group-by-group rerun: a capacity is applied when the results are
    # copied out and a lazy error travels with its group, so the grid is that of all six groups
    others = grid_points(c, [g for g in range(c.G) if g != bs.CAP_SHORT], agg)
    assert n_grid == others + T if not lazy else others + T >= n_grid > others
    lrc, lfields, lbufs = raw_lone(ctx, c, bs.CAP_SHORT, agg, T - 1)
    o = c.ref(bs.CAP_SHORT, agg, capacity=T - 1)
    want = _abi.E_ILLEGAL_DATA if lazy else _abi.E_CAPACITY
    assert rc == lrc == o.code == want, (rc, lrc, o.code)
    assert fields[bs.CAP_SHORT] == lfields, (fields[bs.CAP_SHORT], lfields)
    if lazy:
        assert lfields[1:] == (len(o.ts), o.n_input_points, o.err_index) and lfields[3] == lfields[1] < T - 1
    else:
        assert lfields[1] == 0
    for a, b in zip(bufs[bs.CAP_SHORT], lbufs):
        np.testing.assert_array_equal(a, b)
    n = lfields[1]
    assert all((a[n:].view(np.uint8) == SENTINEL).all() for a in bufs[bs.CAP_SHORT])  # untouched past n_out
    for g in range(c.G):
        if g == bs.CAP_SHORT:
            continue
        code, n_out, n_in, err_at = fields[g]
        ts, isi, bits = bufs[g]
        assert_same((code, ts[:n_out], isi[:n_out], bits[:n_out], n_in, err_at), c.ref(g, agg))
        assert code == 0 and err_at == -1
