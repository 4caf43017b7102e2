"""The direct aligned group without the qualifier stream (reg_run's CERT
instantiation, k_ds_reg.hip) on the value, time and layout domains: the cases
of tests/cert_domains.py, each uploaded as test_values_only_certificate.upload
uploads it (64 bytes of 0xFF behind nbytes), flagged by tsdbhip_desc_certify
and run with "group_direct" "always". On that path dir_fields, dir_key and the
bucket test of ds_reg_direct_body alone decide whether a row is the launch's,
so every case sits on an edge of their arithmetic, and the expected
tsdbhip_timing.paths word comes from cert_domains.verdict, the restatement of
that arithmetic, and from layouts.rows_streamable — never from a run.
test_values_only_domains_cpu.py asserts that each case is what it is named for.

Every query is an integer query: timestamps, values, isInteger,
aggregatedSize, the error code and err_index equal the oracle's bit for bit
(the one exception: a rate in test_flag_is_inert_elsewhere, held to
test_value_domains.py's 1e-9 of the sum of |terms|).

The A/B rule (`ab`): each call runs twice on the same flagged descriptor, with
"quals_proven" "auto" and "off". Both equal the oracle and each other,
paths_auto & ~QP == paths_off, and QP is set exactly when the direct launch
ran, taken or fallen back. The taken-or-not cases run under both
"group_direct_load" settings."""
import numpy as np
import pytest

import cert_domains as cd
import layouts
import oracle
import test_layouts as tl
import test_time_domains as ttd
import time_domains as td
import value_domains as vd
from cert_domains import AVG, PAIRS16, PAIRS4, SUM, U32MAX
from helpers import assert_same
from layouts import NAMES, relayout
from opentsdb_amd import _abi, core, packing
from test_value_domains import as_double, rank_starts, ref
from test_values_only_certificate import upload

pytestmark = pytest.mark.gpu
QP, DQP = _abi.PATH_QUALS_PROVEN, _abi.DESC_QUALS_PROVEN
GD, GDF, GDL, AG, UNI = tl.GD, tl.GDF, tl.GDL, tl.AG, tl.UNI
FALLBACKS = tl.GDF | tl.UFB | tl.AR | tl.DR


@pytest.fixture
def always(ctx):
    ctx.set_option("group_direct", "always")
    yield
    ctx.set_option("group_direct", "on")


@pytest.fixture(params=["lines_nt", "rows"])
def load(request, ctx, always):
    ctx.set_option("group_direct_load", request.param)
    yield request.param
    ctx.set_option("group_direct_load", "auto")


class option:
    """`with option(c, name, value, default):`"""

    def __init__(self, c, name, value, default):
        self.c, self.name, self.value, self.default = c, name, value, default

    def __enter__(self):
        self.c.set_option(self.name, self.value)

    def __exit__(self, *exc):
        self.c.set_option(self.name, self.default)
        return False


_UP = {}


def flagged(ctx, key, ss, lead=0):
    """`ss` uploaded once and certified by tsdbhip_desc_certify: a flagged
    device descriptor"""
    k = (key, lead)
    if k not in _UP:
        d, t = upload(ctx, ss, lead)
        assert core.desc_certify(ctx, d) == (0, 0) and d.flags & DQP, key
        _UP[k] = (d, t)
    return _UP[k][0]


def call(c, d, cap, agg, dsa, interval, start=0, end=U32MAX, rate=False, exact=False):
    res = core.run_spanset(c, None, start, end, agg, rate, interval, dsa, exact=exact, device_desc=d, capacity=cap)
    assert res[0] not in (_abi.E_HIP, _abi.E_RCCL), c.last_error()
    return res, c.timing().paths


def bit_for_bit(o):
    def check(res):
        assert_same(res, o, exact_double=True)
        if o.code:
            assert res[5] == o.err_index, f"err_index gpu={res[5]} oracle={o.err_index}"
        else:
            assert o.is_int.all()
    return check


def identical(a, b):
    assert (a[0], a[4], a[5]) == (b[0], b[4], b[5]), ((a[0], a[4], a[5]), (b[0], b[4], b[5]))
    for x, y in zip(a[1:4], b[1:4]):
        np.testing.assert_array_equal(x, y)


def ab(c, d, cap, check, what, *q, **kw):
    """the A/B rule; returns the paths word of the "auto" call"""
    a, pa = call(c, d, cap, *q, **kw)
    with option(c, "quals_proven", "off", "auto"):
        b, pb = call(c, d, cap, *q, **kw)
    try:
        check(a)
        check(b)
        identical(a, b)
    except AssertionError as e:
        raise AssertionError(f"{what} {q} {kw} paths {pa:#x} / off {pb:#x}: {e}") from None
    assert pa & ~QP == pb, f"{what} {q} {kw}: paths {pa:#x}, with quals_proven off {pb:#x}"
    assert bool(pa & QP) == bool(pb & (GD | GDF)), f"{what} {q} {kw}: paths {pa:#x}, with quals_proven off {pb:#x}"
    return pa


def lines_of(load):
    return GDL if load.startswith("lines") else 0


def taken(p, load, what):
    lines = lines_of(load)
    tl.expect(p, GD | AG | UNI | QP | lines, FALLBACKS | (GDL ^ lines), what)


def fell_back(p, load, what):
    lines = lines_of(load)
    tl.expect(p, GDF | QP | lines, GD | (GDL ^ lines), what)


def cells(ss):
    return max(1, int(ss.n_cells()))


# ---- 1. values ----

@pytest.mark.parametrize("run", cd.VALUE_RUNS, ids=lambda r: f"run{r}")
@pytest.mark.parametrize("step", cd.STEPS)
@pytest.mark.parametrize("pool", cd.VALUE_POOLS)
def test_values(ctx, load, pool, step, run):
    """longs that wrap, negative longs and 4-byte cells of either sign at the
    int's edges; 10 and 60 buckets a span, at step 2 through an interval that
    is no multiple of the step; runs of 1 and 8 spans a wave"""
    g = vd.one_row(pool, step, S=cd.spans_of_run(run))
    d = flagged(ctx, g.key, g.ss)
    with option(ctx, "group_direct_run", str(run), "auto"):
        for interval in cd.VALUE_INTERVALS[step]:
            assert cd.member(g.ss, interval=interval)
            for agg, dsa in PAIRS16:
                what = (pool, step, run, load)
                p = ab(ctx, d, cells(g.ss), bit_for_bit(ref(g, agg, False, interval, dsa)), what, agg, dsa, interval)
                taken(p, load, what + (agg, dsa, interval))


# ---- 2. time ----

@pytest.mark.parametrize("step", cd.STEPS)
@pytest.mark.parametrize("pool", cd.TIME_POOLS)
def test_time(ctx, load, pool, step):
    """2^31 in the first and in a later chunk, a last cell at 2^32 - 1, a first
    cell at timestamp 1: all members"""
    g = td.one_row(pool, step)
    assert cd.member(g.ss)
    d = flagged(ctx, g.key, g.ss)
    for agg, dsa in PAIRS16:
        what = (pool, step, load, agg, dsa)
        taken(ab(ctx, d, cells(g.ss), bit_for_bit(ref(g, agg, False, 60, dsa)), what, agg, dsa, 60), load, what)


def past32_contract(res):
    """include/tsdbhip.h, "Timestamps are 32 bits": a cell at or beyond 2^32
    fails the call at assembly, nothing emitted — the library's one deliberate
    departure from the oracle (test_time_domains.past32_fails)"""
    assert (res[0], len(res[1]), res[5]) == (_abi.E_INVALID_ARG, 0, 0), (res[0], len(res[1]), res[5])


@pytest.mark.parametrize("name", sorted(cd.refused_time_groups()))
def test_time_refused(ctx, load, name):
    """a first cell at timestamp 0, a last cell at 2^32: proven rows, flagged
    by tsdbhip_desc_certify, which dir_key alone keeps off the path"""
    g, end, clauses, _ = cd.refused_time_groups()[name]
    assert sorted(cd.verdict(g.ss, 0, end, 60)) == sorted(clauses)
    d = flagged(ctx, g.key, g.ss)
    for agg, dsa in PAIRS4:
        if g.pool == "EPOCH0":
            o = ttd.ref(g, agg, False, 60, dsa, 0, end)
            assert (o.code, o.err_index) == (_abi.E_OUT_OF_BOUNDS, 0)
            check = bit_for_bit(o)
        else:
            check = past32_contract
        what = (name, load, agg, dsa)
        fell_back(ab(ctx, d, cells(g.ss), check, what, agg, dsa, 60, end=end), load, what)


# ---- 3. windows ----

@pytest.mark.parametrize("pool,step", cd.WINDOW_GROUPS, ids=[f"{p}-{s}" for p, s in cd.WINDOW_GROUPS])
def test_windows(ctx, load, pool, step):
    """every pair of time_domains.windows: taken exactly where [start, end]
    holds [first, last], that window itself included; ends at 2^32 and 2^40"""
    g = td.one_row(pool, step)
    d = flagged(ctx, g.key, g.ss)
    n_taken = 0
    for start, end in td.windows(g):
        v = cd.verdict(g.ss, start, end, cd.WINDOW_INTERVAL)
        for agg, dsa in cd.WINDOW_PAIRS:
            o = ttd.ref(g, agg, False, cd.WINDOW_INTERVAL, dsa, start, end)
            what = (pool, step, load, start, end, agg, dsa, sorted(v))
            p = ab(ctx, d, cells(g.ss), bit_for_bit(o), what, agg, dsa, cd.WINDOW_INTERVAL, start=start, end=end)
            if not v:
                taken(p, load, what)
                n_taken += 1
            else:
                assert not p & GD, f"{what}: paths {p:#x}"
    assert n_taken  # (which windows: test_values_only_domains_cpu.py::test_windows_hold_both_verdicts)


# ---- 4. row geometry ----

@pytest.mark.parametrize("name", list(cd.GEOMETRY))
def test_geometry(ctx, load, name):
    """a last delta of 4095, 64 and 65 buckets, 32760 and 32768 value bytes,
    the largest member (4096 four-byte cells, eight full chunks), the
    workload's row (a 16-cell tail), steps that are no power of two, a
    one-cell row among members"""
    make, intervals, clauses = cd.GEOMETRY[name]
    g = make()
    d = flagged(ctx, g.key, g.ss)
    for interval in intervals:
        assert sorted(cd.verdict(g.ss, 0, U32MAX, interval)) == sorted(clauses)
        for agg, dsa in PAIRS4:
            what = (name, load, interval, agg, dsa)
            p = ab(ctx, d, cells(g.ss), bit_for_bit(ref(g, agg, False, interval, dsa)), what, agg, dsa, interval)
            (fell_back if clauses else taken)(p, load, what)


# ---- 5. layouts ----

class Led:
    """what the alignment predicates say of a layout uploaded behind `lead` bytes"""

    def __init__(self, lg, lead):
        ss, pad = lg.ss, np.full(lead, 0xFF, np.uint8)
        moved = packing.SpanSet(ss.span_row_start, ss.row_base, ss.row_ncells, ss.row_qual_off + np.uint64(lead),
                                ss.row_val_off + np.uint64(lead), ss.row_val_len, np.concatenate([pad, ss.qual_bytes]),
                                np.concatenate([pad, ss.val_bytes]))
        self.g, self.name = lg.g, f"{lg.name}+{lead}"
        self.stream, self.prop = layouts.rows_streamable(moved), layouts.rows_proposable(moved)
        self.member = cd.member(moved)


@pytest.mark.parametrize("run", cd.LAYOUT_RUNS, ids=lambda r: f"run{r}")
@pytest.mark.parametrize("pool", cd.LAYOUT_POOLS)
@pytest.mark.parametrize("name", NAMES)
def test_layouts(ctx, load, name, pool, run):
    """every layout is proven (even qualifier offsets) and certified by the
    kernel; taken on the streamable ones — `poison`, `shuffled`, `reversed`:
    the clamped loads behind a row's last cell meet 0xFF and none of it
    reaches a result — and fallen back, under the flag, on the others"""
    g = vd.one_row(pool, 2, S=cd.spans_of_run(run))
    lg = tl.laid(g, name)
    with option(ctx, "group_direct_run", str(run), "auto"):
        for lead in cd.layout_leads(name):
            led = Led(lg, lead)
            assert led.member == led.stream
            d = flagged(ctx, (g.key, name), lg.ss, lead)
            for agg, dsa in PAIRS4:
                what = (led.name, pool, run, load, agg, dsa)
                p = ab(ctx, d, cells(g.ss), bit_for_bit(ref(g, agg, False, 60, dsa)), what, agg, dsa, 60)
                tl.direct_expect(p, led, load, what)
                assert p & QP, f"{what}: paths {p:#x}"


@pytest.mark.parametrize("run", cd.LAYOUT_RUNS, ids=lambda r: f"run{r}")
@pytest.mark.parametrize("pool", cd.LAYOUT_POOLS)
@pytest.mark.parametrize("source", cd.PACK_SOURCES)
def test_packed(ctx, load, source, pool, run):
    """tsdbhip_desc_pack of an unflagged source that is not streamable: the
    packer flags what it made and the call is taken"""
    g = vd.one_row(pool, 2, S=cd.spans_of_run(run))
    src, _ = upload(ctx, relayout(g.ss, source, seed=tl.SEED))
    assert not src.flags & DQP
    with core.PackedDesc(ctx, src) as out, option(ctx, "group_direct_run", str(run), "auto"):
        assert out.flags & DQP
        for agg, dsa in PAIRS4:
            what = ("packed " + source, pool, run, load, agg, dsa)
            taken(ab(ctx, out, cells(g.ss), bit_for_bit(ref(g, agg, False, 60, dsa)), what, agg, dsa, 60), load, what)


# ---- 6. ranks ----

@pytest.fixture(scope="module")
def mctx3():
    from opentsdb_amd._lib import Context
    c = Context(devices=[0] * 3)
    assert c.ranks == 3
    yield c
    c.close()


@pytest.mark.parametrize("mode", ["auto", "rank0"])
def test_ranks(ctx, mctx3, mode):
    """three in-process ranks of [0, 24), [24, 47) and [47, 70); "rank0": rank
    0 alone runs without the qualifier stream"""
    with option(mctx3, "group_direct", "always", "on"), option(mctx3, "quals_proven", mode, "auto"):
        for g in cd.rank_groups():
            assert rank_starts(g) == [0, 24, 47, 70]
            d = flagged(ctx, g.key, g.ss)
            for agg, dsa in PAIRS4:
                res, p = call(mctx3, d, cells(g.ss), agg, dsa, 60)
                what = (g.pool, mode, agg, dsa)
                try:
                    bit_for_bit(ref(g, agg, False, 60, dsa))(res)
                except AssertionError as e:
                    raise AssertionError(f"{what} paths {p:#x}: {e}") from None
                tl.expect(p, GD | AG | QP, FALLBACKS, what)  # (rank 0's paths)
                assert mctx3.timing().n_collectives == 1, what


# ---- 7. the flag is inert everywhere else ----

def by_hand(d, on):
    d.flags = (d.flags | DQP) if on else (d.flags & ~DQP)
    return d


def rate_scale(abs_bad):
    """test_value_domains.term_scale for a sum of rates: a term (y1 - y0) / dt
    with dt >= 1 is bounded by |y1| + |y0|"""
    a = as_double(oracle.spangroup(abs_bad, 0, U32MAX, SUM))
    return a[1:] + a[:-1]


@pytest.mark.parametrize("pool", cd.INERT_POOLS)
def test_flag_is_inert_elsewhere(ctx, mctx3, pool):
    """a false promise (one qualifier off the cadence, the flag set by hand) on
    every path but the direct launch: lockstep, k_ug_dev, the aligned group and
    its rerun, EXACT_ORDER, the decode variants, the batch, three ranks. Each
    answers for the bytes as they are, with the paths word of the same call on
    the unflagged descriptor and without QP; then the direct launch on the
    same descriptor answers for the clean group"""
    clean = {S: cd.inert_group(pool, S) for S in (70, 100)}
    bad = {S: cd.corrupted(g.ss) for S, g in clean.items()}
    dev = {S: upload(ctx, ss) for S, ss in bad.items()}
    assert not core.quals_proven(bad[70]).all()

    def both(fn, d, what):
        f, pf = fn(by_hand(d, True))
        u, pu = fn(by_hand(d, False))
        assert pf == pu and not pf & QP, f"{what}: paths {pf:#x} flagged, {pu:#x} unflagged"
        return f, u

    for q in cd.inert_queries():
        d, ss = dev[q.S][0], bad[q.S]
        o = oracle.spangroup(ss, 0, U32MAX, q.agg, q.rate, q.interval, q.dsa)
        for name, (value, _) in q.options.items():
            ctx.set_option(name, value)
        try:
            f, u = both(lambda x: call(ctx, x, cells(ss), q.agg, q.dsa, q.interval, rate=q.rate, exact=q.exact), d, q)
        finally:
            for name, (_, default) in q.options.items():
                ctx.set_option(name, default)
        try:
            if q.rate:
                scale = rate_scale(cd.corrupted(clean[q.S].abs().ss))
                assert o.code == 0 and len(scale) == len(o.ts)
                for r in (f, u):
                    assert_same(r, o, abs_scale=scale, exact_double=q.exact)
            else:
                bit_for_bit(o)(f)
                bit_for_bit(o)(u)
                identical(f, u)
        except AssertionError as e:
            raise AssertionError(f"{pool} {q}: {e}") from None

    # the batch: paths 0 either way, each group the oracle's on its own spans
    d, ss, gss = dev[70][0], bad[70], cd.BATCH_CUT
    caps = [600 * (gss[k + 1] - gss[k]) + 1 for k in range(len(gss) - 1)]
    for agg, rate, interval, dsa in cd.BATCH_QUERIES:
        def batch(x):
            rc, res = core.run_spanset_batch(ctx, None, gss, 0, U32MAX, agg, rate, interval, dsa, capacities=caps,
                                             device_desc=x)
            assert rc == 0, ctx.last_error()
            return res, ctx.timing().paths
        f, u = both(batch, d, ("batch", agg, rate, interval, dsa))
        for k in range(len(gss) - 1):
            o = oracle.spangroup(ss.shard(gss[k], gss[k + 1]), 0, U32MAX, agg, rate, interval, dsa)
            for r in (f, u):
                if rate:  # (a max of rates selects one term)
                    assert_same(r[k], o)
                else:
                    bit_for_bit(o)(r[k])

    # three ranks, the aligned group's non-direct form
    with option(mctx3, "group_direct", "off", "on"):
        for agg, rate, interval, dsa in cd.RANK_QUERIES:
            o = oracle.spangroup(ss, 0, U32MAX, agg, rate, interval, dsa)
            f, u = both(lambda x: call(mctx3, x, cells(ss), agg, dsa, interval, rate=rate), d,
                        ("ranks", agg, rate, interval, dsa))
            bit_for_bit(o)(f)
            bit_for_bit(o)(u)
            identical(f, u)

    # ... and where the flag is meant to act, the same descriptor does differ
    with option(ctx, "group_direct", "always", "on"):
        o = ref(clean[70], AVG, False, 60, SUM)
        res, p = call(ctx, by_hand(d, True), cells(ss), AVG, SUM, 60)
        bit_for_bit(o)(res)
        tl.expect(p, GD | AG | QP, FALLBACKS, "the direct launch on the false promise")
        res, p = call(ctx, by_hand(d, False), cells(ss), AVG, SUM, 60)
        bit_for_bit(oracle.spangroup(ss, 0, U32MAX, AVG, False, 60, SUM))(res)
        tl.expect(p, GDF, GD | QP, "the direct launch on the unflagged descriptor")
