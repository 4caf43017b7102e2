"""Extreme longs and special floats through every kernel path: the groups of
tests/value_domains.py (longs that wrap, negative and boundary-width cells,
signed zeros, denormals, NaN first / later / in a bucket, sums that overflow,
longs beyond 2^53 next to a float) on the decode variants, the lockstep and
uniform paths, the aligned group and its direct form, the batch and the rank
merge, each compared with the oracle and each asserting the
tsdbhip_timing.paths bits of the path it is meant to take.

Integers, timestamps, error codes and error indices are bit-exact. Doubles are
bit-exact under TSDBHIP_EXACT_ORDER (the sign of zero included). Without it the
ZEROS pool is still compared by bits (sum, min, max, avg: the project's 1e-9
of the result accepts 0.0 for -0.0, the reference's first-zero rule does not,
and the stricter of the two is kept); every other double is held to 1e-9: of the result where every term has one sign (the NaN
and overflow pools are positive apart from those cells) and for min / max,
which select; else of the same aggregate over |terms| (assert_same's
abs_scale), taken from the oracle on the group's |value| twin — sum and avg
as they are, and max for dev, whose Welford state in any merge order is off
by a few n ulp of the largest |term| (n <= 100 spans: 1e-14 of it). A rate's
term (y1 - y0) / dt is bounded by (|y1| + |y0|) / dt.

test_value_domains_cpu.py asserts, on the oracle alone, that these groups wrap,
truncate, saturate, keep a zero's sign and fail at the designed index."""
import numpy as np
import pytest

import oracle
import value_domains as vd
from helpers import U32MAX, assert_same, with_option
from opentsdb_amd import _abi, core

pytestmark = pytest.mark.gpu

AGGS = [0, 1, 2, 3, 4]
SUM, MIN, MAX, AVG, DEV = AGGS
UNI, LS, AG = _abi.PATH_UNIFORM, _abi.PATH_LOCKSTEP, _abi.PATH_ALIGNED_GROUP
GD, GDF = _abi.PATH_GROUP_DIRECT, _abi.PATH_GROUP_DIRECT_FALLBACK
REDONE = _abi.PATH_UNIFORM_FALLBACK | _abi.PATH_DIRECT_REDO | GDF  # a streaming path tried and given up
STREAMING = UNI | LS | GD | REDONE
SCALED = ("ZEROS", "DENORM", "BIG_MIXED") + vd.INT_POOLS  # mixed signs: doubles against the sum of |terms|
F4, F8 = vd.F4, vd.F8

_REF = {}  # the oracle's results, shared by the tests


def ref(g, agg, rate=False, interval=0, ds_agg=0):
    """the oracle's result, computed once a query and shared"""
    k = (g.key, agg, rate, interval, ds_agg if interval else 0)
    if k not in _REF:
        _REF[k] = oracle.spangroup(g.ss, 0, U32MAX, agg, rate, interval, ds_agg)
    return _REF[k]


def as_double(o):
    return np.where(o.is_int.astype(bool), o.bits.astype(np.float64), o.bits.view(np.float64))


def term_scale(g, agg, rate, interval, ds_agg):
    """the aggregate over |terms| (see the module's docstring)"""
    up = lambda a: a if a in (SUM, AVG) else MAX
    a = as_double(ref(g.abs(), up(agg), False, interval, up(ds_agg)))
    if rate:
        assert g.shape == "one_row" and not interval
        a = (a[1:] + a[:-1]) / g.meta["step"]
    return a


def compare(g, res, o, agg, rate, interval, ds_agg, exact):
    if o.code:
        assert res[5] == o.err_index, f"err_index gpu={res[5]} oracle={o.err_index}"
    if exact or (g.pool == "ZEROS" and agg != DEV and not (interval and ds_agg == DEV)):
        # ZEROS outside EXACT_ORDER too: a sum or avg of zeros is -0.0 only when every term is, in
        # any order, and min / max keep the first zero in span order, which every path's merge
        # follows; 1e-9 of the result cannot tell 0.0 from -0.0, so the bits are compared
        return assert_same(res, o, exact_double=True)
    summed = agg in (SUM, AVG, DEV) or (interval and ds_agg in (SUM, AVG, DEV))
    if g.pool in SCALED and summed and o.code == 0 and not o.is_int.all():
        return assert_same(res, o, abs_scale=term_scale(g, agg, rate, interval, ds_agg))
    assert_same(res, o)


def check(c, g, agg, rate=False, interval=0, ds_agg=0, exact=False):
    """one query on the GPU against the oracle; returns the call's paths word"""
    o = ref(g, agg, rate, interval, ds_agg)
    res = core.run_spanset(c, g.ss, 0, U32MAX, agg, rate, interval, ds_agg, exact=exact)
    assert res[0] not in (_abi.E_HIP, _abi.E_RCCL), c.last_error()
    p = c.timing().paths
    try:
        compare(g, res, o, agg, rate, interval, ds_agg, exact)
    except AssertionError as e:
        raise AssertionError(f"{g.pool} {g.shape} agg={agg} rate={rate} ds=({interval},{ds_agg}) exact={exact} "
                             f"paths={p:#x}: {e}") from None
    return p


# ---- 1. the decode variants ----

@pytest.fixture(params=["auto", "general", "fast", "chunks", "spans", "direct"])
def decode(request):
    yield from with_option(request, "decode", request.param, "auto")


def uniform_expected(g, agg, interval, ds_agg):
    """uniform_run's queries (api.hip) on a group of one class key: integer dev
    without downsampling (k_ug_dev), and downsampling by sum / min / max / avg
    (the aligned group or E on the key's buckets). Lockstep stays with "on"
    for groups this small."""
    if not (g.shape == "one_row" and g.one_class):
        return False
    return (agg == DEV and not g.is_float) if not interval else ds_agg <= 3


DECODE_POOLS = ["WRAP64", "WIDTHS", "INT32_EDGE", "ZEROS", "DENORM", "NAN_LATER", "NAN_FIRST", "NAN_BUCKET",
                "BIG_MIXED"]


@pytest.mark.parametrize("shape", ["one_row", "jittered"])
@pytest.mark.parametrize("pool", DECODE_POOLS)
def test_decode_variants(ctx, decode, pool, shape):
    """no downsampling under every aggregator; 60-s and 13-s buckets under
    every downsampler (the cross-span aggregator turning with it); both
    EXACT_ORDER settings. Float pools: float32 and float64 spans by turns. The
    forced variants and EXACT_ORDER keep off the uniform paths; "auto" takes
    them for the one-class groups (WRAP64, INT32_EDGE on one_row)."""
    g = vd.one_row(pool, 2) if shape == "one_row" else vd.jittered(pool)
    qs = [(agg, 0, 0) for agg in AGGS]
    qs += [((dsa + (1 if interval == 60 else 3)) % 5, interval, dsa) for interval in (60, 13) for dsa in AGGS]
    for agg, interval, dsa in qs:
        for exact in (False, True):
            p = check(ctx, g, agg, False, interval, dsa, exact)
            q = (agg, interval, dsa, exact, hex(p))
            assert not p & REDONE, q
            if decode != "auto" or exact:
                assert not p & STREAMING, q
            else:
                assert bool(p & UNI) == uniform_expected(g, agg, interval, dsa), q


# ---- 2. lockstep and uniform (lockstep=always) ----

@pytest.fixture
def lockstep_always(request):
    yield from with_option(request, "lockstep", "always", "on")


LOCKSTEP_GROUPS = [("WRAP64", None), ("INT32_EDGE", None), ("NEG", None)] + \
    [(p, k) for p in ("ZEROS", "DENORM", "NAN_LATER", "NAN_FIRST", "HUGE") for k in (F4, F8)]


@pytest.mark.parametrize("pool,kind", LOCKSTEP_GROUPS, ids=[p + (k or "") for p, k in LOCKSTEP_GROUPS])
@pytest.mark.parametrize("agg", AGGS)
@pytest.mark.parametrize("rate", [False, True], ids=["norate", "rate"])
def test_lockstep_uniform(ctx, lockstep_always, pool, kind, agg, rate):
    """one_row at step 2: 8-byte, 4-byte and negative longs, and float32 /
    float64 zeros, denormals, NaN later and first, overflow. k_lockstep for
    every query but dev without rate, which is the span-ordered pass: k_ug_dev
    for integers (phases of 96 spans: 100 spans), the general path for floats."""
    int_dev = agg == DEV and not rate and kind is None
    g = vd.one_row(pool, 2, S=100 if int_dev else 70, kind=kind)
    p = check(ctx, g, agg, rate)
    assert not p & REDONE, hex(p)
    if agg != DEV or rate:
        assert p & UNI and p & LS, hex(p)
    elif int_dev:
        assert p & UNI and not p & LS, hex(p)
        assert ref(g, agg).is_int.all()  # (so the comparison above was bit for bit)
    else:
        assert not p & (UNI | LS), hex(p)


def test_ug_dev_saturates(ctx, lockstep_always):
    """Long.MIN_VALUE and Long.MAX_VALUE at one grid point of two spans:
    their deviation is 2^63 and (long) of it Long.MAX_VALUE"""
    g = vd.one_row("WRAP64", 2, S=2)
    assert sorted(g.values(5)) == [vd.INT64_MIN, vd.INT64_MAX]
    res = core.run_spanset(ctx, g.ss, 0, U32MAX, DEV)
    p = ctx.timing().paths
    assert_same(res, ref(g, DEV), exact_double=True)
    assert int(res[3][5]) == vd.INT64_MAX and res[2][5] == 1
    assert p & UNI and not p & (LS | REDONE), hex(p)


# ---- 3. the aligned group ----

INT_GROUPS = ["WRAP64", "NEG", "INT32_EDGE"]


@pytest.mark.parametrize("pool", INT_GROUPS)
@pytest.mark.parametrize("step", [1, 2])
@pytest.mark.parametrize("exact", [False, True], ids=["", "exact"])
def test_aligned_group(ctx, pool, step, exact):
    """60-s buckets over 600 cells at 1 s (10 buckets) and 2 s (20): the
    wrapping sum, signed min / max and truncating avg of k_ds_reg's block
    partials. EXACT_ORDER keeps off the uniform path: the aligned group of the
    general path."""
    g = vd.one_row(pool, step)
    for agg in (SUM, MIN, MAX, AVG):
        for dsa in (SUM, MIN, MAX, AVG):
            p = check(ctx, g, agg, False, 60, dsa, exact)
            q = (agg, dsa, hex(p))
            assert p & AG and not p & (REDONE | _abi.PATH_ALIGNED_RERUN | GD), q
            assert bool(p & UNI) == (not exact), q


# ---- 4. the direct aligned group ----

@pytest.fixture
def group_direct_always(request):
    yield from with_option(request, "group_direct", "always", "on")


def taken(p):
    """as tests/test_group_direct.py defines it"""
    return bool(p & GD) and not p & GDF and bool(p & AG)


@pytest.mark.parametrize("pool", INT_GROUPS)
@pytest.mark.parametrize("step", [1, 2])
@pytest.mark.parametrize("run", [1, 8, 32])
def test_group_direct(ctx, group_direct_always, run, pool, step):
    """runs of 1, 8 and 32 spans a wave over 8 run + 3 spans (wave g of G takes
    spans g, g + G, ...: full and short runs)"""
    ctx.set_option("group_direct_run", str(run))
    try:
        g = vd.one_row(pool, step, S=8 * run + 3)
        for agg in (SUM, MIN, MAX, AVG):
            for dsa in (SUM, MIN, MAX, AVG):
                p = check(ctx, g, agg, False, 60, dsa)
                assert taken(p), (agg, dsa, hex(p))
    finally:
        ctx.set_option("group_direct_run", "auto")


# ---- 5. uniform E ----

@pytest.mark.parametrize("pool", ["ZEROS", "DENORM", "NAN_BUCKET"])
@pytest.mark.parametrize("kind", [F4, F8])
@pytest.mark.parametrize("interval", [60, 10])
def test_uniform_e_floats(ctx, pool, kind, interval):
    """k_ds_reg's E on the key's buckets and k_reduce over it: the sign of a
    bucket's zero, denormal cells, a NaN heading a bucket and one inside it"""
    g = vd.one_row(pool, 2, kind=kind)
    for agg in AGGS:
        for dsa in (SUM, MIN, MAX, AVG):
            p = check(ctx, g, agg, False, interval, dsa)
            assert p & UNI and not p & (AG | LS | REDONE), (agg, dsa, hex(p))


@pytest.mark.parametrize("pool", INT_GROUPS)
@pytest.mark.parametrize("step", [1, 2])
def test_uniform_e_integer_dev(ctx, pool, step):
    """dev across the spans of downsampled integers: E (no aligned group).
    A dev downsampler is none of uniform_run's queries (ds_agg <= 3): those
    calls take the general path, compared all the same."""
    g = vd.one_row(pool, step)
    for dsa in (SUM, MIN, MAX, AVG):
        p = check(ctx, g, DEV, False, 60, dsa)
        assert p & UNI and not p & (AG | LS | REDONE), (dsa, hex(p))
    for agg in AGGS:
        p = check(ctx, g, agg, False, 60, DEV)
        assert not p & STREAMING, (agg, hex(p))


# ---- 6. the batch ----

@pytest.mark.parametrize("pool,kind", [("WRAP64", None), ("NAN_LATER", F8)], ids=["WRAP64", "NAN_LATER"])
@pytest.mark.parametrize("exact", [False, True], ids=["", "exact"])
def test_batch(ctx, pool, kind, exact):
    """three uneven groups cut from one_row, each against the oracle on that
    group alone, its own err_code and err_index included. NAN_LATER's span 35
    heads the third group: there its NaN is the first value (min / max fail),
    in the whole group it is not. The batch's segmented kernels report no
    streaming path."""
    g = vd.one_row(pool, 2, kind=kind)
    gss = [0, 9, 35, 70]
    codes = set()
    for agg in AGGS:
        for rate, interval, dsa in ((False, 0, 0), (True, 0, 0), (False, 60, AVG), (False, 60, MIN)):
            rc, res = core.run_spanset_batch(ctx, g.ss, gss, 0, U32MAX, agg, rate, interval, dsa, exact=exact)
            p = ctx.timing().paths
            assert p == 0, hex(p)
            first = 0
            for k in range(3):
                o = oracle.spangroup(g.ss.shard(gss[k], gss[k + 1]), 0, U32MAX, agg, rate, interval, dsa)
                try:
                    assert_same(res[k], o, exact_double=exact)
                    assert res[k][5] == o.err_index or not o.code
                except AssertionError as e:
                    raise AssertionError(f"group {k} agg={agg} rate={rate} ds=({interval},{dsa}): {e}") from None
                first = first or o.code
                codes.add((k, agg in (MIN, MAX), o.code))
            assert rc == first
    if pool == "NAN_LATER":  # (what the cut is for)
        assert (2, True, _abi.E_NAN_INF) in codes and (0, True, 0) in codes and (1, True, 0) in codes


# ---- 7. the rank merge: three ranks on one GPU ----

def rank_starts(g, ranks=3):
    """plan_shards (api.hip) for a host descriptor: the shards balanced by
    cells, rank r starting at the first span with r / ranks of the cells
    before it (a lower bound over the prefix sums)"""
    ss = g.ss
    rows = np.concatenate([[0], np.cumsum(ss.row_ncells.astype(np.int64))])
    pre = rows[ss.span_row_start.astype(np.int64)]
    b = [0]
    for r in range(1, ranks):
        b.append(max(b[-1], min(int(np.searchsorted(pre, pre[-1] * r // ranks, "left")), ss.n_spans)))
    return b + [ss.n_spans]


@pytest.fixture(scope="module")
def mctx():
    from opentsdb_amd._lib import Context
    c = Context(devices=[0, 0, 0])
    yield c
    c.close()


@pytest.mark.timeout(120)
@pytest.mark.parametrize("pool", INT_GROUPS)
@pytest.mark.parametrize("direct", ["on", "always"])
def test_rank_merge_integers(mctx, pool, direct):
    """the X_I64 min / max and X_U64 wrapping-sum exchanges, ldiv of the merged
    sum; dev is the span-ordered pass over the ranks"""
    mctx.set_option("group_direct", direct)
    try:
        g = vd.one_row(pool, 2)
        for agg in AGGS:
            p = check(mctx, g, agg)
            assert not p & REDONE, (agg, hex(p))
            assert bool(p & UNI) == bool(p & LS) == (agg != DEV), (agg, hex(p))
            p = check(mctx, g, agg, False, 60, AVG)
            assert not p & REDONE, (agg, hex(p))
            if agg != DEV:
                assert p & UNI and p & AG, (agg, hex(p))
                assert bool(p & GD) == (direct == "always"), (agg, hex(p))
            else:
                assert not p & (UNI | AG | GD), hex(p)
    finally:
        mctx.set_option("group_direct", "on")


NAN_PLACES = {"rank0-first": (0, 0, True), "rank1-first": (1, 0, False), "rank2-later": (2, 10, False)}


@pytest.mark.timeout(120)
@pytest.mark.parametrize("kind", [F4, F8])
@pytest.mark.parametrize("where", sorted(NAN_PLACES))
def test_rank_merge_nan_place(mctx, kind, where):
    """70 spans of 600 cells: ranks [0, 24), [24, 47), [47, 70). A NaN in the
    first span of rank 0 is the first value of min / max (E_NAN_INF at its grid
    point). In the first span of rank 1 it is the first value of that rank's
    partial and a later one of the group: the merge drops the rank's
    first-value-NaN flag. In a later span of rank 2 it is passed over at once."""
    rank, off, fails = NAN_PLACES[where]
    starts = rank_starts(vd.nan_at([], 2, kind))
    assert starts == [0, 24, 47, 70]
    span = starts[rank] + off
    g = vd.nan_at([(span, 360)], 2, kind)
    assert rank_starts(g) == starts and starts[rank] <= span < starts[rank + 1]
    for agg in (MIN, MAX):
        o = ref(g, agg)
        assert o.code == (_abi.E_NAN_INF if fails else 0) and (not fails or o.err_index == 360)
        for exact in (False, True):
            p = check(mctx, g, agg, exact=exact)
            assert not p & REDONE and bool(p & UNI) == bool(p & LS) == (not exact), (agg, exact, hex(p))


@pytest.mark.timeout(120)
@pytest.mark.parametrize("pool", ["ZEROS", "NAN_LATER", "NAN_FIRST"])
@pytest.mark.parametrize("kind", [F4, F8])
def test_rank_merge_floats(mctx, pool, kind):
    """min / max across the ranks: the zero of the first span in span order
    (by bits with and without EXACT_ORDER), NaN later (spans 1, 35 and 69: a
    later span of each of the ranks [0, 24), [24, 47), [47, 70)) and first"""
    g = vd.one_row(pool, 2, kind=kind)
    starts = rank_starts(g)
    assert starts == [0, 24, 47, 70] and not set(vd.nan_spans(70)) & set(starts)
    for agg in (MIN, MAX):
        for exact in (False, True):
            p = check(mctx, g, agg, exact=exact)
            assert not p & REDONE and bool(p & UNI) == bool(p & LS) == (not exact), (agg, exact, hex(p))
