"""The time axis through every kernel path: the groups of tests/time_domains.py
(2^31 inside a row, a last cell at 2^32 - 1, a first cell at timestamp 1,
bucket ends past 2^32, lerp brackets up to 2^32 - 2 wide, windows on and one
off every edge, qualifier deltas past the hour) on the decode variants, the
lockstep and uniform paths, the aligned group and its direct form, the batch
and the rank merge, each call compared with the oracle and each asserting its
tsdbhip_timing.paths word.

Timestamps, kinds, longs, codes and error indices are bit-exact; doubles are
bit-exact under TSDBHIP_EXACT_ORDER and held to 1e-9 otherwise, as in
test_value_domains.py: of the result for min / max, of the same aggregate over
|terms| elsewhere (the values are of mixed sign; a rate's term (y1 - y0) / dt
is bounded by (|y1| + |y0|) / dt).

A group at T31, TOP or EPOCH must take the path its twin at T0 takes (the same
deltas and values in T0's rows): every check runs both and compares the paths
words, so a boundary that sends a group to a fallback fails.

A span with a cell at or beyond 2^32 fails the call with E_INVALID_ARG at
assembly, and a span whose first cell is at timestamp 0 with E_OUT_OF_BOUNDS
(include/tsdbhip.h); test_time_domains_cpu.py records what the oracle answers
for the former."""
import numpy as np
import pytest

import oracle
import time_domains as td
from helpers import T0, assert_same, corrupt_qual, with_option
from opentsdb_amd import _abi, core
from time_domains import B31, P31, P32, TOP, U32MAX
from value_domains import F8, I8, Group

pytestmark = pytest.mark.gpu

AGGS = [0, 1, 2, 3, 4]
SUM, MIN, MAX, AVG, DEV = AGGS
UNI, LS, AG = _abi.PATH_UNIFORM, _abi.PATH_LOCKSTEP, _abi.PATH_ALIGNED_GROUP
GD, GDF = _abi.PATH_GROUP_DIRECT, _abi.PATH_GROUP_DIRECT_FALLBACK
REDONE = _abi.PATH_UNIFORM_FALLBACK | _abi.PATH_DIRECT_REDO | GDF  # a streaming path tried and given up
STREAMING = UNI | LS | GD | REDONE

_REF = {}  # the oracle's results, shared by the tests


def ref(g, agg, rate=False, interval=0, ds_agg=0, start=0, end=U32MAX):
    k = (g.key, agg, rate, interval, ds_agg if interval else 0, start, end)
    if k not in _REF:
        _REF[k] = oracle.spangroup(g.ss, start, end, agg, rate, interval, ds_agg)
    return _REF[k]


def as_double(o):
    return np.where(o.is_int.astype(bool), o.bits.astype(np.float64), o.bits.view(np.float64))


def term_scale(g, agg, rate, interval, ds_agg, start, end):
    """the aggregate over |terms| (test_value_domains.py)"""
    up = lambda a: a if a in (SUM, AVG) else MAX
    a = as_double(ref(g.abs(), up(agg), False, interval, up(ds_agg), start, end))
    if rate:
        # terms (y1 - y0) / dt with dt >= 1: bounded by the sum of the two neighbours' |terms|
        a = a[1:] + a[:-1] if len(a) > 1 else a
    return a


def run(c, g, agg, rate=False, interval=0, ds_agg=0, exact=False, start=0, end=U32MAX):
    """one query on the GPU against the oracle; returns the call's paths word"""
    o = ref(g, agg, rate, interval, ds_agg, start, end)
    res = core.run_spanset(c, g.ss, start, end, agg, rate, interval, ds_agg, exact=exact)
    assert res[0] not in (_abi.E_HIP, _abi.E_RCCL), c.last_error()
    p = c.timing().paths
    try:
        if o.code:
            assert res[5] == o.err_index, f"err_index gpu={res[5]} oracle={o.err_index}"
        summed = agg in (SUM, AVG, DEV) or (interval and ds_agg in (SUM, AVG, DEV)) or rate
        if exact or o.code or o.is_int.all():
            assert_same(res, o, exact_double=True)
        elif summed and g.series is not None and not (rate and g.shape != "one_row"):
            assert_same(res, o, abs_scale=term_scale(g, agg, rate, interval, ds_agg, start, end))
        else:
            assert_same(res, o)
    except AssertionError as e:
        raise AssertionError(f"{g.pool} {g.shape} {g.meta} [{start}, {end}] agg={agg} rate={rate} "
                             f"ds=({interval},{ds_agg}) exact={exact} paths={p:#x}: {e}") from None
    return p


def check(c, g, agg, rate=False, interval=0, ds_agg=0, exact=False):
    """run() on the group and on its twin at T0: one paths word"""
    p = run(c, g, agg, rate, interval, ds_agg, exact)
    p0 = run(c, td.twin(g), agg, rate, interval, ds_agg, exact)
    assert p == p0, (f"{g.pool} {g.shape} agg={agg} rate={rate} ds=({interval},{ds_agg}) exact={exact}: paths "
                     f"{p:#x}, at T0 {p0:#x}")
    return p


def uniform_expected(g, agg, interval, ds_agg):
    """uniform_run's queries on a group of one class key (test_value_domains.py)"""
    if not (g.shape == "one_row" and g.one_class):
        return False
    return (agg == DEV and not g.is_float) if not interval else ds_agg <= 3


def group_of(pool, shape):
    if shape == "jittered":
        return td.jittered(pool)
    return td.one_row(pool, int(shape[-1]))


# ---- 1. the decode variants ----

@pytest.fixture(params=["auto", "general", "fast", "chunks", "spans", "direct"])
def decode(request):
    yield from with_option(request, "decode", request.param, "auto")


DECODE_GROUPS = [(p, s) for p in td.POOLS for s in ("one_row1", "one_row2", "jittered")
                 if (p, s) != ("T31B", "jittered")]  # (T31B is a one_row layout: its jittered group is T31's)


def decode_queries():
    """no downsampling under every aggregator, and rate; 60-s and 13-s buckets
    under every downsampler (the cross-span aggregator turning with it); the
    interval list under sum and avg"""
    qs = [(agg, False, 0, 0) for agg in AGGS] + [(SUM, True, 0, 0), (DEV, True, 0, 0), (MIN, True, 0, 0)]
    qs += [((dsa + (1 if interval == 60 else 3)) % 5, False, interval, dsa) for interval in (60, 13) for dsa in AGGS]
    qs += [(a, False, interval, a) for interval in td.INTERVALS for a in (SUM, AVG)]
    return qs


def decode_case(c, decode, g):
    for agg, rate, interval, dsa in decode_queries():
        for exact in (False, True):
            p = check(c, g, agg, rate, interval, dsa, exact)
            q = (agg, rate, interval, dsa, exact, hex(p))
            assert not p & REDONE, q
            if decode != "auto" or exact:
                assert not p & STREAMING, q
            elif not rate and g.shape == "one_row" and interval in (0, 13, 60):
                assert bool(p & UNI) == uniform_expected(g, agg, interval, dsa), q


@pytest.mark.parametrize("pool,shape", DECODE_GROUPS, ids=[f"{p}-{s}" for p, s in DECODE_GROUPS])
def test_decode_variants(ctx, decode, pool, shape):
    decode_case(ctx, decode, group_of(pool, shape))


@pytest.mark.parametrize("merge", [False, True], ids=["uniform", "merged-row"])
def test_decode_variants_top_rows(ctx, decode, merge):
    """three hourly rows a span ending on 2^32 - 1 (k_ds_reg's pieces of
    several waves); one span's last row merged into its predecessor's RowSeq"""
    decode_case(ctx, decode, td.top_rows(merge=merge))


@pytest.mark.parametrize("pool", ["T31", "TOP"])
def test_decode_variants_floats(ctx, decode, pool):
    for g in (td.one_row(pool, 2, kind=F8), td.jittered(pool, kind=F8)):
        for agg, rate, interval, dsa in ((SUM, False, 0, 0), (MAX, False, 0, 0), (AVG, True, 0, 0),
                                         (DEV, False, 60, AVG), (MIN, False, 1696, SUM), (SUM, False, P31 - 1, MAX)):
            for exact in (False, True):
                p = check(ctx, g, agg, rate, interval, dsa, exact)
                assert not p & REDONE and (not p & STREAMING or (decode == "auto" and not exact)), hex(p)


# ---- 2. lockstep and uniform (lockstep=always) ----

@pytest.fixture
def lockstep_always(request):
    yield from with_option(request, "lockstep", "always", "on")


@pytest.mark.parametrize("pool", td.POOLS)
@pytest.mark.parametrize("agg", AGGS)
@pytest.mark.parametrize("rate", [False, True], ids=["norate", "rate"])
def test_lockstep_uniform(ctx, lockstep_always, pool, agg, rate):
    """k_lockstep (its grid_out = x0 + g * step) for every query but dev without
    rate: k_ug_dev for integers (phases of 96 spans: 100 spans), the general
    path for floats"""
    for kind in (I8, F8):
        int_dev = agg == DEV and not rate and kind == I8
        for step in (1, 2):
            g = td.one_row(pool, step, S=100 if int_dev else 70, kind=kind)
            p = check(ctx, g, agg, rate)
            assert not p & REDONE, hex(p)
            if agg != DEV or rate:
                assert p & UNI and p & LS, hex(p)
            elif int_dev:
                assert p & UNI and not p & LS, hex(p)
            else:
                assert not p & (UNI | LS), hex(p)


@pytest.mark.parametrize("pool", ["TOP", "T31"])
@pytest.mark.parametrize("interval", [60, 10, 1696])
def test_uniform_e_floats(ctx, pool, interval):
    """k_ds_reg's E on the key's buckets (reg_flush's formula timestamps) and
    k_reduce over it, float64 cells"""
    for step in (1, 2):
        g = td.one_row(pool, step, kind=F8)
        for agg in AGGS:
            for dsa in (SUM, MIN, MAX, AVG):
                p = check(ctx, g, agg, False, interval, dsa)
                assert p & UNI and not p & (AG | LS | REDONE), (agg, dsa, hex(p))


# ---- 3. the aligned group and its direct form ----

@pytest.mark.parametrize("pool", td.POOLS)
@pytest.mark.parametrize("step", [1, 2])
@pytest.mark.parametrize("exact", [False, True], ids=["", "exact"])
def test_aligned_group(ctx, pool, step, exact):
    g = td.one_row(pool, step)
    for agg in (SUM, MIN, MAX, AVG):
        for dsa in (SUM, MIN, MAX, AVG):
            p = check(ctx, g, agg, False, 60, dsa, exact)
            q = (agg, dsa, hex(p))
            assert p & AG and not p & (REDONE | _abi.PATH_ALIGNED_RERUN | GD), q
            assert bool(p & UNI) == (not exact), q


@pytest.fixture
def group_direct_always(request):
    yield from with_option(request, "group_direct", "always", "on")


def taken(p):
    """as tests/test_group_direct.py defines it"""
    return bool(p & GD) and not p & GDF and bool(p & AG)


@pytest.mark.parametrize("pool", ["T31", "TOP", "EPOCH"])
@pytest.mark.parametrize("step", [1, 2])
@pytest.mark.parametrize("run_len", [1, 8, 32])
def test_group_direct(ctx, group_direct_always, run_len, pool, step):
    """runs of 1, 8 and 32 spans a wave over 8 run + 3 spans; the intervals
    through 4096 (more than 64 buckets a span: not the direct form's, and the
    twin's word says so too)"""
    ctx.set_option("group_direct_run", str(run_len))
    try:
        g = td.one_row(pool, step, S=8 * run_len + 3)
        for agg in (SUM, MIN, MAX, AVG):
            for dsa in (SUM, MIN, MAX, AVG):
                p = check(ctx, g, agg, False, 60, dsa)
                assert taken(p), (agg, dsa, hex(p))
        for interval in [i for i in td.INTERVALS if i <= 4096]:
            for a in (SUM, AVG):
                p = check(ctx, g, a, False, interval, a)
                kk = -(-interval // step)  # cells a bucket; at most 64 buckets a span
                assert taken(p) == (-(-600 // kk) <= 64), (interval, a, hex(p))
    finally:
        ctx.set_option("group_direct_run", "auto")


# ---- 4. windows ----

@pytest.fixture(params=["auto", "general"])
def decode2(request):
    yield from with_option(request, "decode", request.param, "auto")


@pytest.mark.parametrize("pool", ["T31", "TOP"])
@pytest.mark.parametrize("step", [1, 2])
def test_windows(ctx, decode2, pool, step):
    """ends and starts on, one off and far off the first cell, an inside cell
    and the last cell; 2^31 - 1, 2^31, 2^32 - 1, 2^32 and 2^40; start == end
    and start > end. 8-byte cells: a start inside the row is quirk Q1's seek.
    A window equal to [first, last] keeps the group on its uniform path; one
    second inside either end takes it off (ug_probe: first >= start && last
    <= end)."""
    g = td.one_row(pool, step)
    first = g.meta["base"] + g.meta["d0"]
    last = first + step * 599
    for start, end in td.windows(g):
        for agg, interval, dsa in ((SUM, 0, 0), (DEV, 0, 0), (AVG, 60, SUM), (MAX, 60, MAX)):
            p = run(ctx, g, agg, False, interval, dsa, start=start, end=end)
            q = (start - first, end - last, agg, interval, hex(p))
            assert not p & REDONE, q
            if decode2 == "general":
                assert not p & STREAMING, q
            elif start <= first and end >= last:
                assert bool(p & UNI) == uniform_expected(g, agg, interval, dsa), q
            else:
                assert not p & UNI, q
    full = {(agg, iv): run(ctx, g, agg, False, iv, SUM) for agg, iv in ((DEV, 0), (AVG, 60))}
    for (agg, iv), pf in full.items():
        assert run(ctx, g, agg, False, iv, SUM, start=first, end=last) == pf
        for s, e in ((first + 1, last), (first, last - 1)):
            p = run(ctx, g, agg, False, iv, SUM, start=s, end=e)
            assert not p & (UNI | REDONE) and (decode2 == "general" or pf & UNI), (s - first, e - last, hex(p), hex(pf))


# ---- 5. WIDE: a context of its own (the 512 MiB bitmap goes with it) ----

@pytest.fixture(scope="module")
def wctx():
    from opentsdb_amd._lib import Context
    c = Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("x1", td.WIDE_X1)
@pytest.mark.parametrize("dec", ["auto", "general"])
def test_wide(wctx, dec, x1):
    """lerp divisors up to 2^32 - 2 around lerp_long's 2^31 - 1 switch, the
    wrapping product, a union-grid bitmap over [1, x1]"""
    g = td.wide(x1)
    wctx.set_option("decode", dec)
    try:
        for agg in AGGS:
            for rate in (False, True):
                p = run(wctx, g, agg, rate)
                assert not p & STREAMING, (agg, rate, hex(p))
    finally:
        wctx.set_option("decode", "auto")


# ---- 6. ROW_EDGE ----

@pytest.fixture(params=["auto", "general", "chunks"])
def decode3(request):
    yield from with_option(request, "decode", request.param, "auto")


@pytest.mark.parametrize("base", [T0, B31], ids=["T0", "B31"])
@pytest.mark.parametrize("last,nxt", td.ROW_EDGE_CASES)
def test_row_edge(ctx, decode3, base, last, nxt):
    g = td.row_edge(base, last, nxt)
    for agg, rate, interval, dsa in ((SUM, False, 0, 0), (AVG, True, 0, 0), (MAX, False, 60, AVG),
                                     (DEV, False, 3600, SUM), (MIN, False, 4096, MIN)):
        for exact in (False, True):
            p = run(ctx, g, agg, rate, interval, dsa, exact)
            assert not p & STREAMING, hex(p)


# ---- 7. the batch ----

def batch_of(groups):
    series = [s for g in groups for s in g.series]
    gss = np.concatenate([[0], np.cumsum([g.n_spans for g in groups])])
    return Group("BATCH", "batch", series, of=tuple(g.key for g in groups)), [int(x) for x in gss]


BATCH_QUERIES = [(agg, rate, interval, dsa) for agg in AGGS
                 for rate, interval, dsa in ((False, 0, 0), (True, 0, 0), (False, 60, AVG), (False, 1696, MIN))]


@pytest.mark.parametrize("exact", [False, True], ids=["", "exact"])
def test_batch_four_bases(ctx, exact):
    """one call whose groups sit at EPOCH, T0, T31 and TOP (four `lo`s), each
    against the oracle on that group alone"""
    groups = [td.one_row("EPOCH", 2, S=9), td.one_row("T31", 2, S=20, at_t0=True), td.one_row("T31", 1, S=13),
              td.one_row("TOP", 2, S=28), td.jittered("TOP"), td.jittered("EPOCH")]
    b, gss = batch_of(groups)
    for agg, rate, interval, dsa in BATCH_QUERIES:
        rc, res = core.run_spanset_batch(ctx, b.ss, gss, 0, U32MAX, agg, rate, interval, dsa, exact=exact)
        assert rc == 0 and ctx.timing().paths == 0
        for k, g in enumerate(groups):
            try:
                assert_same(res[k], ref(g, agg, rate, interval, dsa), exact_double=exact)
            except AssertionError as e:
                raise AssertionError(f"group {k} agg={agg} rate={rate} ds=({interval},{dsa}): {e}") from None


def test_batch_epoch0_between_good_groups(ctx):
    """per-group code and err_index; rc the first"""
    groups = [td.one_row("EPOCH", 2, S=9), td.one_row("EPOCH0", 2, S=5), td.one_row("TOP", 2, S=11)]
    b, gss = batch_of(groups)
    for agg, rate, interval, dsa in BATCH_QUERIES:
        rc, res = core.run_spanset_batch(ctx, b.ss, gss, 0, U32MAX, agg, rate, interval, dsa)
        assert rc == _abi.E_OUT_OF_BOUNDS
        for k, g in enumerate(groups):
            o = ref(g, agg, rate, interval, dsa)
            assert o.code == (_abi.E_OUT_OF_BOUNDS if k == 1 else 0)
            assert_same(res[k], o)
            assert res[k][5] == o.err_index or not o.code


# ---- 8. the rank merge: three ranks on one GPU ----

@pytest.fixture(scope="module")
def mctx():
    from opentsdb_amd._lib import Context
    c = Context(devices=[0, 0, 0])
    yield c
    c.close()


@pytest.mark.timeout(120)
@pytest.mark.parametrize("pool", ["T31", "TOP"])
@pytest.mark.parametrize("direct", ["on", "always"])
def test_rank_merge_one_row(mctx, pool, direct):
    mctx.set_option("group_direct", direct)
    try:
        for step in (1, 2):
            g = td.one_row(pool, step)
            for agg in AGGS:
                p = check(mctx, g, agg)
                assert not p & REDONE, (agg, hex(p))
                assert bool(p & UNI) == bool(p & LS) == (agg != DEV), (agg, hex(p))
                for interval in (60, 1696):
                    p = check(mctx, g, agg, False, interval, AVG)
                    assert not p & REDONE, (agg, interval, hex(p))
                    if agg != DEV:
                        assert p & UNI and p & AG, (agg, interval, hex(p))
                        assert bool(p & GD) == (direct == "always"), (agg, interval, hex(p))
                    else:
                        assert not p & (UNI | AG | GD), hex(p)
    finally:
        mctx.set_option("group_direct", "on")


@pytest.mark.timeout(120)
def test_rank_merge_jittered_top(mctx):
    """shards of four spans with different first timestamps: the ranks' grids
    differ and their bitmaps are remapped onto the global range (k_bitmap_remap
    with src_lo != dst_lo) up to 2^32 - 1"""
    g = td.jittered("TOP")
    firsts = [min(pts[0][0] for _, pts in g.series[i:i + 4]) for i in (0, 4, 8)]
    assert len(set(firsts)) == 3 and max(pts[-1][0] for _, pts in g.series) == U32MAX
    for agg in AGGS:
        for rate, interval, dsa in ((False, 0, 0), (True, 0, 0), (False, 60, AVG), (False, 1696, MAX),
                                    (False, P31 - 1, SUM)):
            for exact in (False, True):
                p = check(mctx, g, agg, rate, interval, dsa, exact)
                # (a sharded aligned-group query is launched speculatively on every rank and
                # falls back where the group is not one: UNIFORM_FALLBACK alone)
                assert not p & (UNI | LS | AG | GD | GDF | _abi.PATH_DIRECT_REDO), hex(p)


# ---- 9. shift invariance on the GPU ----

def gpu_shifted(c, g, agg, rate=False, interval=0, ds_agg=0, exact=False):
    """the GPU on the group against the GPU on its twin at T0: the same values,
    the timestamps base - T0 apart (a rate's first term y0 / x0 aside)"""
    a = core.run_spanset(c, g.ss, 0, U32MAX, agg, rate, interval, ds_agg, exact=exact)
    p = c.timing().paths
    b = core.run_spanset(c, td.twin(g).ss, 0, U32MAX, agg, rate, interval, ds_agg, exact=exact)
    assert p == c.timing().paths
    assert a[0] == b[0] == 0 and len(a[1]) == len(b[1]) > 0 and a[4] == b[4]
    assert ((a[1] - b[1]) == td.shift(g)).all()
    k = 1 if rate else 0
    assert (a[2][k:] == b[2][k:]).all() and (a[3][k:] == b[3][k:]).all(), "values differ under a shift"
    return p


@pytest.mark.parametrize("pool", td.POOLS)
def test_shift_invariance_streaming(ctx, lockstep_always, pool):
    """one query a streaming path: k_lockstep (sum, rate), k_ug_dev, the aligned
    group, E on the key's buckets"""
    for step in (1, 2):
        g = td.one_row(pool, step, S=100)
        assert gpu_shifted(ctx, g, SUM) & LS and gpu_shifted(ctx, g, MAX, True) & LS
        p = gpu_shifted(ctx, g, DEV)
        assert p & UNI and not p & LS
        assert gpu_shifted(ctx, g, AVG, False, 60, AVG) & AG
        p = gpu_shifted(ctx, g, DEV, False, 1696, SUM)
        assert p & UNI and not p & AG


@pytest.mark.parametrize("pool", ["T31", "TOP", "EPOCH"])
def test_shift_invariance_decode(ctx, decode, pool):
    for g in (td.one_row(pool, 2), td.jittered(pool), td.top_rows(merge=True)):
        for agg, rate, interval, dsa in ((SUM, False, 0, 0), (AVG, False, 60, MAX), (MIN, False, P31 - 1, MIN)):
            gpu_shifted(ctx, g, agg, rate, interval, dsa, exact=True)


def test_shift_invariance_group_direct(ctx, group_direct_always):
    for pool in ("T31", "TOP", "EPOCH"):
        assert taken(gpu_shifted(ctx, td.one_row(pool, 1), AVG, False, 60, SUM))


# ---- 10. EPOCH0 and PAST32 ----

@pytest.mark.parametrize("case", sorted(td.EPOCH0_CASES))
def test_epoch0(ctx, decode, case):
    """a span whose first cell is at timestamp 0 (as span 0, as a later span,
    as the only span): Span.addRow throws while the rows are scanned, on the
    thread-per-span assembly"""
    g = td.epoch0(case)
    for agg, rate, interval in ((SUM, False, 0), (MAX, True, 0), (AVG, False, 60)):
        for exact in (False, True):
            run(ctx, g, agg, rate, interval, SUM, exact)
            assert ref(g, agg, rate, interval, SUM).code == (0 if case == "none" else _abi.E_OUT_OF_BOUNDS)
    if case != "none":
        run(ctx, g, SUM, start=4, end=8)  # whatever the window


def rows5(first):
    """one span of five hourly rows (the wave walk: more than the thread-per-
    span assembly's four) whose first cell is at `first`, next to a plain one"""
    a = [(first + 7 * i, i) for i in range(3)] + [(3600 * h + 11 * i, h * i) for h in range(1, 5) for i in range(1, 4)]
    return Group("EPOCH0", "rows5", [(td.IM, [(10 + 5 * i, i) for i in range(9)]), (td.IM, a)], first=first)


@pytest.mark.parametrize("first", [0, 1])
def test_epoch0_wave_walk(ctx, decode2, first):
    g = rows5(first)
    assert len(g.spans[1]) == 5
    for agg, rate, interval in ((SUM, False, 0), (AVG, True, 0), (MIN, False, 60)):
        run(ctx, g, agg, rate, interval, SUM)
        assert ref(g, agg, rate, interval, SUM).code == (_abi.E_OUT_OF_BOUNDS if first == 0 else 0)


def test_epoch0_streaming_forms(ctx):
    """a one_row group from timestamp 0 on the aligned group's direct form (no
    assembly: dir_key refuses the span and the call runs again from assembly)
    and under lockstep=always"""
    for opt, val, default, q in (("group_direct", "always", "on", (AVG, False, 60, SUM)),
                                 ("lockstep", "always", "on", (SUM, False, 0, 0))):
        ctx.set_option(opt, val)
        try:
            for step in (1, 2):
                g = td.one_row("EPOCH0", step)
                p = run(ctx, g, *q)
                assert ref(g, *q).code == _abi.E_OUT_OF_BOUNDS and not p & (UNI | LS | AG), hex(p)
        finally:
            ctx.set_option(opt, default)


@pytest.mark.timeout(120)
def test_epoch0_three_ranks(mctx):
    for direct in ("on", "always"):  # ("always": the sharded direct form's own refusal, dir_key)
        mctx.set_option("group_direct", direct)
        try:
            for g in (td.one_row("EPOCH0", 2), td.epoch0("later")):
                for q in ((SUM, False, 0, 0), (AVG, False, 60, SUM)):
                    run(mctx, g, *q)
                    assert ref(g, *q).code == _abi.E_OUT_OF_BOUNDS
        finally:
            mctx.set_option("group_direct", "on")


def past32_fails(c, g, agg=SUM, rate=False, interval=0, start=0, end=U32MAX, exact=False):
    """the contract (include/tsdbhip.h): E_INVALID_ARG from the assembly stage,
    nothing emitted, whatever the window. That no decode kernel ran follows
    from reading (an unsharded call throws at its first host round trip, right
    after assembly); the paths word checked here is a proxy: no streaming path
    finished the call."""
    res = core.run_spanset(c, g.ss, start, end, agg, rate, interval, SUM, exact=exact)
    assert res[0] == _abi.E_INVALID_ARG and len(res[1]) == 0 and res[5] == 0, (res[0], len(res[1]), res[5])
    p = c.timing().paths
    assert not p & (UNI | LS | AG), hex(p)  # (no streaming kernel completed the call)


# (inner_*: the cell beyond 2^32 is not its row's last, the row's cells out of order: the guard
# looks at every qualifier of a row that can hold such a cell)
PAST32_GROUPS = {"alone": lambda: td.past32(False), "second": lambda: td.past32(True),
                 "one_row": lambda: td.past32_one_row(), "inner_one_row": lambda: td.past32_inner("one_row"),
                 "inner_rows": lambda: td.past32_inner("rows")}


@pytest.mark.parametrize("which", sorted(PAST32_GROUPS))
def test_past32(ctx, decode, which):
    g = PAST32_GROUPS[which]()
    for end in (U32MAX, 1 << 33):
        for interval in (0, 60):
            for rate in (False, True):
                past32_fails(ctx, g, SUM, rate, interval, end=end)
    past32_fails(ctx, g, AVG, exact=True)
    past32_fails(ctx, g, start=TOP + 1700, end=TOP + 1750)  # (a window of cells beyond 2^32 only)
    past32_fails(ctx, g, start=0, end=TOP)                  # (a window that ends before them)
    past32_fails(ctx, g, start=P32, end=1 << 40)


def test_past32_streaming_forms(ctx):
    g = td.past32_one_row()
    for opt, val, default, q in (("group_direct", "always", "on", (AVG, False, 60)),
                                 ("lockstep", "always", "on", (SUM, False, 0)),
                                 ("lockstep", "always", "on", (MAX, True, 0))):
        ctx.set_option(opt, val)
        try:
            past32_fails(ctx, g, *q)
        finally:
            ctx.set_option(opt, default)


def test_past32_batch(ctx):
    groups = [td.one_row("TOP", 2, S=9), td.past32(True), td.one_row("T31", 2, S=11)]
    b, gss = batch_of(groups)
    inner = corrupt_qual(b.ss, 3, 300, lambda q: (1700 << 4) | (q & 0xF))  # (an inner cell of group 0 as well)
    rc, res = core.run_spanset_batch(ctx, inner, gss, 0, U32MAX, SUM)
    assert rc == _abi.E_INVALID_ARG and [r[0] for r in res] == [_abi.E_INVALID_ARG, _abi.E_INVALID_ARG, 0]
    for agg, rate, interval, dsa in BATCH_QUERIES:
        rc, res = core.run_spanset_batch(ctx, b.ss, gss, 0, U32MAX, agg, rate, interval, dsa)
        assert rc == _abi.E_INVALID_ARG
        assert (res[1][0], len(res[1][1]), res[1][5]) == (_abi.E_INVALID_ARG, 0, 0)
        for k in (0, 2):
            assert_same(res[k], ref(groups[k], agg, rate, interval, dsa))


@pytest.mark.timeout(120)
def test_past32_three_ranks(mctx):
    for direct in ("on", "always"):
        mctx.set_option("group_direct", direct)
        try:
            for g in (td.past32_one_row(), td.past32(True), td.past32_inner("one_row"), td.past32_inner("rows")):
                for q in ((SUM, False, 0), (SUM, True, 0), (AVG, False, 60)):
                    past32_fails(mctx, g, *q)
        finally:
            mctx.set_option("group_direct", "on")


def test_end_and_start_beyond_u32max(ctx, decode2):
    """end_time above 2^32 - 1 is 2^32 - 1; a start_time above it keeps no span"""
    for g in (td.one_row("TOP", 1), td.jittered("TOP")):
        for agg, interval in ((SUM, 0), (AVG, 60)):
            a = core.run_spanset(ctx, g.ss, 0, U32MAX, agg, False, interval, SUM)
            pa = ctx.timing().paths
            for end in (P32, 1 << 33, 1 << 40):
                b = core.run_spanset(ctx, g.ss, 0, end, agg, False, interval, SUM)
                assert pa == ctx.timing().paths
                assert a[0] == b[0] == 0 and all((x == y).all() for x, y in zip(a[1:4], b[1:4])) and a[4] == b[4]
                run(ctx, g, agg, False, interval, SUM, end=end)
            for start in (P32, 1 << 40):
                run(ctx, g, agg, False, interval, SUM, start=start, end=1 << 41)
