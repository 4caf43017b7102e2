"""The direct aligned group (group_direct_try in api.hip, ds_reg_direct_body
in k_ds_reg.hip): an aligned-group query over as many rows as spans starts
with the streaming kernel itself, k_ug_ds_reg's direct instantiation, which
derives from the descriptor and each row's first qualifier word what assembly
would have established (one row, its cells, first / last timestamp inside
[start, end], no seek, no `short` overflow, the class key) and proves every
other qualifier as it streams. No assembly kernel, no kept list, no host round
trip stand before it. A group that is not one row a span on one class does not
stand: the call runs again from assembly and must give the oracle's results
and errors. timing.paths: PATH_GROUP_DIRECT (taken), PATH_GROUP_DIRECT_FALLBACK
(tried, fell back). Integers bit-exact against the oracle in every case."""
import numpy as np
import pytest

from helpers import F, I, T0, U32MAX, assert_same, corrupt_qual, run_both, with_option
from opentsdb_amd import _abi, core, packing, synth

pytestmark = pytest.mark.gpu
I64 = _abi.SYN_INT64_COUNTER
GD, GDF = _abi.PATH_GROUP_DIRECT, _abi.PATH_GROUP_DIRECT_FALLBACK
KC_MAX = 4096  # (k_util.hip: groups beyond it take the tiled assembly, and "on" takes the direct group)


@pytest.fixture(autouse=True)
def always(request):
    """small groups: "always" tries the direct group whatever the span count"""
    yield from with_option(request, "group_direct", "always", "on")


def paths(c):
    return c.timing().paths


def taken(c):
    p = paths(c)
    return bool(p & GD) and not p & GDF and bool(p & _abi.PATH_ALIGNED_GROUP)


def fell_back(c):
    p = paths(c)
    return bool(p & GDF) and not p & GD


def untried(c):
    return not paths(c) & (GD | GDF)


def rows8(ts, vals):
    return I(list(zip(ts, vals)), minimal=False)


# ---- 1. taken ----

@pytest.mark.parametrize("agg", [0, 1, 2, 3])
@pytest.mark.parametrize("dsa", [0, 1, 2, 3])
def test_taken(ctx, agg, dsa):
    ss = synth.regular(200, 3600, I64, seed=12, step=1)
    g, o = run_both(ctx, ss, 0, U32MAX, agg, False, 60, dsa)
    assert_same(g, o)
    assert taken(ctx)


def test_taken_four_byte_integers(ctx):
    # (values past 2^16 and inside int32: every cell 4 bytes wide)
    ss = packing.pack_spans([I([(T0 + 2 * i, 1_000_000 + 13 * i * (s + 1) - 70_000 * (s % 3)) for i in range(300)])
                             for s in range(40)])
    for agg, dsa in ((0, 3), (1, 0), (2, 2), (3, 1)):
        g, o = run_both(ctx, ss, 0, U32MAX, agg, False, 60, dsa)
        assert_same(g, o)
        assert taken(ctx)


@pytest.mark.parametrize("n", [2, 63, 511, 512, 513, 1300])
def test_taken_cells_per_span(ctx, n):
    """below a lane's 8 cells, around the 512-cell chunk, several chunks; step
    2 with 60-s buckets: a partial last bucket"""
    ss = synth.regular(37, n, I64, seed=5, step=2)
    for dsa in (0, 1, 3):
        g, o = run_both(ctx, ss, 0, U32MAX, 0, False, 60, dsa)
        assert_same(g, o)
        assert taken(ctx)


@pytest.mark.parametrize("n_spans", [1, 3, 4, 5])
def test_taken_partial_last_block(ctx, n_spans):
    ss = synth.regular(n_spans, 700, I64, seed=7, step=1)
    for agg in (0, 1, 2, 3):
        g, o = run_both(ctx, ss, 0, U32MAX, agg, False, 60, 3)
        assert_same(g, o)
        assert taken(ctx)


def test_taken_by_the_automatic_rule(ctx):
    """ "on": more than KC_MAX spans of one row each"""
    ctx.set_option("group_direct", "on")
    ss = synth.regular(KC_MAX + 1, 64, I64, seed=9, step=1)
    g, o = run_both(ctx, ss, 0, U32MAX, 0, False, 60, 3)
    assert_same(g, o)
    assert taken(ctx)
    ss = synth.regular(KC_MAX, 64, I64, seed=9, step=1)  # (KC_MAX spans: the present path)
    g, o = run_both(ctx, ss, 0, U32MAX, 0, False, 60, 3)
    assert_same(g, o)
    assert untried(ctx)


# ---- 2. not eligible: the present path, the new bits clear ----

def test_rows_differ_from_spans(ctx):
    ss = packing.pack_spans([rows8(range(T0 + 3000, T0 + 4200), range(s, s + 1200)) for s in range(40)])
    assert ss.n_rows == 2 * ss.n_spans
    g, o = run_both(ctx, ss, 0, U32MAX, 0, False, 60, 3)
    assert_same(g, o)
    assert untried(ctx)


def test_off(ctx):
    ctx.set_option("group_direct", "off")
    ss = synth.regular(100, 3600, I64, seed=3, step=1)
    g, o = run_both(ctx, ss, 0, U32MAX, 0, False, 60, 3)
    assert_same(g, o)
    assert untried(ctx) and paths(ctx) & _abi.PATH_ALIGNED_GROUP


@pytest.mark.parametrize("kw", [dict(rate=True), dict(agg=4), dict(ds_agg=4), dict(exact=True)],
                         ids=["rate", "dev", "ds-dev", "exact-order"])
def test_other_queries(ctx, kw):
    ss = synth.regular(100, 1800, I64, seed=4, step=2)
    a = dict(agg=0, rate=False, ds_interval=60, ds_agg=3, exact=False)
    a.update(kw)
    g, o = run_both(ctx, ss, 0, U32MAX, **a)
    assert_same(g, o)
    assert untried(ctx)


# ---- 3. tried and fell back ----

@pytest.mark.parametrize("span", [0, 77, 119])
@pytest.mark.parametrize("what", ["delta+1", "float-flag", "width-4"])
def test_fell_back_middle_qualifier(ctx, span, what):
    """a middle qualifier off the cadence, which only the streaming wave sees"""
    fn = {"delta+1": lambda q: q + 16, "float-flag": lambda q: q | 0x8, "width-4": lambda q: (q & ~0x7) | 0x3}[what]
    ss = corrupt_qual(synth.regular(120, 1800, I64, seed=2, step=2), span, 900, fn)
    for agg in (0, 2):
        g, o = run_both(ctx, ss, 0, U32MAX, agg, False, 60, 3)
        assert_same(g, o)
        assert fell_back(ctx)


def regular_spans(n, cells, t0=T0, step=1):
    return [rows8(range(t0, t0 + cells * step, step), range(7 * s, 7 * s + cells)) for s in range(n)]


def test_fell_back_empty_and_two_row_span(ctx):
    """as many rows as spans, but one span holds none and another two: the
    empty span's error comes out as the oracle's"""
    spans = regular_spans(30, 1200)
    spans[11] = []
    spans[20] = rows8(range(T0 + 3000, T0 + 4200), range(1200))
    ss = packing.pack_spans(spans)
    assert ss.n_rows == ss.n_spans
    g, o = run_both(ctx, ss, 0, U32MAX, 0, False, 60, 3)
    assert o.code != 0
    assert_same(g, o)
    assert fell_back(ctx)


def test_fell_back_window(ctx):
    """`start` inside the spans (a seek); one span wholly after `end` (not kept)"""
    ss = synth.regular(50, 1800, I64, seed=6, step=2)
    g, o = run_both(ctx, ss, T0 + 10, U32MAX, 0, False, 60, 3)
    assert_same(g, o)
    assert fell_back(ctx)
    spans = regular_spans(30, 1200)
    spans[17] = rows8(range(T0 + 7200, T0 + 8400), range(1200))
    g, o = run_both(ctx, packing.pack_spans(spans), 0, T0 + 3599, 2, False, 60, 3)
    assert_same(g, o)
    assert fell_back(ctx)


def test_fell_back_float_span(ctx):
    rng = np.random.default_rng(2)
    spans = regular_spans(20, 1200)
    spans[9] = F([(t, float(v)) for t, v in zip(range(T0, T0 + 1200), rng.standard_normal(1200))])
    g, o = run_both(ctx, packing.pack_spans(spans), 0, U32MAX, 0, False, 60, 3)
    assert_same(g, o)
    assert fell_back(ctx)


@pytest.mark.parametrize("other", ["length", "first", "step"])
def test_fell_back_other_class(ctx, other):
    spans = regular_spans(25, 1200)
    spans[13] = {"length": rows8(range(T0, T0 + 1199), range(1199)),
                 "first": rows8(range(T0 + 1, T0 + 1201), range(1200)),
                 "step": rows8(range(T0, T0 + 2400, 2), range(1200))}[other]
    for agg in (0, 1):
        g, o = run_both(ctx, packing.pack_spans(spans), 0, U32MAX, agg, False, 60, 3)
        assert_same(g, o)
        assert fell_back(ctx)


def test_fell_back_more_than_64_buckets(ctx):
    ss = synth.regular(50, 3600, I64, seed=8, step=1)
    g, o = run_both(ctx, ss, 0, U32MAX, 0, False, 30, 3)
    assert_same(g, o)
    assert fell_back(ctx)


def test_fell_back_short_index_overflow(ctx):
    """a row of 4096 8-byte cells: 32768 value bytes, where RowSeq.Iterator's
    `short` value index overflows (100-s buckets: 41 of them, so nothing else
    refuses the span)"""
    row = lambda s: [synth.compact_cells(T0, synth.points_int(range(T0, T0 + 4096), range(s, s + 4096), False))]
    ss = packing.pack_spans([row(s) for s in range(12)])
    assert ss.n_rows == ss.n_spans and int(ss.row_val_len[0]) == 32769
    g, o = run_both(ctx, ss, 0, U32MAX, 0, False, 100, 3)
    assert_same(g, o)
    assert fell_back(ctx)


# ---- 4. the call state after each outcome ----

def test_state_after_each_outcome(ctx, capfd):
    """one context: a fell-back call, a taken call, a call on the present
    path; "check_clean" compares the call state with its initial values at
    the start of every call (a line on stderr when it differs)"""
    good = synth.regular(90, 1800, I64, seed=2, step=2)
    bad = corrupt_qual(good, 40, 900, lambda q: q + 16)
    ctx.set_option("check_clean", "on")
    try:
        for agg in (0, 1):
            g, o = run_both(ctx, bad, 0, U32MAX, agg, False, 60, 3)
            assert_same(g, o)
            assert fell_back(ctx)
            g, o = run_both(ctx, good, 0, U32MAX, agg, False, 60, 3)
            assert_same(g, o)
            assert taken(ctx)
            ctx.set_option("group_direct", "off")
            g, o = run_both(ctx, good, 0, U32MAX, agg, False, 60, 3)
            assert_same(g, o)
            assert untried(ctx)
            ctx.set_option("group_direct", "always")
        g, o = run_both(ctx, good, 0, U32MAX, 0, False, 60, 3)  # (its entry checks the last call's state)
        assert_same(g, o)
    finally:
        ctx.set_option("check_clean", "off")
    assert "TSDBHIP_CHECK_CLEAN" not in capfd.readouterr().err


# ---- 5. sharded, in process (3 ranks on one device) ----

@pytest.fixture(scope="module")
def mctx():
    from opentsdb_amd._lib import Context
    c = Context(devices=[0, 0, 0])
    c.set_option("group_direct", "always")
    yield c
    c.close()


def both(c, ss, agg):
    import oracle
    return (core.run_spanset(c, ss, 0, U32MAX, agg, False, 60, 3), oracle.spangroup(ss, 0, U32MAX, agg, False, 60, 3))


@pytest.mark.timeout(120)
@pytest.mark.parametrize("agg", [0, 1, 2, 3])
def test_sharded_all_ranks_direct(mctx, agg):
    ss = synth.regular(30, 3600, I64, seed=9, step=1)
    g, o = both(mctx, ss, agg)
    assert_same(g, o)
    assert taken(mctx) and paths(mctx) & _abi.PATH_UNIFORM
    assert mctx.timing().n_collectives == 1


@pytest.mark.timeout(120)
@pytest.mark.parametrize("span", [2, 14, 29])
def test_sharded_one_shard_breaks(mctx, span):
    """a middle qualifier off the cadence in one rank's shard: every rank
    falls back (the validity is agreed), results and aggregatedSize the
    oracle's"""
    ss = corrupt_qual(synth.regular(30, 1800, I64, seed=4, step=2), span, 1000, lambda q: q + 16)
    g, o = both(mctx, ss, 0)
    assert_same(g, o)
    assert g[4] == o.n_input_points
    assert fell_back(mctx) and paths(mctx) & _abi.PATH_UNIFORM_FALLBACK


@pytest.mark.timeout(120)
def test_sharded_one_rank_not_eligible(mctx):
    """one shard holds a span of two rows, so its rank assembles and launches
    speculatively while the others go direct: every rank must issue the same
    collectives. timing() is rank 0's: with the odd span in the last shard
    rank 0 went direct, with it in the first it did not — the two calls, and a
    call with no rank direct, count the same collectives."""
    def group(odd):
        spans = regular_spans(30, 1200)
        spans[odd] = rows8(range(T0 + 3000, T0 + 4200), range(1200))  # (as many cells: the shards stay 10 spans each)
        return packing.pack_spans(spans)
    n_coll = []
    for odd, rank0_direct in ((25, True), (4, False)):
        g, o = both(mctx, group(odd), 0)
        assert_same(g, o)
        assert bool(paths(mctx) & GDF) == rank0_direct and not paths(mctx) & GD
        assert paths(mctx) & _abi.PATH_UNIFORM_FALLBACK
        n_coll.append(mctx.timing().n_collectives)
    mctx.set_option("group_direct", "off")
    try:
        g, o = both(mctx, group(25), 0)
    finally:
        mctx.set_option("group_direct", "always")
    assert_same(g, o)
    assert untried(mctx)
    n_coll.append(mctx.timing().n_collectives)
    assert n_coll[0] == n_coll[1] == n_coll[2] > 0
