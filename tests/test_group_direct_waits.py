"""The chunk stream of the direct aligned group (reg_run in k_ds_reg.hip) at
its rows' ends, and the launch's grid rule (ug_direct_grid in api.hip).

A value load instruction of a chunk covers 128 cells (W = 8) or 256 (W = 4);
what a chunk's loader does with an instruction whose whole range lies past the
row's end (skip it, or clamp it into the row) must not show. So the
cells-a-span values below sit where an instruction's range ends at, just
before or just after the row's end, with the span last in the value buffer.
Values are distinct per cell, so a stale or misplaced cell changes a bucket's
min, max or sum.

"group_direct_run=fill" (what "auto" is) launches min(ceil(n / 4), resident
blocks) blocks, wave g of the G launched streaming spans g, g + G, ... to the
group's end; "group_direct_blocks" stands in for the resident blocks, so that
small groups reach long strided runs, waves with no span and unequal shares.

Integers bit-exact against the oracle; taken or fallen back as
tests/test_group_direct_runs.py defines it."""
import numpy as np
import pytest

import oracle
from helpers import F, I, T0, U32MAX, assert_same, corrupt_qual, run_both, with_option
from opentsdb_amd import _abi, core, packing, synth
from opentsdb_amd._lib import TsdbHipError
from test_group_direct_runs import fell_back, paths, regular_spans, rows8, taken

pytestmark = pytest.mark.gpu
I64 = _abi.SYN_INT64_COUNTER
LOADS = ["rows", "lines_nt"]
QUERIES = ((0, 0), (1, 1), (2, 2), (0, 3))  # (aggregator, downsampler): sum, min, max, avg


@pytest.fixture(autouse=True)
def always(request):
    yield from with_option(request, "group_direct", "always", "on")


@pytest.fixture(params=LOADS)
def load(request, ctx):
    ctx.set_option("group_direct_load", request.param)
    yield request.param
    ctx.set_option("group_direct_load", "auto")


def set_grid(c, run, blocks="auto"):
    c.set_option("group_direct_run", str(run))
    c.set_option("group_direct_blocks", str(blocks))


@pytest.fixture(params=[("auto", "auto"), ("fill", 1)], ids=["wave_a_span", "fill1"])
def grid(request, ctx):
    """a span a wave (what "auto" gives a group this small), and one block
    whose four waves stream the whole group: a span's last chunk is followed
    by the next span's first in the same register sets"""
    set_grid(ctx, *request.param)
    yield request.param
    set_grid(ctx, "auto")


@pytest.fixture(params=[1, 2], ids=lambda b: f"blocks{b}")
def fill(request, ctx):
    set_grid(ctx, "fill", request.param)
    yield request.param
    set_grid(ctx, "auto")


# a group and the oracle's answers to the queries made of it: built once,
# shared by the loaders and the grids, never changed
_GROUPS = {}


def check(ctx, key, make, agg, dsa, interval=60):
    if key not in _GROUPS:
        _GROUPS[key] = (make(), {})
    ss, refs = _GROUPS[key]
    q = (agg, dsa, interval)
    if q not in refs:
        refs[q] = oracle.spangroup(ss, 0, U32MAX, agg, False, interval, dsa)
    assert_same(core.run_spanset(ctx, ss, 0, U32MAX, agg, False, interval, dsa), refs[q])
    return refs[q]


def scrambled8(c, s):
    """distinct per cell, not linear in it, 8 bytes wide"""
    return ((c * c * 2654435761 + 40503 * s) ^ (c << 23)) % (1 << 40) - (1 << 39) + c


def scrambled4(c, s):
    """distinct per cell (an odd multiplier modulo 2^30), past 2^16 and inside
    int32: every cell 4 bytes wide"""
    return 70_000 + (c * 2654435761 + 40503 * s) % (1 << 30)


def ends_the_buffer(ss):
    r = ss.n_rows - 1
    assert 0 <= len(ss.val_bytes) - (int(ss.row_val_off[r]) + int(ss.row_val_len[r])) < 16
    return ss


# ---- 1. row ends ----

@pytest.mark.parametrize("n", [2, 16, 127, 128, 129, 256, 511, 512, 513, 528, 1040])
def test_row_ends_eight_byte_cells(ctx, load, grid, n):
    """the last span ends val_bytes (a host descriptor: copied with 64 B of
    slack behind it); step 2 with 60-s buckets: a partial last bucket"""
    def make():
        return ends_the_buffer(packing.pack_spans(
            [rows8(range(T0, T0 + 2 * n, 2), [scrambled8(c, s) for c in range(n)]) for s in range(9)]))
    for agg, dsa in QUERIES:
        check(ctx, ("w8", n), make, agg, dsa)
        assert taken(ctx)


@pytest.mark.parametrize("n", [2, 255, 256, 257, 512, 513, 1040])
def test_row_ends_four_byte_cells(ctx, load, grid, n):
    def make():
        ss = packing.pack_spans([I([(T0 + 2 * c, scrambled4(c, s)) for c in range(n)]) for s in range(9)])
        assert int(ss.row_val_len[0]) == 4 * n + 1
        return ends_the_buffer(ss)
    for agg, dsa in QUERIES:
        check(ctx, ("w4", n), make, agg, dsa)
        assert taken(ctx)


# ---- 2. one generation of blocks ----

@pytest.mark.parametrize("cells", [700, 1040])
def test_fill_span_counts(ctx, fill, cells):
    """fewer spans than waves (waves with no span), one more than the waves,
    shares of n / G and n / G + 1 spans, runs of up to 17 spans"""
    for n_spans in (1, 3, 4, 5, 8, 9, 29, 67):
        check(ctx, ("count", n_spans, cells), lambda: synth.regular(n_spans, cells, I64, seed=7 + n_spans, step=1), 0, 3)
        assert taken(ctx), n_spans


def test_fill_aggregators(ctx, fill):
    for agg in (0, 1, 2, 3):
        for dsa in (0, 1, 3):
            check(ctx, "aggs", lambda: synth.regular(37, 1040, I64, seed=12, step=1), agg, dsa)
            assert taken(ctx)


def test_run_of_64(ctx):
    """67 spans at 64 a wave: one block, runs of 17, 17, 17 and 16"""
    set_grid(ctx, 64)
    try:
        for agg, dsa in QUERIES:
            check(ctx, ("count", 67, 700), lambda: synth.regular(67, 700, I64, seed=7 + 67, step=1), agg, dsa)
            assert taken(ctx)
    finally:
        set_grid(ctx, "auto")


def test_auto_is_taken(ctx):
    set_grid(ctx, "auto")
    check(ctx, ("auto", 21), lambda: synth.regular(21, 1040, I64, seed=3, step=1), 0, 3)
    assert taken(ctx)


# ---- 3. tried and fell back, the call state clean after it ----

@pytest.fixture
def clean(ctx, capfd):
    """ "check_clean" compares the call state with its initial values at the
    start of every call (a line on stderr when it differs): a good call after
    the test's last one checks that one's state too"""
    ctx.set_option("check_clean", "on")
    try:
        yield
        g, o = run_both(ctx, synth.regular(9, 700, I64, seed=2, step=1), 0, U32MAX, 0, False, 60, 3)
        assert_same(g, o)
        assert taken(ctx)
    finally:
        ctx.set_option("check_clean", "off")
    assert "TSDBHIP_CHECK_CLEAN" not in capfd.readouterr().err


N_BROKEN = 29


def third_of_a_run(blocks, g=1):
    """the third span of wave g's run in a group of 29 spans on `blocks` blocks"""
    G = 4 * min((N_BROKEN + 3) // 4, blocks)
    r = list(range(g, N_BROKEN, G))
    assert len(r) >= 3
    return r[2]


def fallen(ctx, ss, aggs=(0, 2)):
    for agg in aggs:
        g, o = run_both(ctx, ss, 0, U32MAX, agg, False, 60, 3)
        assert_same(g, o)
        assert fell_back(ctx)
    return o


@pytest.mark.parametrize("other", ["length", "first", "step"])
def test_fill_fell_back_other_class(ctx, fill, clean, other):
    spans = regular_spans(N_BROKEN, 1200)
    spans[third_of_a_run(fill)] = {"length": rows8(range(T0, T0 + 1199), range(1199)),
                                   "first": rows8(range(T0 + 1, T0 + 1201), range(1200)),
                                   "step": rows8(range(T0, T0 + 2400, 2), range(1200))}[other]
    fallen(ctx, packing.pack_spans(spans))


def test_fill_fell_back_float_span(ctx, fill, clean):
    rng = np.random.default_rng(2)
    spans = regular_spans(N_BROKEN, 1200)
    spans[third_of_a_run(fill)] = F([(t, float(v)) for t, v in zip(range(T0, T0 + 1200), rng.standard_normal(1200))])
    fallen(ctx, packing.pack_spans(spans), aggs=(0,))


def test_fill_fell_back_two_row_span(ctx, fill, clean):
    """as many rows as spans: one span empty, the third of a run of two rows;
    the empty span's error comes out as the oracle's"""
    spans = regular_spans(N_BROKEN, 1200)
    spans[third_of_a_run(fill, g=2)] = []
    spans[third_of_a_run(fill)] = rows8(range(T0 + 3000, T0 + 4200), range(1200))
    ss = packing.pack_spans(spans)
    assert ss.n_rows == ss.n_spans
    o = fallen(ctx, ss, aggs=(0,))
    assert o.code != 0


def test_fill_fell_back_middle_qualifier(ctx, fill, clean):
    """a middle qualifier off the cadence in a chunk that is loaded while the
    span before it streams"""
    fallen(ctx, corrupt_qual(synth.regular(N_BROKEN, 1800, I64, seed=2, step=2), third_of_a_run(fill), 600,
                             lambda q: q + 16))


# ---- 4. sharded, in process (3 ranks on one device) ----

@pytest.fixture(scope="module")
def mctx():
    from opentsdb_amd._lib import Context
    c = Context(devices=[0, 0, 0])
    c.set_option("group_direct", "always")
    yield c
    c.close()


@pytest.fixture(params=[1, 2], ids=lambda b: f"blocks{b}")
def mfill(request, mctx):
    set_grid(mctx, "fill", request.param)
    yield request.param
    set_grid(mctx, "auto")


def both(c, ss, agg):
    return (core.run_spanset(c, ss, 0, U32MAX, agg, False, 60, 3), oracle.spangroup(ss, 0, U32MAX, agg, False, 60, 3))


@pytest.mark.timeout(120)
def test_sharded_all_ranks_fill(mctx, mfill):
    ss = synth.regular(30, 1040, I64, seed=9, step=1)
    for agg in (0, 1, 2, 3):
        g, o = both(mctx, ss, agg)
        assert_same(g, o)
        assert taken(mctx) and paths(mctx) & _abi.PATH_UNIFORM
        assert mctx.timing().n_collectives == 1


@pytest.mark.timeout(120)
def test_sharded_one_shard_breaks_inside_a_run(mctx, mfill):
    """span 19 is the last of the second rank's ten: the last span of its
    wave's run (spans 1, 5, 9 of the shard on one block; 1, 9 on two). Every
    rank falls back (the validity is agreed), results and aggregatedSize the
    oracle's"""
    ss = corrupt_qual(synth.regular(30, 1800, I64, seed=4, step=2), 19, 1000, lambda q: q + 16)
    g, o = both(mctx, ss, 0)
    assert_same(g, o)
    assert g[4] == o.n_input_points
    assert fell_back(mctx) and paths(mctx) & _abi.PATH_UNIFORM_FALLBACK


# ---- 5. the options ----

def test_option_values(ctx):
    try:
        for v in ("fill", "64", "128", "256", "32", "1", "auto"):
            ctx.set_option("group_direct_run", v)
        for v in ("1", "2", "1024", "auto"):
            ctx.set_option("group_direct_blocks", v)
        for name, bad in (("group_direct_run", ("", "0", "3", "512", "FILL", "-1")),
                          ("group_direct_blocks", ("", "0", "-1", "x", "1.5", "fill"))):
            for v in bad:
                with pytest.raises(TsdbHipError) as e:
                    ctx.set_option(name, v)
                assert e.value.code == _abi.E_INVALID_ARG
    finally:
        set_grid(ctx, "auto")
