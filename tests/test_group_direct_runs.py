"""Runs of spans in the direct aligned group (ds_reg_direct_body / reg_run in
k_ds_reg.hip): a wave of k_ug_ds_reg's direct instantiation streams a run of
`group_direct_run` one-row spans as one chunk stream (wave g of the launch's
G = 4 ceil(n / 4 run) waves: spans g, g + G, ...), the next span's fields and
first chunk loaded while the present one streams, and the block pays its
partial atomics and its done count once per 4 runs. Results
never depend on the run length: every case runs at 1, 2 and 4 spans a wave,
integers bit-exact against the oracle, taken or fallen back as
tests/test_group_direct.py defines it."""
import numpy as np
import pytest

from helpers import F, I, T0, U32MAX, assert_same, corrupt_qual, run_both, with_option
from opentsdb_amd import _abi, core, packing, synth

pytestmark = pytest.mark.gpu
I64 = _abi.SYN_INT64_COUNTER
GD, GDF = _abi.PATH_GROUP_DIRECT, _abi.PATH_GROUP_DIRECT_FALLBACK
RUNS = [1, 2, 4]


@pytest.fixture(autouse=True)
def always(request):
    yield from with_option(request, "group_direct", "always", "on")


@pytest.fixture(params=RUNS, ids=lambda r: f"run{r}")
def run(request, ctx):
    ctx.set_option("group_direct_run", str(request.param))
    yield request.param
    ctx.set_option("group_direct_run", "auto")


def paths(c):
    return c.timing().paths


def taken(c):
    p = paths(c)
    return bool(p & GD) and not p & GDF and bool(p & _abi.PATH_ALIGNED_GROUP)


def fell_back(c):
    p = paths(c)
    return bool(p & GDF) and not p & GD


def rows8(ts, vals):
    return I(list(zip(ts, vals)), minimal=False)


def regular_spans(n, cells, t0=T0, step=1):
    return [rows8(range(t0, t0 + cells * step, step), range(7 * s, 7 * s + cells)) for s in range(n)]


# ---- 1. taken ----

def test_taken_span_counts(ctx, run):
    """around the run's and the block's (4 runs) edges; 700 cells: a full
    chunk and a tail, so a run goes from span to span with loads in flight"""
    R = run
    for n_spans in sorted({1, R - 1, R, R + 1, 4 * R - 1, 4 * R, 4 * R + 1, 8 * R + 3} - {0}):
        ss = synth.regular(n_spans, 700, I64, seed=7 + n_spans, step=1)
        g, o = run_both(ctx, ss, 0, U32MAX, 0, False, 60, 3)
        assert_same(g, o)
        assert taken(ctx), n_spans


@pytest.mark.parametrize("n", [2, 16, 511, 512, 513, 1040])
def test_taken_cells_per_span(ctx, run, n):
    """below a lane's 8 cells, two lanes, around the 512-cell chunk, two full
    chunks and a 16-cell tail (3600 cells' shape); step 2 with 60-s buckets: a
    partial last bucket"""
    ss = synth.regular(8 * run + 3, n, I64, seed=5, step=2)
    for dsa in (0, 1, 3):
        g, o = run_both(ctx, ss, 0, U32MAX, 0, False, 60, dsa)
        assert_same(g, o)
        assert taken(ctx)


@pytest.mark.parametrize("agg", [0, 1, 2, 3])
def test_taken_aggregators(ctx, run, agg):
    ss = synth.regular(37, 1040, I64, seed=12, step=1)
    for dsa in (0, 1, 3):
        g, o = run_both(ctx, ss, 0, U32MAX, agg, False, 60, dsa)
        assert_same(g, o)
        assert taken(ctx)


def test_taken_four_byte_integers(ctx, run):
    # (values past 2^16 and inside int32: every cell 4 bytes wide)
    ss = packing.pack_spans([I([(T0 + 2 * i, 1_000_000 + 13 * i * (s + 1) - 70_000 * (s % 3)) for i in range(600)])
                             for s in range(19)])
    for agg, dsa in ((0, 3), (1, 0), (2, 1)):
        g, o = run_both(ctx, ss, 0, U32MAX, agg, False, 60, dsa)
        assert_same(g, o)
        assert taken(ctx)


def test_auto_run_is_taken(ctx):
    """ "auto" on a small group: one span a wave, the results the same"""
    ctx.set_option("group_direct_run", "auto")
    ss = synth.regular(21, 1040, I64, seed=3, step=1)
    g, o = run_both(ctx, ss, 0, U32MAX, 0, False, 60, 3)
    assert_same(g, o)
    assert taken(ctx)


# ---- 2. tried and fell back, the call state clean after it ----

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
        g, o = run_both(ctx, synth.regular(3, 16, I64, seed=2, step=1), 0, U32MAX, 0, False, 60, 3)
        assert_same(g, o)
    finally:
        ctx.set_option("check_clean", "off")
    assert "TSDBHIP_CHECK_CLEAN" not in capfd.readouterr().err


def fallen(ctx, ss, aggs=(0, 2)):
    for agg in aggs:
        g, o = run_both(ctx, ss, 0, U32MAX, agg, False, 60, 3)
        assert_same(g, o)
        assert fell_back(ctx)
    return o


def run_of(n, R, g):
    """the spans wave g takes in a group of n spans at run length R"""
    return list(range(g, n, 4 * ((n + 4 * R - 1) // (4 * R))))


def run_spans(R, g=3):
    """a group of 10 R + 2 spans (3 blocks: the last wave's runs are short),
    and the first, a middle and the last span of wave g's run"""
    n = 10 * R + 2
    r = run_of(n, R, g)
    assert r and len(r) >= R - 1
    return n, (r[0], r[len(r) // 2], r[-1])


@pytest.mark.parametrize("where", [0, 1, 2], ids=["first", "middle", "last"])
def test_fell_back_middle_qualifier(ctx, run, clean, where):
    """a middle qualifier off the cadence, which only the streaming wave sees"""
    n, at = run_spans(run)
    fallen(ctx, corrupt_qual(synth.regular(n, 1800, I64, seed=2, step=2), at[where], 900, lambda q: q + 16))


@pytest.mark.parametrize("cell", [100, 600], ids=["chunk0", "chunk1"])
def test_fell_back_prefetched_chunk(ctx, run, clean, cell):
    """a span that is not the first of its run: its chunks 0 and 1 are loaded
    while the span before it streams"""
    n, at = run_spans(run)
    for what in (lambda q: q + 16, lambda q: q | 0x8):
        fallen(ctx, corrupt_qual(synth.regular(n, 1800, I64, seed=4, step=2), at[2], cell, what), aggs=(0,))


def test_fell_back_two_row_span(ctx, run, clean):
    """as many rows as spans, one span empty and a later one of two rows,
    both inside runs: the empty span's error comes out as the oracle's"""
    n, at = run_spans(run)
    spans = regular_spans(n, 1200)
    spans[at[1]] = []
    spans[run_spans(run, g=6)[1][1]] = rows8(range(T0 + 3000, T0 + 4200), range(1200))
    ss = packing.pack_spans(spans)
    assert ss.n_rows == ss.n_spans
    o = fallen(ctx, ss, aggs=(0,))
    assert o.code != 0


def test_fell_back_float_span(ctx, run, clean):
    n, at = run_spans(run)
    rng = np.random.default_rng(2)
    spans = regular_spans(n, 1200)
    spans[at[1]] = F([(t, float(v)) for t, v in zip(range(T0, T0 + 1200), rng.standard_normal(1200))])
    fallen(ctx, packing.pack_spans(spans), aggs=(0,))


@pytest.mark.parametrize("other", ["length", "first", "step"])
def test_fell_back_other_class(ctx, run, clean, other):
    n, at = run_spans(run)
    spans = regular_spans(n, 1200)
    spans[at[2]] = {"length": rows8(range(T0, T0 + 1199), range(1199)),
                    "first": rows8(range(T0 + 1, T0 + 1201), range(1200)),
                    "step": rows8(range(T0, T0 + 2400, 2), range(1200))}[other]
    fallen(ctx, packing.pack_spans(spans), aggs=(0, 1))


@pytest.mark.parametrize("what", ["qualifier", "length"])
def test_fell_back_last_span_of_the_group(ctx, run, clean, what):
    n, _ = run_spans(run)
    if what == "qualifier":
        ss = corrupt_qual(synth.regular(n, 1800, I64, seed=6, step=2), n - 1, 1700, lambda q: q + 16)
    else:
        spans = regular_spans(n, 1200)
        spans[n - 1] = rows8(range(T0, T0 + 1100), range(1100))
        ss = packing.pack_spans(spans)
    fallen(ctx, ss, aggs=(0,))


# ---- 3. sharded, in process (3 ranks on one device) ----

@pytest.fixture(scope="module")
def mctx():
    from opentsdb_amd._lib import Context
    c = Context(devices=[0, 0, 0])
    c.set_option("group_direct", "always")
    yield c
    c.close()


@pytest.fixture(params=RUNS, ids=lambda r: f"run{r}")
def mrun(request, mctx):
    mctx.set_option("group_direct_run", str(request.param))
    yield request.param
    mctx.set_option("group_direct_run", "auto")


def both(c, ss, agg):
    import oracle
    return (core.run_spanset(c, ss, 0, U32MAX, agg, False, 60, 3), oracle.spangroup(ss, 0, U32MAX, agg, False, 60, 3))


@pytest.mark.timeout(120)
def test_sharded_all_ranks_direct(mctx, mrun):
    ss = synth.regular(30, 1040, I64, seed=9, step=1)
    for agg in (0, 1, 2, 3):
        g, o = both(mctx, ss, agg)
        assert_same(g, o)
        assert taken(mctx) and paths(mctx) & _abi.PATH_UNIFORM
        assert mctx.timing().n_collectives == 1


@pytest.mark.timeout(120)
def test_sharded_one_shard_breaks_inside_a_run(mctx, mrun):
    """span 19 is the last of the second rank's ten: the last span of its
    wave's run (spans 1, 9 at 2 spans a wave and 8 waves; 1, 5, 9 at 4 and 4).
    Every rank falls back (the validity is agreed), results and aggregatedSize
    the oracle's"""
    ss = corrupt_qual(synth.regular(30, 1800, I64, seed=4, step=2), 19, 1000, lambda q: q + 16)
    g, o = both(mctx, ss, 0)
    assert_same(g, o)
    assert g[4] == o.n_input_points
    assert fell_back(mctx) and paths(mctx) & _abi.PATH_UNIFORM_FALLBACK
