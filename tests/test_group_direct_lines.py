"""The chunk loaders of the direct aligned group (reg_run in k_ds_reg.hip,
option "group_direct_load"): `rows` has a lane load its own 8 cells, `lines_nt`
has a wave instruction load 1 KB contiguous (non-temporal) and transposes the
chunk through LDS into the same layout. Results
never depend on the loader: every case runs for each loader in the tree, at 1
and 4 spans a wave, integers bit-exact against the oracle, taken or fallen
back as tests/test_group_direct.py defines it; timing.paths bit
PATH_GROUP_DIRECT_LINES says which kind of loader ran. The new
tsdbhip_bw_probe modes (4-7) run on a small device descriptor."""
import ctypes as C

import pytest

import oracle
import value_domains as vd
from helpers import I, T0, U32MAX, assert_same, corrupt_qual, run_both, with_option
from opentsdb_amd import _abi, core, packing, synth
from opentsdb_amd._lib import TsdbHipError

pytestmark = pytest.mark.gpu
I64 = _abi.SYN_INT64_COUNTER
GD, GDF, GDL = _abi.PATH_GROUP_DIRECT, _abi.PATH_GROUP_DIRECT_FALLBACK, _abi.PATH_GROUP_DIRECT_LINES
LOADS = ["rows", "lines_nt"]  # (every value but "auto", which is one of them)
RUNS = [1, 4]


@pytest.fixture(autouse=True)
def always(request):
    yield from with_option(request, "group_direct", "always", "on")


@pytest.fixture(params=LOADS)
def load(request, ctx):
    ctx.set_option("group_direct_load", request.param)
    yield request.param
    ctx.set_option("group_direct_load", "auto")


@pytest.fixture(params=RUNS, ids=lambda r: f"run{r}")
def run(request, ctx):
    ctx.set_option("group_direct_run", str(request.param))
    yield request.param
    ctx.set_option("group_direct_run", "auto")


def taken(c, load):
    p = c.timing().paths
    return bool(p & GD) and not p & GDF and bool(p & _abi.PATH_ALIGNED_GROUP) and bool(p & GDL) == load.startswith("lines")


def fell_back(c, load):
    p = c.timing().paths
    return bool(p & GDF) and not p & GD and bool(p & GDL) == load.startswith("lines")


# a group and the oracle's answers to the queries made of it: built once,
# shared by the loaders and the run lengths, never changed
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


def rows8(ts, vals):
    return I(list(zip(ts, vals)), minimal=False)


# ---- 1. taken ----

@pytest.mark.parametrize("n", [2, 3, 16, 127, 128, 129, 255, 256, 257, 511, 512, 513, 640, 1040])
def test_taken_cells_per_span(ctx, load, run, n):
    """one piece; the 128-cell edge of a load instruction; the 256-cell one
    (4-byte cells'); the chunk edge; a chunk and exactly one instruction; two
    chunks and a 16-cell tail (3600 cells' shape). Step 2 with 60-s buckets: a
    partial last bucket"""
    for dsa in (0, 1, 3):
        check(ctx, ("cells", run, n), lambda: synth.regular(8 * run + 3, n, I64, seed=5, step=2), 0, dsa)
        assert taken(ctx, load)


@pytest.mark.parametrize("n", [255, 256, 257, 600])
def test_taken_four_byte_integers(ctx, load, run, n):
    # (values past 2^16 and inside int32: every cell 4 bytes wide)
    def make():
        return packing.pack_spans([I([(T0 + 2 * i, 1_000_000 + 13 * i * (s + 1) - 70_000 * (s % 3)) for i in range(n)])
                                   for s in range(19)])
    for agg, dsa in ((0, 3), (1, 0), (2, 1)):
        check(ctx, ("four", n), make, agg, dsa)
        assert taken(ctx, load)


@pytest.mark.parametrize("agg", [0, 1, 2, 3])
def test_taken_aggregators(ctx, load, run, agg):
    for dsa in (0, 1, 3):
        check(ctx, "aggs", lambda: synth.regular(37, 1040, I64, seed=12, step=1), agg, dsa)
        assert taken(ctx, load)


def test_taken_span_counts(ctx, load, run):
    """around the run's and the block's (4 runs) edges; 700 cells: a full
    chunk and a tail"""
    R = run
    for n_spans in sorted({1, R - 1, R, R + 1, 4 * R - 1, 4 * R, 4 * R + 1, 8 * R + 3} - {0}):
        check(ctx, ("count", n_spans), lambda: synth.regular(n_spans, 700, I64, seed=7 + n_spans, step=1), 0, 3)
        assert taken(ctx, load), n_spans


def test_auto_is_taken(ctx, run):
    ctx.set_option("group_direct_load", "auto")
    check(ctx, "aggs", lambda: synth.regular(37, 1040, I64, seed=12, step=1), 0, 3)
    p = ctx.timing().paths
    assert p & GD and not p & GDF


# ---- 2. values that show a misplaced cell ----

@pytest.mark.parametrize("pool", ["WRAP64", "NEG"])
def test_value_pools(ctx, load, run, pool):
    """extreme and negative longs, 600 cells (a chunk and a tail of 88): a
    bucket's min and max name the cells it holds"""
    g = vd.one_row(pool, 1, S=35)
    for agg, dsa in ((0, 0), (0, 1), (0, 2), (0, 3), (1, 1), (2, 2)):
        check(ctx, ("pool", pool), lambda: g.ss, agg, dsa)
        assert taken(ctx, load)


def scrambled(c, s):
    """distinct per cell, not linear in it"""
    return ((c * c * 2654435761 + 40503 * s) ^ (c << 23)) % (1 << 40) - (1 << 39) + c


def spike_group(n=640):
    """span 0 scrambled values; the others small values and one large one: in
    cell n - 1, in cell 128 k - 1 (the last cell of a load instruction's
    range, k = 1 .. 5), in cell 128 k (the first of the next)"""
    spans = [rows8(range(T0, T0 + n), [scrambled(c, 0) for c in range(n)])]
    for at in [n - 1] + [128 * k - 1 for k in range(1, 6)] + [128 * k for k in range(1, 5)]:
        v = [c % 7 for c in range(n)]
        v[at] = (1 << 50) + at
        spans.append(rows8(range(T0, T0 + n), v))
        v = [-(c % 5) for c in range(n)]
        v[at] = -(1 << 50) - at
        spans.append(rows8(range(T0, T0 + n), v))
    return packing.pack_spans(spans)


@pytest.mark.parametrize("interval", [10, 60])
def test_spikes_stay_in_their_cells(ctx, load, run, interval):
    """640 cells: a chunk plus exactly one instruction; 10-s buckets (64 of
    them) place a cell within 10, min and max over the spans keep the spikes"""
    for agg, dsa in ((0, 0), (1, 1), (2, 2), (0, 2), (0, 1), (0, 3)):
        check(ctx, "spikes", spike_group, agg, dsa, interval)
        assert taken(ctx, load)


# ---- 3. the buffer's end ----

@pytest.mark.parametrize("n", [2, 129, 513])
def test_last_row_ends_the_buffer(ctx, load, run, n):
    """pack_spans' layout: the descriptor's last row ends where val_bytes
    ends (its length rounded up to 16 B), and a lane past the row's end reads
    the piece that holds its last cell"""
    def make():
        ss = packing.pack_spans([rows8(range(T0, T0 + n), [scrambled(c, s) for c in range(n)]) for s in range(9)])
        r = ss.n_rows - 1
        assert 0 <= len(ss.val_bytes) - (int(ss.row_val_off[r]) + int(ss.row_val_len[r])) < 16  # (the buffer's length is rounded up to 16 B)
        return ss
    for agg, dsa in ((0, 0), (1, 1), (2, 2), (0, 3)):
        check(ctx, ("end", n), make, agg, dsa, 10)
        assert taken(ctx, load)


# ---- 4. tried and fell back, the call state clean after it ----

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
        p = ctx.timing().paths
        assert p & GD and not p & GDF
        g, o = run_both(ctx, synth.regular(3, 16, I64, seed=2, step=1), 0, U32MAX, 0, False, 60, 3)
        assert_same(g, o)
    finally:
        ctx.set_option("check_clean", "off")
    assert "TSDBHIP_CHECK_CLEAN" not in capfd.readouterr().err


def run_of(n, R, g):
    """the spans wave g takes in a group of n spans at run length R"""
    return list(range(g, n, 4 * ((n + 4 * R - 1) // (4 * R))))


@pytest.mark.parametrize("cell", [77, 128, 511, 600, 1100, 1799], ids=lambda c: f"cell{c}")
def test_fell_back_inside_a_run(ctx, load, run, clean, cell):
    """a qualifier off the cadence in the first, a middle and the last chunk
    (1800 cells: 512 + 512 + 512 + 264) of a middle span of a wave's run:
    only the streaming wave sees it"""
    n = 10 * run + 2
    r = run_of(n, run, 3)
    span = r[len(r) // 2]
    for agg in (0, 2):
        check(ctx, ("bad", run, cell),
              lambda: corrupt_qual(synth.regular(n, 1800, I64, seed=2, step=2), span, cell, lambda q: q + 16), agg, 3)
        assert fell_back(ctx, load)


# ---- 5. the option and the probes ----

def test_option_values(ctx):
    for v in ["auto"] + LOADS + ["auto"]:
        ctx.set_option("group_direct_load", v)
    for v in ("", "lines", "rows_nt", "LINES_NT", "nt", "2"):
        with pytest.raises(TsdbHipError) as e:
            ctx.set_option("group_direct_load", v)
        assert e.value.code == _abi.E_INVALID_ARG


def test_probe_modes(ctx):
    L = ctx._lib
    d = _abi.SgDesc()
    p = _abi.SynthParams(seed=3, n_spans=64, n_points=700, t0=T0, step=1, kind=I64, span0=0)
    ctx.check(L.tsdbhip_synth_generate(ctx.handle, C.byref(p), C.byref(d)))
    try:
        ms, nb = C.c_float(), C.c_uint64()
        for mode in (4, 5, 6, 7):
            ms.value, nb.value = 0.0, 0
            assert L.tsdbhip_bw_probe(ctx.handle, C.byref(d), mode, 8, C.byref(ms), C.byref(nb)) == 0
            want = d.val_nbytes // 16 * 16 if mode == 7 else d.qual_nbytes + d.val_nbytes
            assert nb.value == want and ms.value > 0, mode
        for mode in (-1, 8, 10, 1 << 20):
            assert L.tsdbhip_bw_probe(ctx.handle, C.byref(d), mode, 8, C.byref(ms), C.byref(nb)) == _abi.E_INVALID_ARG
    finally:
        L.tsdbhip_synth_free(ctx.handle, C.byref(d))
