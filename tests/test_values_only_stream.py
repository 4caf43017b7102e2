"""The direct aligned group on a descriptor that carries
TSDBHIP_DESC_QUALS_PROVEN (reg_run's CERT instantiation, k_ds_reg.hip): the
launch reads each row's fields, its first qualifier word and its values, and
no other qualifier. timing.paths: PATH_QUALS_PROVEN beside PATH_GROUP_DIRECT.

That the qualifier stream is gone is shown by behaviour: a descriptor whose
qualifiers past the first word are wrong, flagged by hand (a false promise),
gives the results of the uncorrupted rows on the path, where the same
descriptor without the flag, or with "quals_proven" "off", falls back and
gives the oracle's answer for the bytes as they are. What depends on the query
or the class still falls back under the flag. Integers bit-exact against the
oracle in every case; "group_direct" is "always", as in test_group_direct.py."""
import ctypes as C

import numpy as np
import pytest

import oracle
from helpers import T0, U32MAX, assert_same, corrupt_qual, with_option
from opentsdb_amd import _abi, core, packing, synth
from test_values_only_certificate import upload
from test_group_direct import regular_spans, rows8

pytestmark = pytest.mark.gpu
I64 = _abi.SYN_INT64_COUNTER
QP, DQP = _abi.PATH_QUALS_PROVEN, _abi.DESC_QUALS_PROVEN
GD, GDF, GDL = _abi.PATH_GROUP_DIRECT, _abi.PATH_GROUP_DIRECT_FALLBACK, _abi.PATH_GROUP_DIRECT_LINES
AG = _abi.PATH_ALIGNED_GROUP
FALLBACKS = GDF | _abi.PATH_UNIFORM_FALLBACK | _abi.PATH_ALIGNED_RERUN | _abi.PATH_DIRECT_REDO


@pytest.fixture(autouse=True)
def always(request):
    yield from with_option(request, "group_direct", "always", "on")


@pytest.fixture(params=["lines_nt", "rows"])
def load(request):
    yield from with_option(request, "group_direct_load", request.param, "auto")


def run(c, d, agg, dsa, start=0, end=U32MAX, interval=60):
    """one query over the device descriptor; (result, paths)"""
    g = core.run_spanset(c, None, start, end, agg, False, interval, dsa, device_desc=d, capacity=1 << 16)
    assert g[0] not in (_abi.E_HIP, _abi.E_RCCL), c.last_error()
    return g, c.timing().paths


def ref(ss, agg, dsa, start=0, end=U32MAX, interval=60):
    return oracle.spangroup(ss, start, end, agg, False, interval, dsa)


def proven(ctx, ss):
    """`ss` uploaded and certified: a flagged device descriptor"""
    d, t = upload(ctx, ss)
    assert core.desc_certify(ctx, d) == (0, 0) and d.flags & DQP
    return d, t


def taken(p, what=""):
    assert p & (GD | AG | QP) == GD | AG | QP and not p & FALLBACKS, f"{what}: paths {p:#x}"


def fell_back(p, what=""):
    assert p & GDF and not p & GD, f"{what}: paths {p:#x}"


# ---- 1. taken, with the bit ----

_UP = {}


def shape(ctx, n_spans, n):
    k = (n_spans, n)
    if k not in _UP:
        ss = synth.regular(n_spans, n, I64, seed=5, step=2)
        _UP[k] = (ss, *proven(ctx, ss), {})
    return _UP[k]


def want(ctx, n_spans, n, agg, dsa):
    ss, _, _, refs = shape(ctx, n_spans, n)
    if (agg, dsa) not in refs:
        refs[agg, dsa] = ref(ss, agg, dsa)
    return refs[agg, dsa]


@pytest.mark.parametrize("n", [2, 63, 511, 512, 513, 1300])
def test_taken_shapes(ctx, load, n):
    """below a lane's 8 cells, around the 512-cell chunk, several chunks; step 2
    with 60-s buckets: a partial last bucket; 1 to 37 spans: a partial block"""
    for n_spans in (1, 3, 4, 5, 37):
        _, d, _, _ = shape(ctx, n_spans, n)
        for agg, dsa in ((0, 3), (1, 0), (2, 1), (3, 2)):
            g, p = run(ctx, d, agg, dsa)
            assert_same(g, want(ctx, n_spans, n, agg, dsa))
            taken(p, f"{n_spans} x {n} agg {agg} ds {dsa} {load}")
            assert bool(p & GDL) == (load == "lines_nt")


@pytest.mark.parametrize("agg", [0, 1, 2, 3])
@pytest.mark.parametrize("dsa", [0, 1, 2, 3])
def test_taken_every_aggregator(ctx, load, agg, dsa):
    _, d, _, _ = shape(ctx, 37, 1300)
    g, p = run(ctx, d, agg, dsa)
    assert_same(g, want(ctx, 37, 1300, agg, dsa))
    taken(p)


@pytest.mark.parametrize("blocks", ["1", "2"])
def test_taken_runs_of_spans(ctx, load, blocks):
    """one or two resident blocks: 4 or 8 waves, runs of up to 10 spans a wave"""
    ctx.set_option("group_direct_blocks", blocks)
    try:
        for n in (2, 63, 512, 513, 1300):
            _, d, _, _ = shape(ctx, 37, n)
            for agg, dsa in ((0, 3), (1, 0), (2, 1), (3, 2)):
                g, p = run(ctx, d, agg, dsa)
                assert_same(g, want(ctx, 37, n, agg, dsa))
                taken(p, f"37 x {n} agg {agg} ds {dsa} blocks {blocks} {load}")
    finally:
        ctx.set_option("group_direct_blocks", "auto")


def test_taken_four_byte_integers(ctx, load):
    # (values past 2^16 and inside int32: every cell 4 bytes wide; test_group_direct.py's group)
    from helpers import I
    ss = packing.pack_spans([I([(T0 + 2 * i, 1_000_000 + 13 * i * (s + 1) - 70_000 * (s % 3)) for i in range(300)])
                             for s in range(40)])
    d, _ = proven(ctx, ss)
    for blocks in ("auto", "1"):
        ctx.set_option("group_direct_blocks", blocks)
        try:
            for agg, dsa in ((0, 3), (1, 0), (2, 2), (3, 1)):
                g, p = run(ctx, d, agg, dsa)
                assert_same(g, ref(ss, agg, dsa))
                taken(p, f"W 4 agg {agg} ds {dsa} blocks {blocks}")
        finally:
            ctx.set_option("group_direct_blocks", "auto")


def test_option_off_proves_again(ctx, load):
    _, d, _, _ = shape(ctx, 37, 513)
    ctx.set_option("quals_proven", "off")
    try:
        g, p = run(ctx, d, 0, 3)
    finally:
        ctx.set_option("quals_proven", "auto")
    assert_same(g, want(ctx, 37, 513, 0, 3))
    assert p & GD and not p & (QP | FALLBACKS)


# ---- 2. the qualifiers are not read ----

def ff_after_first_word(ss):
    """every qualifier byte after each row's first word (cells 0 and 1) 0xFF"""
    qb = ss.qual_bytes.copy()
    for r in range(ss.n_rows):
        qo, n = int(ss.row_qual_off[r]), int(ss.row_ncells[r])
        qb[qo + 4:qo + 2 * n] = 0xFF
    return packing.SpanSet(ss.span_row_start, ss.row_base, ss.row_ncells, ss.row_qual_off, ss.row_val_off,
                           ss.row_val_len, qb, ss.val_bytes)


CORRUPT = {
    "delta+1": lambda ss: corrupt_qual(ss, 20, 650, lambda q: q + 16),
    "float-flag": lambda ss: corrupt_qual(ss, 20, 650, lambda q: q | 0x8),
    "width-4": lambda ss: corrupt_qual(ss, 20, 650, lambda q: (q & ~0x7) | 0x3),
    "0xFF": ff_after_first_word,
}


@pytest.mark.parametrize("what", list(CORRUPT))
def test_false_promise_shows_the_load_is_gone(ctx, load, what):
    clean = synth.regular(41, 1300, I64, seed=8, step=2)
    bad = CORRUPT[what](clean)
    assert not core.quals_proven(bad).all()
    d, _ = upload(ctx, bad)
    for agg, dsa in ((0, 3), (2, 0)):
        d.flags |= DQP  # by hand: the promise is false
        g, p = run(ctx, d, agg, dsa)
        assert_same(g, ref(clean, agg, dsa))
        taken(p, f"{what} flagged")
        # the same bytes with "quals_proven" "off", then without the flag: proven as they stream, today's fallback
        ctx.set_option("quals_proven", "off")
        try:
            g_off, p_off = run(ctx, d, agg, dsa)
        finally:
            ctx.set_option("quals_proven", "auto")
        d.flags &= ~DQP
        g_no, p_no = run(ctx, d, agg, dsa)
        # (0xFF: 1298 cells of one timestamp a row, which the general path refuses as unsorted where the oracle
        # emits them — the rerun's own business, in code the flag does not reach: the two runs agree with each other)
        o = ref(bad, agg, dsa) if what != "0xFF" else None
        for g2, p2, how in ((g_off, p_off, "off"), (g_no, p_no, "unflagged")):
            if o is not None:
                assert_same(g2, o)
            fell_back(p2, f"{what} {how}")
            assert not p2 & QP
        assert g_off[0] == g_no[0] and g_off[4:] == g_no[4:]
        for x, y in zip(g_off[1:4], g_no[1:4]):
            np.testing.assert_array_equal(x, y)
    # ... and the certificate is refused
    assert core.desc_certify(ctx, d)[1] == int((~core.quals_proven(bad)).sum()) and not d.flags & DQP


# ---- 3. still falling back under the flag ----

def test_fell_back_two_classes(ctx, load):
    spans = regular_spans(25, 1200)
    spans[13] = rows8(range(T0, T0 + 2400, 2), range(1200))
    ss = packing.pack_spans(spans)
    d, _ = proven(ctx, ss)
    for agg in (0, 1):
        g, p = run(ctx, d, agg, 3)
        assert_same(g, ref(ss, agg, 3))
        fell_back(p)
        assert p & QP  # (the launch that fell back ran without the stream)


def test_fell_back_seek(ctx, load):
    ss = synth.regular(50, 1800, I64, seed=6, step=2)
    d, _ = proven(ctx, ss)
    g, p = run(ctx, d, 0, 3, start=T0 + 10)
    assert_same(g, ref(ss, 0, 3, start=T0 + 10))
    fell_back(p)


def test_fell_back_more_than_64_buckets(ctx, load):
    ss = synth.regular(30, 1300, I64, seed=6, step=2)
    d, _ = proven(ctx, ss)
    g, p = run(ctx, d, 0, 3, interval=30)  # 87 buckets
    assert_same(g, ref(ss, 0, 3, interval=30))
    fell_back(p)


def test_rows_differ_from_spans(ctx):
    """not eligible: the present path, none of the direct group's bits"""
    ss = packing.pack_spans([rows8(range(T0 + 3000, T0 + 4200), range(s, s + 1200)) for s in range(40)])
    assert ss.n_rows == 2 * ss.n_spans
    d, _ = proven(ctx, ss)
    g, p = run(ctx, d, 0, 3)
    assert_same(g, ref(ss, 0, 3))
    assert not p & (GD | GDF | QP)


# ---- 4. a host descriptor's flag is ignored ----

def test_host_descriptor_flag_ignored(ctx):
    clean = synth.regular(41, 1300, I64, seed=8, step=2)
    for ss in (clean, CORRUPT["delta+1"](clean)):
        h = _abi.SgDesc()
        ss.fill_desc(h)
        h.flags = DQP
        g, p = run(ctx, h, 0, 3)
        assert_same(g, ref(ss, 0, 3))  # (the bytes as they are)
        assert not p & QP and p & (GD | GDF)
        assert bool(p & GDF) == (ss is not clean)


# ---- 5. ranks that differ ----

@pytest.fixture(scope="module")
def mctx3():
    from opentsdb_amd._lib import Context
    c = Context(devices=[0] * 3)
    assert c.ranks == 3
    c.set_option("group_direct", "always")
    yield c
    c.close()


@pytest.mark.parametrize("mode", ["rank0", "auto", "off"])
def test_three_ranks(ctx, mctx3, mode):
    """three in-process ranks over one flagged descriptor; "rank0": rank 0 runs
    without the qualifier stream and the other two prove theirs, the partials
    meeting in the call's one collective"""
    _, d, _, _ = shape(ctx, 37, 1300)
    mctx3.set_option("quals_proven", mode)
    try:
        for agg, dsa in ((0, 3), (1, 0), (2, 1), (3, 2)):
            g, p = run(mctx3, d, agg, dsa)
            assert_same(g, want(ctx, 37, 1300, agg, dsa))
            assert p & GD and p & AG and not p & FALLBACKS, f"{mode}: paths {p:#x}"
            assert bool(p & QP) == (mode != "off")  # (rank 0's paths)
            assert mctx3.timing().n_collectives == 1
    finally:
        mctx3.set_option("quals_proven", "auto")
