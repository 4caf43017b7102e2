"""Every kernel path on descriptor layouts other than the packer's
(tests/layouts.py): the groups and the comparison rules of
test_value_domains.py (integers, timestamps, codes and err_index bit-exact;
doubles bit-exact under TSDBHIP_EXACT_ORDER, else its 1e-9 rules), the
expected values from the oracle on the packed group (test_layouts_cpu.py: the
oracle is layout-blind), and the tsdbhip_timing.paths word asserted on every
call against what the kernels' membership predicates say of the layout.

The predicates (opentsdb_amd/csrc), restated in layouts.py:

  proposable  ug_probe      k_assemble.hip:253   (qo & 1) == 0 && (vo & (W-1)) == 0, first row of a span
              ls_probe      k_direct.hip:68      the same
  streamable  reg_rows_ok   k_ds_reg.hip:293-294 (qo & 7) == 0 && (vo & 15) == 0, every row
              ds_reg_body   k_ds_reg.hip:404     (qo & 7) == 0, first row
              dir_fields    k_ds_reg.hip:570     (qo & 7) == 0 && (vo & 15) == 0
              k_ds_spans    k_ds_chunks.hip:543  the same (one row), :551-552 (several)
  (k_decode_fast.hip:68-69 and k_direct_scan, k_direct.hip:300, take (qo & 7) == 0 && (vo & (W-1)) == 0 and
  hand other rows to the general code inside the same call: no bit of the paths word tells them apart)

None of them looks at the order of the rows or at the bytes between them.

  layout                      proposable          streamable
  packed poison shuffled      yes                 yes
    reversed
  v8                          W 8 and W 4         no
  v4 v12                      W 4 only            no
  q2 q4 q6                    yes                 no
  one_off_v one_off_q         yes                 no (the one row)
  vodd mixed compact          no (compact: the    no
                              one-row groups here
                              have rows at 2 mod 4)

  path (options)                      layout       bits set            bits clear
  1 decode != auto, or exact          all          -                   UNI LS GD REDONE(*)
    (rows3, three rows a span: these calls only; k_ds_spans' and k_decode_fast's several-row branches)
  1 auto, no downsampling             proposable   UNI iff packed's    LS GD REDONE UFB
                                      else         -                   UNI LS GD REDONE UFB
  1 auto, downsampling                streamable   UNI iff packed's    LS GD REDONE UFB
                                      proposable   UFB iff packed's    UNI LS GD DR GDF
                                                   UNI (k_ug_ds_reg declines at :293 / :404: api.hip, kSgEdges' RC_UG_FALLBACK edges)
                                      else         -                   UNI UFB LS GD REDONE
  2 lockstep=always, not dev          proposable   UNI LS              REDONE
    integer dev without rate          proposable   UNI                 LS REDONE
    float dev without rate            all          -                   UNI LS REDONE
    any                               else         -                   UNI LS REDONE (ls_probe declines too)
  3 aligned group                     streamable   AG, UNI iff !exact  AR GD REDONE
                                      proposable   AR, UFB iff !exact  AG UNI GD GDF DR
                                      else         AR                  AG UNI UFB GD GDF DR
    (AR: the general k_ds_reg's members fail reg_rows_ok, the group is broken, api.hip: SgCall::plan_reduce's fap_use)
  4 group_direct=always               streamable   GD AG UNI, GDL iff  GDF UFB AR
                                                   lines_nt
                                      proposable   GDF UFB AR, GDL     GD AG UNI DR
                                      else         GDF AR, GDL         GD AG UNI UFB DR
  5 batch                             all          -                   every bit (paths == 0)
  6 ranks: no downsampling as 2 (dev: the span-ordered pass, no bit); integers in 60-s buckets:
                                      streamable   UNI AG              AR GD REDONE
                                      else         UFB AR              AG UNI GD GDF DR
    (every rank of a sharded call makes the uniform attempt, api.hip: SgCall::uniform_try, so a group that does not stand falls back)
    exact                             all          -                   UNI LS GD AG AR REDONE
    (no aligned group on a sharded exact call, api.hip: SgCall::plan)
  7 device descriptors                as the host descriptor's row above
  8 the chain (compact_rows' layout)  as `compact`

(*) REDONE = UFB | DR (PATH_DIRECT_REDO) | GDF, as in test_value_domains.py."""
import ctypes as C

import numpy as np
import pytest

import layouts
import oracle
import time_domains as td
import value_domains as vd
from helpers import U32MAX, assert_same, run_both, with_option
from layouts import NAMES, relayout
from opentsdb_amd import _abi, compaction, core, packing, synth
from test_find_spans import W3, Scan, key, to_device
from test_group_direct_lines import run_of
from test_value_domains import compare, rank_starts, ref, uniform_expected

pytestmark = pytest.mark.gpu

AGGS = [0, 1, 2, 3, 4]
SUM, MIN, MAX, AVG, DEV = AGGS
UNI, LS, AG, AR = _abi.PATH_UNIFORM, _abi.PATH_LOCKSTEP, _abi.PATH_ALIGNED_GROUP, _abi.PATH_ALIGNED_RERUN
GD, GDF, GDL = _abi.PATH_GROUP_DIRECT, _abi.PATH_GROUP_DIRECT_FALLBACK, _abi.PATH_GROUP_DIRECT_LINES
UFB, DR = _abi.PATH_UNIFORM_FALLBACK, _abi.PATH_DIRECT_REDO
REDONE = UFB | DR | GDF
F4, F8 = vd.F4, vd.F8
SEED = 3


class Laid:
    """a group of value_domains / time_domains on a layout: the group's own
    fields (its key names the packed group: the oracle's results are shared by
    every layout) and the relayout's SpanSet with what the predicates say of it"""

    def __init__(self, g, name, odd_row=None):
        self.g, self.name = g, name
        self.ss = relayout(g.ss, name, seed=SEED, odd_row=odd_row)
        self.stream = layouts.rows_streamable(self.ss)
        self.prop = layouts.rows_proposable(self.ss)


_LAID = {}


def laid(g, name, odd_row=None):
    k = (g.key, name, odd_row)
    if k not in _LAID:
        _LAID[k] = Laid(g, name, odd_row)
    return _LAID[k]


def check(c, lg, agg, rate=False, interval=0, ds_agg=0, exact=False, desc=None):
    """one query on the GPU against the oracle on the packed group; returns
    the call's paths word"""
    g = lg.g
    o = ref(g, agg, rate, interval, ds_agg)
    if desc is None:
        res = core.run_spanset(c, lg.ss, 0, U32MAX, agg, rate, interval, ds_agg, exact=exact)
    else:
        res = core.run_spanset(c, None, 0, U32MAX, agg, rate, interval, ds_agg, exact=exact, device_desc=desc,
                               capacity=max(1, lg.ss.n_cells()))
    assert res[0] not in (_abi.E_HIP, _abi.E_RCCL), c.last_error()
    p = c.timing().paths
    try:
        compare(g, res, o, agg, rate, interval, ds_agg, exact)
    except AssertionError as e:
        raise AssertionError(f"{lg.name} {g.pool} {g.shape} agg={agg} rate={rate} ds=({interval},{ds_agg}) "
                             f"exact={exact} paths={p:#x}: {e}") from None
    return p


def expect(p, on, off, what):
    assert p & on == on and not p & off, f"{what}: paths {p:#x}, wanted {on:#x} set and {off:#x} clear"


# ---- 1. the decode variants ----

@pytest.fixture(params=["auto", "general", "fast", "chunks", "spans", "direct"])
def decode(request):
    yield from with_option(request, "decode", request.param, "auto")


DECODE_GROUPS = {
    "one_row-WRAP64": lambda: vd.one_row("WRAP64", 2),               # W 8 integer
    "one_row-INT32_EDGE": lambda: vd.one_row("INT32_EDGE", 2),       # W 4 integer
    "one_row-NAN_LATER-f4": lambda: vd.one_row("NAN_LATER", 2, kind=F4),
    "one_row-ZEROS-f8": lambda: vd.one_row("ZEROS", 2, kind=F8),
    "jittered-WIDTHS": lambda: vd.jittered("WIDTHS"),
    "jittered-NAN_LATER": lambda: vd.jittered("NAN_LATER"),          # float32 / float64 spans by turns
    "jittered-BIG_MIXED": lambda: vd.jittered("BIG_MIXED"),          # longs of every width next to a float64 span
}


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("group", sorted(DECODE_GROUPS))
def test_decode_variants(ctx, decode, group, name):
    """no downsampling under every aggregator; 60-s and 13-s buckets under
    every downsampler; both EXACT_ORDER settings (test_value_domains.py's
    queries)"""
    lg = laid(DECODE_GROUPS[group](), name)
    g = lg.g
    qs = [(agg, 0, 0) for agg in AGGS]
    qs += [((dsa + (1 if interval == 60 else 3)) % 5, interval, dsa) for interval in (60, 13) for dsa in AGGS]
    for agg, interval, dsa in qs:
        for exact in (False, True):
            p = check(ctx, lg, agg, False, interval, dsa, exact)
            q = (name, group, agg, interval, dsa, exact)
            ue = uniform_expected(g, agg, interval, dsa)
            if decode != "auto" or exact or not ue or not lg.prop:
                expect(p, 0, UNI | LS | GD | REDONE, q)
            elif not interval or lg.stream:
                expect(p, UNI, LS | GD | REDONE, q)
            else:
                expect(p, UFB, UNI | LS | GD | DR | GDF, q)


@pytest.mark.parametrize("name", NAMES)
def test_decode_variants_top_rows(ctx, decode, name):
    """three hourly rows a span (360, 360 and 170 cells), 20 spans: the
    several-row branches of the forced variants and of EXACT_ORDER"""
    lg = laid(td.top_rows(S=20), name)
    for agg, interval, dsa in ((SUM, 0, 0), (MAX, 0, 0), (DEV, 0, 0), (AVG, 60, SUM), (MIN, 60, MAX), (SUM, 13, AVG),
                               (MAX, 13, DEV)):
        for exact in (False, True):
            if decode == "auto" and not exact:
                continue
            p = check(ctx, lg, agg, False, interval, dsa, exact)
            expect(p, 0, UNI | LS | GD | REDONE, (name, agg, interval, dsa, exact))


# ---- 2. lockstep and uniform (lockstep=always) ----

@pytest.fixture
def lockstep_always(request):
    yield from with_option(request, "lockstep", "always", "on")


# (603 and 597 cells: the row's last 16-B qualifier group holds 6 and 10 bytes that are not the row's)
LOCKSTEP_GROUPS = [("WRAP64", None, 600), ("INT32_EDGE", None, 600), ("NAN_LATER", F4, 600), ("NAN_LATER", F8, 600),
                   ("ZEROS", F4, 600), ("ZEROS", F8, 600), ("WRAP64", None, 603), ("INT32_EDGE", None, 597)]


def lockstep_case(c, pool, kind, name, n=600, desc_of=None):
    for agg in AGGS:
        for rate in (False, True):
            int_dev = agg == DEV and not rate and kind is None
            lg = laid(vd.one_row(pool, 2, S=100 if int_dev else 70, n=n, kind=kind), name)
            p = check(c, lg, agg, rate, desc=desc_of(lg) if desc_of else None)
            q = (name, pool, kind, agg, rate)
            if not lg.prop or (agg == DEV and not rate and not int_dev):
                expect(p, 0, UNI | LS | GD | REDONE, q)
            elif int_dev:
                expect(p, UNI, LS | REDONE, q)
                assert ref(lg.g, agg).is_int.all()  # (so the comparison above was bit for bit)
            else:
                expect(p, UNI | LS, REDONE, q)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("pool,kind,n", LOCKSTEP_GROUPS, ids=[f"{p}{k or ''}-{n}" for p, k, n in LOCKSTEP_GROUPS])
def test_lockstep_uniform(ctx, lockstep_always, pool, kind, n, name):
    """k_lockstep with and without rate under every aggregator, k_ug_dev for
    integer dev without rate (100 spans: its phases). v8 at W 8, v4 / v12 at
    W 4 and q2 / q4 / q6 are the rows ug_probe admits off the packer's
    alignment: raw_buffer_load_b128 from a base at 8 or 4 mod 16 (values) and
    at 2, 4 or 6 mod 8 (qualifiers)"""
    lockstep_case(ctx, pool, kind, name, n)


# ---- 3. the aligned group ----

INT_GROUPS = ["WRAP64", "NEG", "INT32_EDGE"]


def aligned_expect(p, lg, exact, q):
    if lg.stream:
        expect(p, AG | (0 if exact else UNI), AR | GD | REDONE | (UNI if exact else 0), q)
    elif lg.prop and not exact:
        expect(p, AR | UFB, AG | UNI | GD | GDF | DR, q)
    else:
        expect(p, AR, AG | UNI | UFB | GD | GDF | DR, q)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("pool", INT_GROUPS)
@pytest.mark.parametrize("step", [1, 2])
@pytest.mark.parametrize("exact", [False, True], ids=["", "exact"])
def test_aligned_group(ctx, pool, step, exact, name):
    """60-s buckets over 600 cells: k_ug_ds_reg (the uniform form) and, under
    EXACT_ORDER or after its fall-back, the general k_ds_reg; a layout that is
    not streamable leaves both and the members' E is written by the rerun"""
    lg = laid(vd.one_row(pool, step), name)
    for agg in (SUM, MIN, MAX, AVG):
        for dsa in (SUM, MIN, MAX, AVG):
            aligned_expect(check(ctx, lg, agg, False, 60, dsa, exact), lg, exact, (name, pool, step, agg, dsa))


# ---- 4. the direct aligned group ----

@pytest.fixture
def group_direct_always(request):
    yield from with_option(request, "group_direct", "always", "on")


@pytest.fixture(params=["rows", "lines_nt"])
def load(request, ctx, group_direct_always):
    ctx.set_option("group_direct_load", request.param)
    yield request.param
    ctx.set_option("group_direct_load", "auto")


@pytest.fixture(params=[1, 4], ids=lambda r: f"run{r}")
def run(request, ctx, load):
    ctx.set_option("group_direct_run", str(request.param))
    yield request.param
    ctx.set_option("group_direct_run", "auto")


@pytest.fixture
def clean(ctx, capfd, run):
    """test_group_direct_lines.py's: "check_clean" compares the call state
    with its initial values at the start of every call; a taken call and a
    small one after the test's last check that one's state too"""
    ctx.set_option("check_clean", "on")
    try:
        yield
        g, o = run_both(ctx, synth.regular(9, 700, _abi.SYN_INT64_COUNTER, seed=2, step=1), 0, U32MAX, 0, False, 60, 3)
        assert_same(g, o)
        p = ctx.timing().paths
        assert p & GD and not p & GDF
        g, o = run_both(ctx, synth.regular(3, 16, _abi.SYN_INT64_COUNTER, seed=2, step=1), 0, U32MAX, 0, False, 60, 3)
        assert_same(g, o)
    finally:
        ctx.set_option("check_clean", "off")
    assert "TSDBHIP_CHECK_CLEAN" not in capfd.readouterr().err


def direct_expect(p, lg, load, q):
    lines = GDL if load.startswith("lines") else 0
    if lg.stream:
        expect(p, GD | AG | UNI | lines, GDF | UFB | AR | DR | (GDL ^ lines), q)
    elif lg.prop:
        expect(p, GDF | UFB | AR | lines, GD | AG | UNI | DR | (GDL ^ lines), q)
    else:
        expect(p, GDF | AR | lines, GD | AG | UNI | UFB | DR | (GDL ^ lines), q)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("pool", ["WRAP64", "INT32_EDGE"])
def test_group_direct(ctx, load, run, pool, name):
    """8 run + 3 spans (full and short runs): taken on every streamable
    layout whatever the rows' order and the bytes between them, fallen back on
    every other one"""
    lg = laid(vd.one_row(pool, 2, S=8 * run + 3), name)
    for agg in (SUM, MIN, MAX, AVG):
        for dsa in (SUM, MIN, MAX, AVG):
            direct_expect(check(ctx, lg, agg, False, 60, dsa), lg, load, (name, pool, run, load, agg, dsa))


@pytest.mark.parametrize("name", ["one_off_v", "one_off_q"])
@pytest.mark.parametrize("pool", ["WRAP64", "INT32_EDGE"])
def test_group_direct_odd_row_inside_a_run(ctx, load, run, clean, pool, name):
    """the one row off the alignment is a middle span of a wave's run (as
    test_fell_back_inside_a_run places its qualifier): only the streaming wave
    meets it, while its predecessor streams (reg_run's tick, k_ds_reg.hip:662)"""
    n = 10 * run + 2
    r = run_of(n, run, 3)
    span = r[len(r) // 2]
    lg = laid(vd.one_row(pool, 2, S=n), name, odd_row=span)
    assert not lg.stream and lg.prop
    assert int(lg.ss.row_val_off[span]) % 16 == (8 if name == "one_off_v" else 0)
    assert int(lg.ss.row_qual_off[span]) % 8 == (2 if name == "one_off_q" else 0)
    for agg, dsa in ((SUM, AVG), (MAX, MIN), (MIN, SUM)):
        direct_expect(check(ctx, lg, agg, False, 60, dsa), lg, load, (name, pool, run, load, agg, dsa))


# ---- 5. the batch ----

BATCH_CUT = [0, 9, 10, 35, 52, 70]  # five groups, [9, 10) of one span; row 34 ends the third
BATCH_LAYOUTS = ["poison", "shuffled", "reversed", "v8", "v4", "vodd", "q2", "q6", "compact", "mixed", "one_off_v",
                 "one_off_q"]
_SHARD_REF = {}


def shard_ref(g, lo, hi, q):
    k = (g.key, lo, hi) + q
    if k not in _SHARD_REF:
        _SHARD_REF[k] = oracle.spangroup(g.ss.shard(lo, hi), 0, U32MAX, *q)
    return _SHARD_REF[k]


def batch_case(c, g, ss, gss, exact, device_desc=None, span_of=None, what=""):
    """every group of the batch against the oracle on the packed group's
    spans alone (span_of: the packed group's span behind each span of ss)"""
    caps = None
    if device_desc is not None:
        caps = [max(1, 600 * (gss[k + 1] - gss[k])) for k in range(len(gss) - 1)]
    for agg in AGGS:
        for rate, interval, dsa in ((False, 0, 0), (True, 0, 0), (False, 60, AVG), (False, 13, MIN)):
            rc, res = core.run_spanset_batch(c, ss, gss, 0, U32MAX, agg, rate, interval, dsa, exact=exact,
                                             capacities=caps, device_desc=device_desc)
            assert rc not in (_abi.E_HIP, _abi.E_RCCL), c.last_error()
            p = c.timing().paths
            assert p == 0, hex(p)
            first = 0
            for k in range(len(gss) - 1):
                if span_of is None:
                    o = shard_ref(g, gss[k], gss[k + 1], (agg, rate, interval, dsa))
                else:
                    o = oracle.spangroup(span_of(gss[k], gss[k + 1]), 0, U32MAX, agg, rate, interval, dsa)
                try:
                    assert_same(res[k], o, exact_double=exact)
                    assert res[k][5] == o.err_index or not o.code
                except AssertionError as e:
                    raise AssertionError(f"{what} group {k} agg={agg} rate={rate} ds=({interval},{dsa}): {e}") from None
                first = first or o.code
            assert rc == first


@pytest.mark.parametrize("name", BATCH_LAYOUTS)
@pytest.mark.parametrize("pool,kind", [("WRAP64", None), ("INT32_EDGE", None), ("NAN_LATER", F8)],
                         ids=["WRAP64", "INT32_EDGE", "NAN_LATER"])
@pytest.mark.parametrize("exact", [False, True], ids=["", "exact"])
def test_batch(ctx, pool, kind, exact, name):
    """five uneven groups cut from one relayout's buffers, one of a single
    span; one_off_*: the odd row is row 34, the last of the third group"""
    g = vd.one_row(pool, 2, kind=kind)
    lg = laid(g, name, odd_row=34 if name.startswith("one_off") else None)
    if name.startswith("one_off"):
        off = lg.ss.row_val_off if name == "one_off_v" else lg.ss.row_qual_off
        bad = np.nonzero(off.astype(np.int64) % (16 if name == "one_off_v" else 8))[0]
        assert bad.tolist() == [34] and BATCH_CUT[3] == 35
    batch_case(ctx, g, lg.ss, BATCH_CUT, exact, what=name)


# ---- 6. two and three ranks on one GPU ----

@pytest.fixture(scope="module", params=[2, 3], ids=["ranks2", "ranks3"])
def mctx(request):
    from opentsdb_amd._lib import Context
    c = Context(devices=[0] * request.param)
    c.n_ranks = request.param
    yield c
    c.close()


@pytest.mark.timeout(120)
@pytest.mark.parametrize("name", ["shuffled", "reversed", "mixed", "compact"])
@pytest.mark.parametrize("pool,kind", [("WRAP64", None), ("INT32_EDGE", None), ("NAN_LATER", F8), ("ZEROS", F4)],
                         ids=["WRAP64", "INT32_EDGE", "NAN_LATER", "ZEROS"])
def test_ranks(mctx, pool, kind, name):
    """plan_shards (api.hip) on offsets that are not monotone and not the
    packer's: a shard's byte range is the min and max of its rows' (the whole
    buffer, nearly, on `shuffled`), its start rounded down to 16 B, which
    keeps every residue"""
    g = vd.one_row(pool, 2, kind=kind)
    lg = laid(g, name)
    starts = rank_starts(g, mctx.n_ranks)
    assert len(set(starts)) == mctx.n_ranks + 1  # (no empty rank)
    if name == "shuffled":  # a rank's rows are not one contiguous piece of the buffer
        r0, r1 = starts[0], starts[1]
        vo = lg.ss.row_val_off.astype(np.int64)
        assert ((vo[r1:] > vo[r0:r1].min()) & (vo[r1:] < vo[r0:r1].max())).any()
    flt = kind is not None
    for agg in (SUM, MAX, AVG, DEV):
        for exact in (False, True):
            p = check(mctx, lg, agg, exact=exact)
            q = (name, pool, agg, exact)
            if exact or not lg.prop or agg == DEV:  # (sharded: no k_ug_dev; the span-ordered pass)
                expect(p, 0, UNI | LS | GD | AG | AR | REDONE, q)
            else:
                expect(p, UNI | LS, GD | REDONE, q)
            if agg == DEV or (flt and not exact):
                continue
            # (sharded, not exact: every rank makes the uniform attempt, api.hip: SgCall::uniform_try, and a group that
            # does not stand on every rank falls back; exact: no attempt and no aligned group, api.hip: SgCall::plan)
            p = check(mctx, lg, agg, False, 60, AVG, exact)
            if exact:
                expect(p, 0, UNI | LS | GD | AG | AR | REDONE, q)
            elif lg.stream:
                expect(p, UNI | AG, AR | GD | REDONE, q)
            else:
                expect(p, UFB | AR, AG | UNI | GD | GDF | DR, q)


# ---- 7. device descriptors ----

DESC_FIELDS = (("span_row_start", _abi.P64), ("row_base", _abi.P32), ("row_ncells", _abi.P32),
               ("row_qual_off", _abi.P64), ("row_val_off", _abi.P64), ("row_val_len", _abi.P32))
_DEV = {}


def device_desc(ctx, lg):
    """the relayout's arrays uploaded: qual_nbytes / val_nbytes end exactly
    where the last row ends, the allocations go on for 64 poisoned bytes more
    (never a buffer that truly ends at the last row: nothing here may fault)"""
    k = (lg.g.key, lg.name)
    if k not in _DEV:
        ss = lg.ss
        qn, vn = layouts.extents(ss)
        assert len(ss.qual_bytes) >= qn + 64 and len(ss.val_bytes) >= vn + 64
        assert (ss.qual_bytes[qn:] == 0xFF).all() and (ss.val_bytes[vn:] == 0xFF).all()
        t = {f: to_device(ctx, getattr(ss, f)) for f, _ in DESC_FIELDS}
        t["qual_bytes"], t["val_bytes"] = to_device(ctx, ss.qual_bytes), to_device(ctx, ss.val_bytes)
        d = _abi.SgDesc()
        d.flags = _abi.DESC_DEVICE
        d.n_spans, d.n_rows = ss.n_spans, ss.n_rows
        for f, pt in DESC_FIELDS:
            setattr(d, f, C.cast(C.c_void_p(t[f].data_ptr()), pt))
        d.qual_bytes, d.qual_nbytes = C.cast(C.c_void_p(t["qual_bytes"].data_ptr()), _abi.P8), qn
        d.val_bytes, d.val_nbytes = C.cast(C.c_void_p(t["val_bytes"].data_ptr()), _abi.P8), vn
        _DEV[k] = (d, t)
    return _DEV[k][0]


DEVICE_LAYOUTS = ["poison", "shuffled", "v8", "compact"]


@pytest.mark.parametrize("name", DEVICE_LAYOUTS)
@pytest.mark.parametrize("pool,kind", [("WRAP64", None), ("INT32_EDGE", None), ("NAN_LATER", F8)],
                         ids=["WRAP64", "INT32_EDGE", "NAN_LATER"])
def test_device_lockstep_uniform(ctx, lockstep_always, pool, kind, name):
    lockstep_case(ctx, pool, kind, name, desc_of=lambda lg: device_desc(ctx, lg))


@pytest.mark.parametrize("name", DEVICE_LAYOUTS)
@pytest.mark.parametrize("pool", ["WRAP64", "INT32_EDGE"])
@pytest.mark.parametrize("exact", [False, True], ids=["", "exact"])
def test_device_aligned_group(ctx, pool, exact, name):
    lg = laid(vd.one_row(pool, 2), name)
    d = device_desc(ctx, lg)
    for agg, dsa in ((SUM, SUM), (MIN, MAX), (MAX, AVG), (AVG, MIN)):
        aligned_expect(check(ctx, lg, agg, False, 60, dsa, exact, desc=d), lg, exact, (name, pool, agg, dsa))


@pytest.mark.parametrize("name", DEVICE_LAYOUTS)
@pytest.mark.parametrize("pool", ["WRAP64", "INT32_EDGE"])
def test_device_group_direct(ctx, load, run, pool, name):
    lg = laid(vd.one_row(pool, 2, S=8 * run + 3), name)
    d = device_desc(ctx, lg)
    for agg, dsa in ((SUM, SUM), (MIN, MAX), (MAX, AVG), (AVG, MIN)):
        direct_expect(check(ctx, lg, agg, False, 60, dsa, desc=d), lg, load, (name, pool, run, load, agg, dsa))


@pytest.mark.parametrize("name", ["v8", "compact"])
@pytest.mark.parametrize("pool,kind", [("WRAP64", None), ("NAN_LATER", F8)], ids=["WRAP64", "NAN_LATER"])
def test_device_gather_batch(ctx, pool, kind, name):
    """tsdbhip_desc_gather with a permuted order on top of the layout, then
    the batch over the gathered descriptor: the spans' offsets neither grow
    with the row index nor sit at the packer's residues"""
    g = vd.one_row(pool, 2, kind=kind)
    lg = laid(g, name)
    d = device_desc(ctx, lg)
    order = np.random.default_rng(8).permutation(g.n_spans).astype(np.uint32)
    out = _abi.SgDesc()
    ctx.check(ctx._lib.tsdbhip_desc_gather(ctx.handle, C.byref(d), _abi.ptr(order, C.c_uint32), len(order),
                                           C.byref(out)))
    try:
        assert out.n_spans == g.n_spans and out.n_rows == g.ss.n_rows and out.flags & _abi.DESC_DEVICE
        spans_of = lambda lo, hi: packing.pack_spans([g.spans[int(s)] for s in order[lo:hi]])  # noqa: E731
        batch_case(ctx, g, None, BATCH_CUT, False, device_desc=out, span_of=spans_of, what=name)
    finally:
        ctx._lib.tsdbhip_desc_gather_free(ctx.handle, C.byref(out))


# ---- 8. the real chain at kernel-path size ----

def test_chain_at_kernel_path_size(ctx, lockstep_always, group_direct_always):
    """compact_rows -> find_spans -> spangroup_run on the C3* class: 70 spans
    of one hourly row of 600 eight-byte cells, each written as 600 single
    cells. tsdbhip_rows_out places row r's value at 4800 r + r: every residue
    mod 16, so no span is proposable and the streaming paths must all decline
    (the direct aligned group by falling back)"""
    S, n = 70, 600
    g = vd.one_row("WRAP64", 2, S=S, n=n)
    tags = [[(1, s % 5), (2, s)] for s in range(S)]
    order = sorted(range(S), key=lambda s: core.span_cmp_key(key(synth.T0, tags[s])))
    base = g.spans[0][0].base_time
    raw, keys = [], []
    for i, s in enumerate(order):  # (span i of the group is the i-th series in SpanCmp order)
        (kv,) = g.spans[i]
        assert kv.base_time == base and len(kv.value) == 8 * n + 1
        raw.append([(kv.qualifier[2 * c:2 * c + 2], kv.value[8 * c:8 * c + 8]) for c in range(n)])
        keys.append(key(base, tags[s]))
    res = compaction.compact_rows(ctx, compaction.pack_rows(raw))
    assert (res.status == _abi.ROW_TRIVIAL).all()
    np.testing.assert_array_equal(res.val_off, 4801 * np.arange(S, dtype=np.uint64))
    np.testing.assert_array_equal(res.qual_off, 1200 * np.arange(S, dtype=np.uint64))
    scan = Scan([(k, 0) for k in keys], W3, res.status, cells=False)
    scan.cells = (res.qual_off, res.qual_len, res.val_off, res.val_len)
    rc, fs = scan.run(ctx)
    assert rc == 0, ctx.last_error()
    assert (fs.n_spans, fs.n_rows, fs.n_skipped) == (S, S, 0)
    ss = packing.SpanSet(fs.span_row_start, fs.row_base, fs.row_ncells, fs.row_qual_off, fs.row_val_off,
                         fs.row_val_len, res.qual, res.val)
    for s in range(S):
        assert ss.span_rows(s) == g.ss.span_rows(s)
    assert not layouts.rows_proposable(ss) and not layouts.rows_streamable(ss)
    lg = Laid.__new__(Laid)
    lg.g, lg.name, lg.ss, lg.stream, lg.prop = g, "chain", ss, False, False
    for agg in (SUM, MAX):
        expect(check(ctx, lg, agg), 0, UNI | LS | GD | AG | AR | REDONE, ("chain", agg))
    ctx.set_option("group_direct_load", "rows")
    try:
        p = check(ctx, lg, AVG, False, 60, AVG)
    finally:
        ctx.set_option("group_direct_load", "auto")
    expect(p, GDF | AR, GD | GDL | AG | UNI | UFB | DR, "chain avg 60")
