"""The value domains of tests/value_domains.py on the CPU: the oracle against
the closed form on every pool and both shapes, bit for bit, and the conditions
that keep the GPU tests of test_value_domains.py from passing on nothing (a
pool that never wraps, never truncates, never meets a NaN where it matters),
asserted on the oracle alone."""
import struct

import numpy as np
import pytest

import closed_form
import oracle
import value_domains as vd
from helpers import U32MAX
from opentsdb_amd import _abi

AGGS = [0, 1, 2, 3, 4]
SUM, MIN, MAX, AVG, DEV = AGGS


def queries():
    for agg in AGGS:
        for rate in (False, True):
            for interval, ds_agg in ((0, 0), (10, agg), (60, (agg + 1) % 5)):
                yield agg, rate, interval, ds_agg


def dbits(v):
    return struct.unpack("<q", struct.pack("<d", v))[0]


def check_closed_form(g):
    for agg, rate, interval, ds_agg in queries():
        q = (g.pool, g.shape, agg, rate, interval, ds_agg)
        r = oracle.spangroup(g.ss, 0, U32MAX, agg, rate, interval, ds_agg)
        try:
            exp, err = closed_form.spangroup(g.spans, 0, U32MAX, agg, rate, interval, ds_agg), None
        except ArithmeticError as e:
            err, exp = e.args
        if err is None:
            assert r.code == 0, q
        else:
            assert r.code == _abi.E_NAN_INF and r.err_index == err, q
        assert [int(x) for x in r.ts] == [e[0] for e in exp], q
        for i, (t, isint, v) in enumerate(exp):
            assert bool(r.is_int[i]) == isint, (q, i)
            if isint:
                assert int(r.bits[i]) == v, (q, i)
            else:
                got = float(r.bits[i:i + 1].view(np.float64)[0])
                assert int(r.bits[i]) == dbits(v) or (got != got and v != v), (q, i, got, v)


# (the closed form is pure Python, cubic in the group: one_row at 7 spans of
# 130 cells — two 64-cell waves, two 60-cell buckets, and the 12 spans of
# `jittered` as they are)
@pytest.mark.parametrize("pool", vd.POOLS)
@pytest.mark.parametrize("step", [1, 2])
def test_oracle_matches_closed_form_one_row(pool, step):
    check_closed_form(vd.one_row(pool, step, S=7, n=130))


@pytest.mark.parametrize("pool", vd.POOLS)
def test_oracle_matches_closed_form_jittered(pool):
    check_closed_form(vd.jittered(pool))


@pytest.mark.parametrize("pool", ["WRAP64", "NEG", "INT32_EDGE", "WIDTHS", "ZEROS", "DENORM", "BIG_MIXED"])
@pytest.mark.parametrize("step", [1, 2])
def test_finite_pools_give_results(pool, step):
    g = vd.one_row(pool, step)
    for agg, rate, interval, ds_agg in queries():
        r = oracle.spangroup(g.ss, 0, U32MAX, agg, rate, interval, ds_agg)
        assert r.code == 0, (agg, rate, interval, ds_agg)
        # 600 cells (at least 100 points) without downsampling; a point a bucket with it (60 and 10
        # at 1 s, 20 and 5 at 2 s: 10-s and 60-s buckets cannot leave 100 points of 600 cells);
        # a rate has no point at a span's first
        kk = vd.cells_per_bucket(interval, step) if interval else 1
        assert len(r.ts) == (600 + kk - 1) // kk - (1 if rate else 0) and (interval or len(r.ts) >= 100)


def test_pools_hold_what_they_name():
    every = set()
    for _, pts in vd.one_row("NEG").series:
        every |= {v for _, v in pts}
    assert every == set(range(-1000, 0))
    for pool, minimal in (("INT32_EDGE", 3), ("WRAP64", 7), ("NEG", 7)):
        g = vd.one_row(pool, 2)
        assert g.one_class
        assert {kv.qualifier[1] & 0xF for rows in g.spans for kv in rows} == {minimal}
        assert any(v < 0 for _, pts in g.series for _, v in pts)
    widths = {kv.qualifier[i + 1] & 0x7 for rows in vd.jittered("WIDTHS").spans for kv in rows
              for i in range(0, len(kv.qualifier), 2)}
    assert widths == {0, 1, 3, 7}
    for kind, flag in ((vd.F4, 0xB), (vd.F8, 0xF)):
        for pool in vd.FLOAT_POOLS:
            g = vd.one_row(pool, 2, kind=kind)
            assert g.one_class and g.spans[0][0].qualifier[1] & 0xF == flag
    g = vd.one_row("BIG_MIXED")
    assert not g.one_class and [k for k, _ in g.series].count(vd.F8) == 1
    r = oracle.spangroup(g.ss, 0, U32MAX, SUM)
    assert not r.is_int.any()  # (every value converted to double)
    g = vd.jittered("BIG_MIXED")
    assert not oracle.spangroup(g.ss, 0, U32MAX, SUM).is_int.any()


@pytest.mark.parametrize("step", [1, 2])
def test_nan_later(step):
    for kind in (vd.F4, vd.F8):
        g = vd.one_row("NAN_LATER", step, kind=kind)
        n = g.meta["n"]
        for agg, rate, interval, ds_agg in queries():
            r = oracle.spangroup(g.ss, 0, U32MAX, agg, rate, interval, ds_agg)
            q = (agg, rate, interval, ds_agg)
            if agg in (MIN, MAX):
                assert r.code == 0, q
            else:
                grid = n if not interval else (n + vd.cells_per_bucket(interval, step) - 1) // vd.cells_per_bucket(
                    interval, step)
                if interval and ds_agg in (MIN, MAX):
                    # (sum, 60 s, min): the downsampler's own min drops a NaN that is not its bucket's
                    # first cell, and none of the later NaNs heads a bucket of 60 or 30 cells
                    assert all(c % vd.cells_per_bucket(interval, step) for c in g.meta["later"]), q
                    assert r.code == 0, q
                    continue
                assert r.code == _abi.E_NAN_INF, q
                assert r.err_index >= grid // 4, q


def designed_index(g, rate, interval):
    k = g.meta["k0"] // (vd.cells_per_bucket(interval, g.meta["step"]) if interval else 1)
    return k - 1 if rate else k


@pytest.mark.parametrize("step", [1, 2])
def test_nan_first(step):
    """the first span's NaN is the first cell of its bucket at 10 and 60 s, so
    every downsampler emits it and every aggregator starts from it"""
    for kind in (vd.F4, vd.F8):
        g = vd.one_row("NAN_FIRST", step, kind=kind)
        n = g.meta["n"]
        for agg, rate, interval, ds_agg in queries():
            r = oracle.spangroup(g.ss, 0, U32MAX, agg, rate, interval, ds_agg)
            q = (agg, rate, interval, ds_agg)
            k = designed_index(g, rate, interval)
            grid = n // (vd.cells_per_bucket(interval, step) if interval else 1)
            assert r.code == _abi.E_NAN_INF and r.err_index == k, q
            assert k >= grid // 2, q


@pytest.mark.parametrize("step", [1, 2])
def test_huge(step):
    """float64: the cross-span sum of same-signed 1.7e308 overflows in any
    order (sum, avg, and dev's squares). float32 cannot: 70 spans of 3.4e38
    widened to double stay finite, so that group returns results."""
    g = vd.one_row("HUGE", step, kind=vd.F8)
    for agg in (SUM, AVG, DEV):
        for rate in (False, True):
            r = oracle.spangroup(g.ss, 0, U32MAX, agg, rate)
            k = designed_index(g, rate, 0)
            assert r.code == _abi.E_NAN_INF and r.err_index == k and k >= g.meta["n"] // 2, (agg, rate)
    g = vd.one_row("HUGE", step, kind=vd.F4)
    for agg in AGGS:
        r = oracle.spangroup(g.ss, 0, U32MAX, agg)
        assert r.code == 0
        big = r.bits.view(np.float64) > 1e38
        assert big.sum() == (0 if agg == MIN else 1) and (agg == MIN or big[g.meta["k0"]])


def test_nan_bucket():
    for step in (1, 2):
        g = vd.one_row("NAN_BUCKET", step, kind=vd.F8)
        k0 = g.meta["k0"]
        for interval in (10, 60):
            kk = vd.cells_per_bucket(interval, step)
            assert k0 % kk == 0 and (k0 + 61) % kk != 0
            # the downsampler's min: the NaN that heads its bucket comes out, the later one does not
            r = oracle.spangroup(g.ss, 0, U32MAX, SUM, False, interval, MIN)
            assert r.code == _abi.E_NAN_INF and r.err_index == k0 // kk
            r = oracle.spangroup(g.ss, 0, U32MAX, MIN, False, interval, MIN)
            assert r.code == 0  # (neither is in the first span)
            r = oracle.spangroup(g.ss, 0, U32MAX, SUM, False, interval, SUM)
            assert r.code == _abi.E_NAN_INF and r.err_index == k0 // kk


@pytest.mark.parametrize("step", [1, 2])
def test_wrap64_wraps_truncates_and_saturates(step):
    g = vd.one_row("WRAP64", step)
    S, n = g.n_spans, g.meta["n"]
    rs, ra, rd = (oracle.spangroup(g.ss, 0, U32MAX, a) for a in (SUM, AVG, DEV))
    assert rs.code == ra.code == rd.code == 0 and rs.is_int.all() and ra.is_int.all() and rd.is_int.all()
    wrapped = truncated = 0
    for i in range(n):
        v = g.values(i)
        w = vd.wrap(sum(v))
        assert int(rs.bits[i]) == w
        wrapped += w != sum(v)
        if w < 0 and w % S:
            truncated += 1
            assert int(ra.bits[i]) == -((-w) // S) != w // S  # (Java's division truncates)
    assert wrapped and truncated
    # Long.MIN_VALUE / Long.MAX_VALUE by turns at cell 5: (long) of their deviation saturates
    assert set(g.values(5)) == {vd.INT64_MIN, vd.INT64_MAX}
    two = vd.one_row("WRAP64", step, S=2)
    r2 = oracle.spangroup(two.ss, 0, U32MAX, DEV)
    assert sorted(two.values(5)) == [vd.INT64_MIN, vd.INT64_MAX] and int(r2.bits[5]) == vd.INT64_MAX
    assert (rd.bits == vd.INT64_MAX).any()
    rmin, rmax = (oracle.spangroup(g.ss, 0, U32MAX, a) for a in (MIN, MAX))
    assert int(rmin.bits[5]) == vd.INT64_MIN and int(rmax.bits[5]) == vd.INT64_MAX


@pytest.mark.parametrize("kind", [vd.F4, vd.F8])
def test_zeros_keep_their_sign(kind):
    g = vd.one_row("ZEROS", 2, kind=kind)
    neg = dbits(-0.0)
    for agg in (MIN, MAX):
        r = oracle.spangroup(g.ss, 0, U32MAX, agg)
        assert r.code == 0 and set(r.bits.tolist()) == {0, neg}
        # the first span's zero stays: neither 0.0 < -0.0 nor -0.0 < 0.0
        first = [dbits(v) for _, v in g.series[0][1]]
        assert r.bits.tolist() == first
