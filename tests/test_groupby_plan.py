"""GROUP BY planning and SpanGroup tags on the GPU: tsdbhip_groupby_plan (the
grouping loop of TsdbQuery.groupByAndAggregate, TsdbQuery.java:294-363, and
SpanGroup.computeTags, SpanGroup.java:149-173) and tsdbhip_desc_gather.

Yardsticks: core.plan_groups (pinned by tests/test_groupby.py) for groups and
order, literal expectations, and for tags a brute force written here (set
intersection of the kept spans' (name, value) pairs; aggregated = the first
kept span's names minus the common names). Every comparison is on exact
bytes."""
import ctypes as C
import functools
import json
import os
import shutil
import subprocess
import threading

import numpy as np
import pytest

from helpers import I, T0, U32MAX, assert_same
from opentsdb_amd import _abi, core, packing
from time_domains import EDGE_BASES  # (base times 0, either side of 2^31, the last hourly row below 2^32)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W3 = (3, 3, 3)
# from the kernels' constants (opentsdb_amd/csrc/k_groupby.hip, k_util.hip): a
# sort tile is GB_TILE positions; the digit-major count matrix (256 x tiles)
# goes through the device-wide scan in blocks of 1024 entries
GB_TILE = 1024
SCAN_BLOCK = 1024
N_BIG = 70_001  # 69 tiles: 17,664 counts, 18 scan blocks


def key(metric, ts, *tags, w=W3):
    """row key: metric | base_time(4) | (tagk tagv)*"""
    b = metric.to_bytes(w[0], "big") + ts.to_bytes(4, "big")
    for k, v in tags:
        b += k.to_bytes(w[1], "big") + v.to_bytes(w[2], "big")
    return b


def uid(x, n=3):
    return x.to_bytes(n, "big")


def pairs_of(k, w):
    pos, out = w[0] + 4, []
    while pos < len(k):
        out.append((k[pos:pos + w[1]], k[pos + w[1]:pos + w[1] + w[2]]))
        pos += w[1] + w[2]
    return out


def brute_tags(keys, kept, w=W3):
    """common: the intersection of the kept spans' pair sets; aggregated: the
    first kept span's names minus the common names (in its key's order)"""
    live = [k for i, k in enumerate(keys) if kept is None or kept[i]]
    if not live:
        return {}, []
    common = set(pairs_of(live[0], w))
    for k in live[1:]:
        common &= set(pairs_of(k, w))
    names = {nm for nm, _ in common}
    return dict(common), [nm for nm, _ in pairs_of(live[0], w) if nm not in names]


def pack_keys(keys):
    off = np.zeros(len(keys) + 1, np.uint64)
    if keys:
        off[1:] = np.cumsum([len(k) for k in keys])
    return off, np.frombuffer(b"".join(keys), np.uint8).copy()


def sorted_keys(keys, w=W3):
    return sorted(keys, key=lambda k: core.span_cmp_key(k, w[0]))


# ===================================================================== CPU ====
def test_compute_tags_hand_cases():
    host, dc, rack = uid(1), uid(2), uid(3)
    a = key(7, 0, (1, 10), (2, 20))
    # a single span: every tag is common
    assert core.compute_tags([a]) == ({host: uid(10), dc: uid(20)}, [])
    # a differing value
    b = key(7, 0, (1, 11), (2, 20))
    assert core.compute_tags([a, b]) == ({dc: uid(20)}, [host])
    # a tag missing in a later span
    c = key(7, 0, (2, 20))
    assert core.compute_tags([a, c]) == ({dc: uid(20)}, [host])
    # a tag only a later span carries is reported nowhere
    d = key(7, 0, (1, 10), (2, 20), (3, 30))
    assert core.compute_tags([a, d]) == ({host: uid(10), dc: uid(20)}, [])
    assert rack not in core.compute_tags([a, d])[1]
    # the first span filtered out: the base changes
    assert core.compute_tags([c, a, b], kept=[False, True, True]) == ({dc: uid(20)}, [host])
    assert core.compute_tags([c, d, a], kept=[False, True, True]) == ({host: uid(10), dc: uid(20)}, [rack])
    # nothing kept
    assert core.compute_tags([a, b], kept=[False, False]) == ({}, [])
    assert core.compute_tags([]) == ({}, [])
    # the aggregated names come in the base key's order
    e = key(7, 0, (1, 99), (2, 98), (3, 30))
    assert core.compute_tags([d, e]) == ({rack: uid(30)}, [host, dc])
    for ks, kept in [([a, b, c, d, e], None), ([a, b, c, d, e], [0, 1, 0, 1, 1]), ([d, a], None)]:
        assert core.compute_tags(ks, kept) == brute_tags(ks, kept)


def test_compute_tags_other_widths():
    w = (2, 1, 4)
    a, b = key(7, 0, (1, 10), (2, 0x01020304), w=w), key(7, 0, (1, 11), (2, 0x01020304), w=w)
    assert core.compute_tags([a, b], None, *w) == ({uid(2, 1): uid(0x01020304, 4)}, [uid(1, 1)])


def test_span_in_range():
    T = T0
    s = core.Span(I([(T + 100, 1), (T + 200, 2)]) + I([(T + 3600 + 5, 3)]))
    assert core.span_in_range(s, 0, U32MAX)
    assert core.span_in_range(s, T + 3605, T + 9999)      # last >= start
    assert not core.span_in_range(s, T + 3606, T + 9999)  # ends before the window
    assert core.span_in_range(s, 0, T + 100)              # first <= end
    assert not core.span_in_range(s, 0, T + 99)           # starts after the window
    assert core.span_in_range(core.Span(), 0, 1)          # no rows: kept (the run reports E_EMPTY_SPAN)


def test_struct_layout_matches_ctypes(tmp_path):
    """sizeof / offsetof of the two new structs, from C (gcc, C11, -Werror),
    == _abi.py's ctypes."""
    exe = str(tmp_path / "abi_check_groupby")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "abi_check_groupby.c"), "-o", exe], check=True)
    d = json.loads(subprocess.run([exe], capture_output=True, text=True, check=True).stdout)
    assert d["abi_version"] == _abi.ABI_VERSION == 8
    assert d["max_tags"] == _abi.MAX_TAGS and d["hot_groupby"] == _abi.HOT_GROUPBY
    ctypes_of = {"tsdbhip_keys_desc": _abi.KeysDesc, "tsdbhip_groups_out": _abi.GroupsOut}
    assert set(d["structs"]) == set(ctypes_of)
    for name, st in ctypes_of.items():
        c = d["structs"][name]
        assert c["size"] == C.sizeof(st), name
        assert [f[0] for f in st._fields_] == list(c["fields"]), name
        for fname, ftype in st._fields_:
            off, size = c["fields"][fname]
            assert getattr(st, fname).offset == off, (name, fname)
            assert C.sizeof(ftype) == size, (name, fname)


def test_exports_and_header_agree_on_v8():
    from opentsdb_amd import _lib
    for name in ("tsdbhip_groupby_plan", "tsdbhip_desc_gather", "tsdbhip_desc_gather_free"):
        assert name in _lib.EXPORTS
    hdr = open(os.path.join(ROOT, "include", "tsdbhip.h")).read()
    assert "#define TSDBHIP_ABI_VERSION 8" in hdr


def test_host_checks_clean_under_asan_ubsan(tmp_path):
    """the host-side validation (key_off bounds, group_bys order, the gather's
    order range: csrc/groupby_host.h) as a stand-alone program under
    AddressSanitizer + UndefinedBehaviorSanitizer; any report aborts it"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "san_groupby")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "san_groupby.cc"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "groupby host checks ok" in r.stdout


class FakeTsdb:
    tag_names = {uid(1): "host", uid(2): "dc", uid(3): "rack"}
    tag_values = {uid(10): "web01", uid(11): "web02", uid(20): "lga", uid(30): "r7"}


def test_spangroup_tags_host_path():
    T = T0
    a = core.Span(I([(T + 1, 1)]), key=key(7, T, (1, 10), (2, 20), (3, 30)))
    b = core.Span(I([(T + 2, 2)]), key=key(7, T, (1, 11), (2, 20)))
    late = core.Span(I([(T + 9000, 2)]), key=key(7, T + 7200, (1, 10), (2, 21)))
    sg = core.SpanGroup(None, 0, U32MAX, [a, b], False, core.Aggregators.SUM)
    assert sg.getTags() == {uid(2): uid(20)}
    assert sg.getAggregatedTags() == [uid(1), uid(3)]
    named = core.SpanGroup(FakeTsdb(), 0, U32MAX, [a, b], False, core.Aggregators.SUM)
    assert named.getTags() == {"dc": "lga"}
    assert named.getAggregatedTags() == ["host", "rack"]
    # SpanGroup.add's time filter: the late span does not take part
    win = core.SpanGroup(FakeTsdb(), 0, T + 100, [a, b, late], False, core.Aggregators.SUM)
    assert win.getTags() == {"dc": "lga"}
    allin = core.SpanGroup(None, 0, U32MAX, [a, b, late], False, core.Aggregators.SUM)
    assert allin.getTags() == {} and allin.getAggregatedTags() == [uid(1), uid(2), uid(3)]
    empty = core.SpanGroup(None, 0, U32MAX, [], False, core.Aggregators.SUM)
    assert empty.getTags() == {} and empty.getAggregatedTags() == []
    nokey = core.SpanGroup(None, 0, U32MAX, [core.Span(I([(T + 1, 1)]))], False, core.Aggregators.SUM)
    with pytest.raises(ValueError, match="row key"):
        nokey.getTags()


# ===================================================================== GPU ====
def run_plan(ctx, keys, group_bys, kept=None, w=W3, **kw):
    off, kb = pack_keys(keys)
    return core.run_groupby_plan(ctx, off, kb, group_bys, kept, *w, **kw)


def expected_plan(keys, group_bys, kept, w):
    """(group keys, order, group_span_start, tags per group) from plan_groups
    and the brute force; keys in SpanCmp order"""
    gk, order, gss = core.plan_groups(keys, group_bys, *w)
    if not keys:
        gk, gss = [], [0]  # (no spans: no group, TsdbQuery.java:295-297)
    tags = []
    for g in range(len(gk)):
        members = order[gss[g]:gss[g + 1]]
        tags.append(brute_tags([keys[i] for i in members], None if kept is None else [kept[i] for i in members], w))
    return gk, order, gss, tags


def assert_plan(plan, exp, n):
    gk, order, gss, tags = exp
    assert plan.n_groups == len(gk)
    assert plan.n_grouped == len(order) and plan.n_dropped == n - len(order)
    assert plan.group_keys == gk
    assert plan.order.tolist() == order
    assert plan.group_span_start.tolist() == gss
    for g in range(len(gk)):
        assert plan.tags_of(g) == tags[g], g


def check(ctx, keys, group_bys, kept=None, w=W3):
    rc, plan = run_plan(ctx, keys, group_bys, kept, w)
    assert rc == 0, ctx.last_error()
    assert_plan(plan, expected_plan(keys, group_bys, kept, w), len(keys))
    return plan


def make_keys(n, seed, host_values, w=W3, drop_every=0, dc_values=3):
    """n distinct keys in SpanCmp order: host (name 1), dc (name 2), a constant
    tag (name 3) and a unique one (name 4); every drop_every-th lacks host"""
    rng = np.random.default_rng(seed)
    hv = rng.choice(np.asarray(host_values), n) if n else []
    dv = rng.integers(0, dc_values, n) if n else []
    keys = []
    for i in range(n):
        tags = [(2, int(dv[i])), (3, 7), (4, i)]
        if not (drop_every and i % drop_every == drop_every - 1):
            tags.insert(0, (1, int(hv[i])))
        keys.append(key(9, int(rng.integers(0, 1 << 31)), *tags, w=w))
    return sorted_keys(keys, w)


@functools.lru_cache(maxsize=None)
def big_case():
    """the 70k-span case, its kept mask and both expectations, built once"""
    keys = make_keys(N_BIG, 21, [1, 2, 3, 0x800000, 0x0100, 0x010203, 70000], drop_every=16)
    kept = (np.random.default_rng(4).random(N_BIG) < 0.6).astype(np.uint8)
    gbs = [uid(1)]
    return keys, kept, gbs, expected_plan(keys, gbs, None, W3), expected_plan(keys, gbs, kept.tolist(), W3)


@pytest.mark.gpu
def test_hand_example(ctx):
    """the five keys of test_plan_groups_orders_like_bytemap_and_spancmp, in SpanCmp order"""
    host, dc = 1, 2
    keys = [
        key(7, 0, (dc, 1)),                     # no host tag: dropped when grouping by host
        key(7, 7200, (dc, 1), (host, 3)),
        key(7, 0, (dc, 1), (host, 0x800000)),   # unsigned compare: 0x80.. after 0x00..
        key(7, 0, (dc, 2), (host, 1)),
        key(7, 3600, (dc, 2), (host, 9)),
    ]
    assert keys == sorted_keys(keys)
    rc, p = run_plan(ctx, keys, [uid(host)])
    assert rc == 0, ctx.last_error()
    assert p.group_keys == [uid(1), uid(3), uid(9), uid(0x800000)]
    assert p.order.tolist() == [3, 1, 4, 2] and p.group_span_start.tolist() == [0, 1, 2, 3, 4]
    assert (p.n_groups, p.n_grouped, p.n_dropped) == (4, 4, 1)
    assert p.tags_of(0) == ({uid(dc): uid(2), uid(host): uid(1)}, [])
    rc, p = run_plan(ctx, keys, [uid(dc)])
    assert rc == 0, ctx.last_error()
    assert p.group_keys == [uid(1), uid(2)]
    assert p.order.tolist() == [0, 1, 2, 3, 4] and p.group_span_start.tolist() == [0, 3, 5]
    assert p.tags_of(0) == ({uid(dc): uid(1)}, [])          # base: the key without host
    assert p.tags_of(1) == ({uid(dc): uid(2)}, [uid(host)])
    # two group_bys: 2 * value_width bytes, the lower name id (host) most significant
    rc, p = run_plan(ctx, keys, [uid(host), uid(dc)])
    assert rc == 0, ctx.last_error()
    assert p.group_keys == [uid(1) + uid(2), uid(3) + uid(1), uid(9) + uid(2), uid(0x800000) + uid(1)]
    assert p.order.tolist() == [3, 1, 4, 2] and p.n_dropped == 1
    # no GROUP BY: one group of every span, a key of length 0
    rc, p = run_plan(ctx, keys, None)
    assert rc == 0, ctx.last_error()
    assert p.group_keys == [b""] and p.group_span_start.tolist() == [0, 5] and p.order.tolist() == [0, 1, 2, 3, 4]
    assert p.tags_of(0) == ({}, [uid(dc)])
    # plan_groups_device: keys in any order, order mapped back to the caller's indices
    shuffled = [keys[i] for i in (4, 2, 1, 3, 0)]
    gk, order, gss, tags = core.plan_groups_device(ctx, shuffled, [uid(host)])
    assert (gk, order, gss) == core.plan_groups(shuffled, [uid(host)])
    assert order == [3, 2, 0, 1] and len(tags) == 4


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, GB_TILE + 1, SCAN_BLOCK // 256 * GB_TILE + 1])
def test_wave_and_block_edges(ctx, n):
    keys = make_keys(n, 100 + n, [5, 6, 0x800000, 0x0201, 300], drop_every=7 if n > 7 else 0)
    check(ctx, keys, [uid(1)])
    check(ctx, keys, None)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [97, 2 * GB_TILE + 5])
def test_edge_base_times(ctx, n):
    """keys that differ in their 4-byte base time only by these values: the
    base time takes no part in SpanCmp, the grouping or the tags; against the
    host plan"""
    rng = np.random.default_rng(n)
    keys = []
    for i in range(n):
        tags = [(1, int(rng.choice([5, 6, 0x800000, 0x0201]))), (2, int(rng.integers(0, 3))), (3, 7), (4, i)]
        keys.append(key(9, EDGE_BASES[int(rng.integers(0, 4))], *(tags[1:] if i % 7 == 6 else tags)))
    keys = sorted_keys(keys)
    assert {int.from_bytes(k[3:7], "big") for k in keys} == set(EDGE_BASES)
    kept = (rng.random(n) < 0.6).astype(np.uint8)
    for gbs in ([uid(1)], [uid(1), uid(2)], None):
        check(ctx, keys, gbs)
        check(ctx, keys, gbs, kept.tolist())
    gk, order, gss, _ = core.plan_groups_device(ctx, keys[::-1], [uid(1)])
    assert (gk, order, gss) == core.plan_groups(keys[::-1], [uid(1)])


@pytest.mark.gpu
def test_more_than_one_scan_block(ctx):
    keys, _, gbs, exp, _ = big_case()
    rc, plan = run_plan(ctx, keys, gbs)
    assert rc == 0, ctx.last_error()
    assert_plan(plan, exp, N_BIG)
    t = ctx.timing()
    assert t.hot_kernel == _abi.HOT_GROUPBY and t.alg_bytes > sum(len(k) for k in keys)


@pytest.mark.gpu
def test_digit_handling(ctx):
    n = 3000
    # values below 256: one live digit
    check(ctx, make_keys(n, 1, list(range(200))), [uid(1)])
    assert ctx.timing().n_grid == 1
    # values that use all three bytes
    vals = np.random.default_rng(2).integers(0, 1 << 24, 500).tolist() + [0xFFFFFF, 0]
    check(ctx, make_keys(n, 2, vals), [uid(1)])
    assert ctx.timing().n_grid == 3
    # two group-by tags: six digit positions
    check(ctx, make_keys(n, 3, vals, dc_values=1 << 24), [uid(1), uid(2)])
    assert ctx.timing().n_grid == 6
    # a tag constant over all spans: a single group, every pass skipped
    p = check(ctx, make_keys(n, 4, [5]), [uid(3)])
    assert p.n_groups == 1 and ctx.timing().n_grid == 0
    # ... and with dropped spans only the drop pass runs
    p = check(ctx, make_keys(n, 5, [5], drop_every=3), [uid(1)])
    assert p.n_groups == 1 and p.n_dropped == n // 3 and ctx.timing().n_grid == 1


@pytest.mark.gpu
def test_stability(ctx):
    keys = make_keys(20_000, 8, [3, 0x800000, 0x0100, 77, 0x010000])
    p = check(ctx, keys, [uid(1)])
    assert p.n_groups == 5
    gss, order = p.group_span_start.tolist(), p.order
    for g in range(5):
        assert gss[g + 1] - gss[g] > 3000
        assert (np.diff(order[gss[g]:gss[g + 1]].astype(np.int64)) > 0).all()


@pytest.mark.gpu
def test_all_dropped(ctx):
    keys = make_keys(500, 9, [1, 2])
    rc, p = run_plan(ctx, keys, [uid(9)])
    assert rc == 0 and p.n_groups == 0 and p.n_dropped == 500 and p.n_grouped == 0
    assert p.group_span_start.tolist() == [0]


@pytest.mark.gpu
@pytest.mark.parametrize("w,n", [((3, 2, 4), 2000), ((2, 1, 1), 200)])
def test_other_widths(ctx, w, n):
    vals = [1, 2, 200] if w[2] == 1 else [1, 0x80000000, 0x01000000, 0x00010000, 258]
    keys = make_keys(n, 10, vals, w=w, drop_every=9, dc_values=3)
    check(ctx, keys, [uid(1, w[1])], w=w)
    check(ctx, keys, [uid(1, w[1]), uid(2, w[1])], w=w)
    kept = (np.random.default_rng(1).random(n) < 0.5).astype(np.uint8)
    check(ctx, keys, [uid(2, w[1])], kept=kept.tolist(), w=w)


@pytest.mark.gpu
def test_span_kept(ctx):
    keys = sorted_keys([
        key(7, 0, (1, 5), (2, 1)),           # group 5, first: no rack
        key(7, 0, (1, 5), (2, 1), (3, 9)),
        key(7, 0, (1, 5), (2, 2), (3, 9)),
        key(7, 0, (1, 6), (2, 1)),           # group 6
        key(7, 0, (1, 6), (2, 3)),
    ])
    p = check(ctx, keys, [uid(1)])
    assert p.tags_of(0) == ({uid(1): uid(5)}, [uid(2)])
    # clearing a group's first span changes its base tags
    p = check(ctx, keys, [uid(1)], kept=[0, 1, 1, 1, 1])
    assert p.tags_of(0) == ({uid(1): uid(5), uid(3): uid(9)}, [uid(2)])
    assert p.group_ntags.tolist() == [3, 2]
    # clearing a whole group: still present, no tags
    p = check(ctx, keys, [uid(1)], kept=[1, 1, 1, 0, 0])
    assert p.n_groups == 2 and p.group_ntags.tolist() == [2, 0] and p.tags_of(1) == ({}, [])
    assert p.group_span_start.tolist() == [0, 3, 5]
    p = check(ctx, keys, None, kept=[0, 0, 0, 0, 0])
    assert p.n_groups == 1 and p.group_ntags.tolist() == [0]


@pytest.mark.gpu
def test_span_kept_random_mask(ctx):
    keys, kept, gbs, _, exp = big_case()
    rc, plan = run_plan(ctx, keys, gbs, kept)
    assert rc == 0, ctx.last_error()
    assert_plan(plan, exp, N_BIG)


@pytest.mark.gpu
def test_device_resident_keys(ctx):
    import torch
    keys, kept, gbs, _, exp = big_case()
    off, kb = pack_keys(keys)
    dev = torch.device("cuda", ctx.device)
    t_off = torch.from_numpy(off.view(np.int64)).to(dev)
    t_kb = torch.from_numpy(kb).to(dev)
    t_kept = torch.from_numpy(kept).to(dev)
    torch.cuda.synchronize(dev)
    rc, plan = core.run_groupby_plan(ctx, t_off.data_ptr(), t_kb.data_ptr(), gbs, t_kept.data_ptr(), device=True,
                                     n_spans=len(keys), key_nbytes=len(kb))
    assert rc == 0, ctx.last_error()
    assert_plan(plan, exp, N_BIG)
    assert ctx.timing().h2d_bytes == 0
    rc, host_plan = run_plan(ctx, keys, gbs, kept)
    assert rc == 0 and ctx.timing().h2d_bytes > 0
    for a, b in [(plan.order, host_plan.order), (plan.group_span_start, host_plan.group_span_start),
                 (plan.group_tags, host_plan.group_tags), (plan.group_common, host_plan.group_common),
                 (plan.group_ntags, host_plan.group_ntags)]:
        np.testing.assert_array_equal(a, b)
    assert plan.group_keys == host_plan.group_keys


def assert_rejected(ctx, rc, plan, code, words=()):
    assert rc == code, (_abi.ERR_NAMES.get(rc, rc), ctx.last_error())
    for word in words:
        assert word in ctx.last_error(), ctx.last_error()
    for a in plan.raw:  # nothing was written
        assert not a.any()


@pytest.mark.gpu
def test_rejections(ctx):
    keys = make_keys(300, 12, [1, 2, 3])
    gb = [uid(1)]
    # a swapped pair, a duplicate, a base-time-only difference
    bad = list(keys)
    bad[130], bad[131] = bad[131], bad[130]
    assert_rejected(ctx, *run_plan(ctx, bad, gb), _abi.E_UNSORTED, ["span 131"])
    bad = keys[:200] + [keys[199]] + keys[200:]
    assert_rejected(ctx, *run_plan(ctx, bad, gb), _abi.E_UNSORTED, ["span 200"])
    twin = keys[64][:3] + (int.from_bytes(keys[64][3:7], "big") ^ 1).to_bytes(4, "big") + keys[64][7:]
    bad = keys[:65] + [twin] + keys[65:]
    assert_rejected(ctx, *run_plan(ctx, bad, gb), _abi.E_UNSORTED, ["span 65"])
    # (the first offending span wins)
    bad[10], bad[11] = bad[11], bad[10]
    assert_rejected(ctx, *run_plan(ctx, bad, gb), _abi.E_UNSORTED, ["span 11"])
    # key shape
    bad = list(keys)
    bad[77] = bad[77][:-1]
    assert_rejected(ctx, *run_plan(ctx, bad, gb), _abi.E_INVALID_ARG, ["span 77"])
    bad[5] = bad[5][:6]  # shorter than metric + base time
    assert_rejected(ctx, *run_plan(ctx, bad, gb), _abi.E_INVALID_ARG, ["span 5"])
    nine = sorted_keys(keys + [key(9, 0, *[(k, 1) for k in range(1, 10)])])
    assert_rejected(ctx, *run_plan(ctx, nine, gb), _abi.E_INVALID_ARG, ["span"])
    eight = sorted_keys(keys + [key(9, 0, *[(k, 1) for k in range(1, 9)])])
    assert run_plan(ctx, eight, gb)[0] == 0
    # arguments
    assert_rejected(ctx, *run_plan(ctx, keys, [uid(2), uid(1)]), _abi.E_INVALID_ARG, ["ascending"])
    assert_rejected(ctx, *run_plan(ctx, keys, [uid(1), uid(1)]), _abi.E_INVALID_ARG, ["ascending"])
    assert_rejected(ctx, *run_plan(ctx, keys, [uid(k) for k in range(1, 10)]), _abi.E_INVALID_ARG)
    assert_rejected(ctx, *run_plan(ctx, keys, gb, w=(0, 3, 3)), _abi.E_INVALID_ARG, ["width"])
    assert_rejected(ctx, *run_plan(ctx, keys, gb, w=(3, 3, 9)), _abi.E_INVALID_ARG, ["width"])
    # key_off does not end at key_nbytes (the buffer holds the extra bytes)
    off, kb = pack_keys(keys)
    kb4 = np.concatenate([kb, np.zeros(4, np.uint8)])
    assert_rejected(ctx, *core.run_groupby_plan(ctx, off, kb4, gb), _abi.E_INVALID_ARG, ["key_off"])
    off2 = off.copy()
    off2[100] = off2[101] + 1  # decreasing
    assert_rejected(ctx, *core.run_groupby_plan(ctx, off2, kb, gb), _abi.E_INVALID_ARG, ["key_off"])
    # capacity: n_groups set for the retry, nothing written
    rc, full = run_plan(ctx, keys, gb)
    assert rc == 0 and full.n_groups == 3
    rc, p = run_plan(ctx, keys, gb, capacity=full.n_groups - 1)
    assert_rejected(ctx, rc, p, _abi.E_CAPACITY)
    assert (p.n_groups, p.n_grouped, p.n_dropped) == (3, 300, 0)


@pytest.mark.gpu
def test_rejections_device_resident(ctx):
    """the same checks run on the device for keys already in HBM"""
    import torch
    keys = make_keys(300, 12, [1, 2, 3])
    dev = torch.device("cuda", ctx.device)

    def run(off, kb, nbytes=None):
        t_off, t_kb = torch.from_numpy(off.view(np.int64)).to(dev), torch.from_numpy(kb).to(dev)
        torch.cuda.synchronize(dev)
        return core.run_groupby_plan(ctx, t_off.data_ptr(), t_kb.data_ptr(), [uid(1)], device=True,
                                     n_spans=len(off) - 1, key_nbytes=len(kb) if nbytes is None else nbytes)

    off, kb = pack_keys(keys)
    assert run(off, kb)[0] == 0
    kb4 = np.concatenate([kb, np.zeros(4, np.uint8)])
    assert_rejected(ctx, *run(off, kb4), _abi.E_INVALID_ARG, ["key_off"])
    off2 = off.copy()
    off2[100] = off2[101] + 1
    assert_rejected(ctx, *run(off2, kb), _abi.E_INVALID_ARG, ["span 99"])  # (its key now has a bad length)
    off3 = off.copy()
    off3[200] = len(kb) + 1000  # past the key bytes: never read
    assert_rejected(ctx, *run(off3, kb), _abi.E_INVALID_ARG, ["key_off", "span 199"])
    bad = list(keys)
    bad[130], bad[131] = bad[131], bad[130]
    assert_rejected(ctx, *run(*pack_keys(bad)), _abi.E_UNSORTED, ["span 131"])


@pytest.mark.gpu
def test_reentrant(ctx):
    cases = [(make_keys(5000, 30 + i, [1, 2, 3, 0x800000][:2 + i], drop_every=5 + i), [uid(1)]) for i in range(2)]
    exps = [expected_plan(k, g, None, W3) for k, g in cases]
    errs = []
    gate = threading.Barrier(2)

    def work(i):
        try:
            gate.wait()
            for _ in range(5):
                rc, plan = run_plan(ctx, cases[i][0], cases[i][1])
                assert rc == 0
                assert_plan(plan, exps[i], 5000)
        except BaseException as e:  # noqa: BLE001
            errs.append(e)

    ts = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs


# ------------------------------------------------------------------ gather ----
def download(ctx, d):
    R, S = int(d.n_rows), int(d.n_spans)
    arrs = [np.zeros(S + 1, np.uint64), np.zeros(R, np.uint32), np.zeros(R, np.uint32), np.zeros(R, np.uint64),
            np.zeros(R, np.uint64), np.zeros(R, np.uint32), np.zeros(d.qual_nbytes, np.uint8),
            np.zeros(d.val_nbytes, np.uint8)]
    ctx.check(ctx._lib.tsdbhip_desc_download(ctx.handle, C.byref(d), *[a.ctypes.data for a in arrs]))
    return packing.SpanSet(*arrs)


def numpy_gather(ss, order):
    rows = [np.arange(int(ss.span_row_start[s]), int(ss.span_row_start[s + 1])) for s in order]
    srs = np.zeros(len(order) + 1, np.uint64)
    if rows:
        srs[1:] = np.cumsum([len(r) for r in rows])
    r = np.concatenate(rows).astype(np.int64) if rows else np.zeros(0, np.int64)
    return packing.SpanSet(srs, ss.row_base[r], ss.row_ncells[r], ss.row_qual_off[r], ss.row_val_off[r],
                           ss.row_val_len[r], ss.qual_bytes, ss.val_bytes)


def gather(ctx, d, order):
    out = _abi.SgDesc()
    o = np.ascontiguousarray(order, np.uint32)
    rc = ctx._lib.tsdbhip_desc_gather(ctx.handle, C.byref(d), _abi.ptr(o, C.c_uint32), len(o), C.byref(out))
    return rc, out


@pytest.mark.gpu
@pytest.mark.parametrize("n_spans,n_points,step", [(120, 700, 10), (6, 3600 * 70, 1)])
def test_gather(ctx, n_spans, n_points, step):
    """(120 spans of 700 points at step 10: two rows a span; 70 hourly rows a span: more than a wave of rows)"""
    import oracle
    L = ctx._lib
    p = _abi.SynthParams(seed=11, n_spans=n_spans, n_points=n_points, t0=T0, step=step, kind=_abi.SYN_INT64_COUNTER)
    d = _abi.SgDesc()
    ctx.check(L.tsdbhip_synth_generate(ctx.handle, C.byref(p), C.byref(d)))
    try:
        host = download(ctx, d)
        rng = np.random.default_rng(6)
        perm = rng.permutation(n_spans)
        subset = np.sort(rng.choice(n_spans, n_spans // 3, replace=False))[::-1].copy()
        for order in (perm, subset):
            rc, g = gather(ctx, d, order)
            assert rc == 0, ctx.last_error()
            try:
                exp = numpy_gather(host, order)
                assert g.n_spans == len(order) and g.n_rows == exp.n_rows and g.flags & _abi.DESC_DEVICE
                assert C.cast(g.qual_bytes, C.c_void_p).value == C.cast(d.qual_bytes, C.c_void_p).value  # borrowed
                got = download(ctx, g)
                for a, b in zip([got.span_row_start, got.row_base, got.row_ncells, got.row_qual_off,
                                 got.row_val_off, got.row_val_len],
                                [exp.span_row_start, exp.row_base, exp.row_ncells, exp.row_qual_off,
                                 exp.row_val_off, exp.row_val_len]):
                    np.testing.assert_array_equal(a, b)
                # the batch over the gathered descriptor, group by group against the oracle
                n = len(order)
                gss = sorted({0, n} | set(rng.integers(1, n, 4).tolist()))
                cells = np.concatenate([[0], np.cumsum(exp.row_ncells.astype(np.int64))])
                cum = cells[exp.span_row_start.astype(np.int64)]
                caps = np.maximum(1, cum[np.array(gss[1:])] - cum[np.array(gss[:-1])])
                for agg in (_abi.AGG_SUM, _abi.AGG_DEV):
                    for ds in ((0, 0), (60, _abi.AGG_AVG)):
                        rc, res = core.run_spanset_batch(ctx, None, gss, 0, U32MAX, agg, False, ds[0], ds[1],
                                                         capacities=caps, device_desc=g)
                        assert rc == 0, ctx.last_error()
                        for k in range(len(gss) - 1):
                            o = oracle.spangroup(exp.shard(gss[k], gss[k + 1]), 0, U32MAX, agg, False, ds[0], ds[1])
                            assert_same(res[k], o)
            finally:
                assert L.tsdbhip_desc_gather_free(ctx.handle, C.byref(g)) == 0
                assert not g.span_row_start and not g.row_base and not g.row_val_len
                assert L.tsdbhip_desc_gather_free(ctx.handle, C.byref(g)) == 0  # a second call is harmless
        # rejections
        rc, _ = gather(ctx, d, [0, n_spans])
        assert rc == _abi.E_INVALID_ARG and "order[1]" in ctx.last_error()
        hd = _abi.SgDesc()
        host.fill_desc(hd)
        hd.flags = 0
        rc, _ = gather(ctx, hd, [0])
        assert rc == _abi.E_INVALID_ARG
        rc, g = gather(ctx, d, [])
        assert rc == 0 and g.n_spans == 0 and g.n_rows == 0
        L.tsdbhip_desc_gather_free(ctx.handle, C.byref(g))
    finally:
        L.tsdbhip_synth_free(ctx.handle, C.byref(d))


# -------------------------------------------------------------- end to end ----
@pytest.mark.gpu
def test_group_by_and_aggregate_device_plan(ctx):
    """the scenario of test_group_by_and_aggregate_mirror with device_plan=True"""
    import oracle
    T = T0
    host = uid(1)
    spans, expect = {}, {}
    rng = np.random.default_rng(3)
    for h in range(5):
        for s in range(1 + h):
            k = key(9, T, (1, 0x10 + h), (2, s))
            pts = [(T + 10 * i + s, int(rng.integers(-50, 50))) for i in range(30)]
            spans[k] = core.Span(I(pts))
            expect.setdefault(h, []).append((k, I(pts)))
    groups = core.group_by_and_aggregate(spans, [host], 0, U32MAX, False, core.Aggregators.SUM, ctx=ctx,
                                         device_plan=True)
    assert len(groups) == 5
    for h, grp in enumerate(groups):
        members = sorted(expect[h], key=lambda kv: core.span_cmp_key(kv[0]))
        o = oracle.spangroup(packing.pack_spans([r for _, r in members]), 0, U32MAX, 0)
        got = list(grp)
        assert [p.timestamp() for p in got] == list(o.ts)
        assert [p.longValue() for p in got] == list(o.bits)
        assert grp.aggregatedSize() == o.n_input_points
        common, agg = brute_tags([k for k, _ in members], None)
        assert grp.getTags() == common and grp.getAggregatedTags() == agg
        assert grp.getTags()[host] == uid(0x10 + h)
        assert (grp.getAggregatedTags() == [uid(2)]) == (h > 0)
    # the host plan gives the same groups and, computed on first use, the same tags
    plain = core.group_by_and_aggregate(spans, [host], 0, U32MAX, False, core.Aggregators.SUM, ctx=ctx)
    for a, b in zip(groups, plain):
        assert a.getTags() == b.getTags() and a.getAggregatedTags() == b.getAggregatedTags()
        assert [p.longValue() for p in a] == [p.longValue() for p in b]
