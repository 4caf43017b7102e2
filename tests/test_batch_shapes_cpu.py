"""The batches of tests/batch_shapes.py checked without a GPU: each reaches the
regime it is named for (through the restatement of the batch's host geometry,
so a retuned constant fails here and the shapes get re-picked), the oracle
gives every group the code the GPU test expects, and capacities and closed
forms are what test_batch_shapes.py assumes."""
import time

import numpy as np
import pytest

import batch_shapes as bs
from helpers import T0
from opentsdb_amd import _abi

AGGS = [0, 1, 2, 3, 4]
DS = [(0, 0), (60, 3)]


def chunk_sizes(nk, spc, n_chunks):
    return [min(spc, nk - c * spc) for c in range(n_chunks)]


# ---- the builders ----
def test_pack_cells_matches_the_packer():
    """the vectorised writer lays rows out as packing.pack_spans does"""
    from helpers import F, I
    from opentsdb_amd import packing
    rng = np.random.default_rng(1)
    ts = [np.sort(rng.choice(9000, 40, replace=False)) + T0 for _ in range(4)]
    iv = [bs.wide_ints(rng, 40) for _ in range(4)]
    fv = [bs.finite(rng, 40) for _ in range(4)]
    kinds = [bs.KI, bs.K8, bs.KF4, bs.KF8]
    ref = packing.pack_spans([I(list(zip(ts[0].tolist(), iv[0].tolist()))),
                              I(list(zip(ts[1].tolist(), iv[1].tolist())), minimal=False),
                              F(list(zip(ts[2].tolist(), fv[2].tolist()))),
                              F(list(zip(ts[3].tolist(), fv[3].tolist())), double=True)])
    flt = np.repeat(np.array(kinds) >= bs.KF4, 40)
    got = bs.pack_cells([40] * 4, kinds, np.concatenate(ts), np.where(flt, 0, np.concatenate(iv)),
                        np.where(flt, np.concatenate(fv), 0.0))
    for f in ("span_row_start", "row_base", "row_ncells", "row_qual_off", "row_val_off", "row_val_len"):
        np.testing.assert_array_equal(getattr(got, f), getattr(ref, f), err_msg=f)
    nq, nv = len(ref.qual_bytes), len(ref.val_bytes)
    np.testing.assert_array_equal(got.qual_bytes[:nq], ref.qual_bytes)
    np.testing.assert_array_equal(got.val_bytes[:nv], ref.val_bytes)
    assert (got.row_qual_off % 8 == 0).all() and (got.row_val_off % 16 == 0).all()


def test_many_groups_builds_fast():
    """65 537 groups are written without a Python step a span: the best of
    three builds (a busy machine slows one, hardly all) stays under a second,
    where a loop over the spans through the KeyValue encoders takes several"""
    best = np.inf
    for _ in range(3):
        bs._CACHE.pop(("many_groups", 65537), None)
        t = time.perf_counter()
        c = bs.many_groups(65537)
        best = min(best, time.perf_counter() - t)
        if best < 1.0:
            break
    assert c.G == 65537 and c.ss.n_spans >= 65537
    assert best < 1.0, f"{best:.2f} s"


# ---- A / G: tile groups ----
@pytest.mark.parametrize("kind", bs.LONG_KINDS)
@pytest.mark.parametrize("pos", bs.POSITIONS)
def test_tile_groups_regime(pos, kind):
    c = bs.tile_groups(pos, kind)
    rate = kind == "rate"
    L1, L2 = c.meta["L1"], c.meta["L2"]
    assert c.G == bs.N_FILL + 2
    assert {"first": L1 == 0, "middle": 0 < L1 < L2 < c.G - 1, "last": L1 == c.G - 1 and L2 == 0}[pos]
    for ds in DS:
        for agg in AGGS:
            for exact in (False, True):
                q = bs.geom(c, agg, rate, exact)
                assert not q.wide and q.nk[L1] == q.nk[L2] == 3 and q.nk[L1] / q.n_kept < 1 / 256
                for L in (L1, L2):
                    o = c.ref(L, agg, rate, ds)
                    assert o.code == 0
                    spc, n_chunks, tpw, ntg, _ = q.rg(L, len(o.ts))
                    assert n_chunks == 1 and spc == 3
                    if ds[0] == 0:
                        assert tpw == 2 if L == L1 else tpw >= 3, (L, tpw, len(o.ts))
                    else:
                        assert tpw >= 2, (L, tpw, len(o.ts))  # (60-s buckets: fewer points, still a tile group)
                    assert ntg >= 2
        assert q.mode[L1] == q.mode[L2] == {"int": 0, "float": 1, "dual": 2, "rate": 1}[kind]
    # offsets of the later long group are non-zero: it follows a group with T > 0
    assert q.wbase[max(L1, L2)] > 1024
    # span b skips an interior tile (its bracket is carried), span c ends before the last tile
    for L in (L1, L2):
        grid = c.ref(L, 0, rate).ts
        tiles = [grid[i:i + 64] for i in range(0, len(grid), 64)]
        s0 = int(c.gss[L])
        pb, pc = c.span_points(s0 + 1), c.span_points(s0 + 2)
        skipped = [i for i, t in enumerate(tiles[1:-1], 1)
                   if pb[0] < t[0] and t[-1] < pb[-1] and not ((pb >= t[0]) & (pb <= t[-1])).any()]
        assert len(skipped) >= 2, "span b has a point in every interior tile"
        assert pc[-1] < tiles[-1][0] and pc[0] > tiles[0][-1]


@pytest.mark.parametrize("kind", bs.LONG_KINDS)
def test_tile_groups_fillers_closed_form(kind):
    """every one-cell group emits its own point (0 under dev; nothing under
    rate): the closed form the GPU test holds the 1000 fillers to"""
    c = bs.tile_groups("middle", kind)
    rate = kind == "rate"
    fill = [g for g in range(c.G) if g not in (c.meta["L1"], c.meta["L2"])]
    for ds in DS:
        for agg in AGGS:
            for g in fill[::7] if (agg, ds) != (0, DS[0]) else fill:
                o = c.ref(g, agg, rate, ds)
                ts, isint, bits = filler_expect(c, g, agg, rate)
                assert o.code == 0 and o.n_input_points == 1
                np.testing.assert_array_equal(o.ts, ts)
                np.testing.assert_array_equal(o.is_int, isint)
                np.testing.assert_array_equal(o.bits, bits)


def filler_expect(c, g, agg, rate):
    s = int(c.gss[g])
    p = int(c.pt0[s])
    if rate:
        z = np.zeros(0, np.int64)
        return z, z.astype(np.uint8), z
    isint = c.kinds[s] < bs.KF4
    v = 0 if agg == 4 else (int(c.ival[p]) if isint else int(c.fval[p:p + 1].view(np.int64)[0]))
    return np.array([c.ts[p]]), np.array([isint], np.uint8), np.array([v], np.int64)


def test_deep_lazy_errors_regime():
    """G: the 3-byte long of L1 and the +Inf of L2 surface past the group's
    first 1024 bitmap words, in a tile a wave reaches after its first tpw"""
    c = bs.tile_groups("middle", "dual", True)
    clean = bs.tile_groups("middle", "dual")
    L1, L2 = c.meta["L1"], c.meta["L2"]
    q = bs.geom(c)
    assert L1 > 0 and q.wbase[L1] > 0
    for L, code in ((L1, _abi.E_ILLEGAL_DATA), (L2, _abi.E_NAN_INF)):
        o = c.ref(L, 0)
        T = len(clean.ref(L, 0).ts)
        tpw = q.rg(L, T)[2]
        assert o.code == code and o.err_index == len(o.ts) and 0 < o.err_index < T
        assert tpw >= 2 and o.err_index // 64 >= tpw
        t_err = int(clean.ref(L, 0).ts[o.err_index])
        assert (t_err - q.lo[L]) // 32 >= bs.RANK_BLOCK
    for g in (L1 - 1, L2 + 1):
        assert c.ref(g, 0).code == 0


def test_deep_errors_regime():
    """G outside a tile group: the errors of groups 1 and 2 lie past the
    group's first 1024 bitmap words"""
    c = bs.deep_errors()
    q = bs.geom(c)
    for g, code in ((bs.DEEP_BAD, _abi.E_ILLEGAL_DATA), (bs.DEEP_INF, _abi.E_NAN_INF)):
        o = c.ref(g, 0)
        assert o.code == code and 0 < o.err_index == len(o.ts)
        grid = np.unique(np.concatenate([c.span_points(s) for s in range(int(c.gss[g]), int(c.gss[g + 1]))]))
        assert o.err_index < len(grid) and (grid[o.err_index] - q.lo[g]) // 32 >= bs.RANK_BLOCK
        assert q.wbase[g] > 0 and q.rg(g, len(grid))[2] == 1
    assert c.ref(0, 0).code == 0 == c.ref(3, 0).code


# ---- B: span chunks ----
def test_span_chunks_regime():
    c = bs.span_chunks()
    q = bs.geom(c)
    assert list(q.nk) == list(bs.CHUNK_NK)
    assert list(q.mode) == [0, 1, 2, 0, 1]  # an int, a float and a dual group side by side
    want = {0: 2, 1: 3, 2: 6}
    for g in range(c.G):
        o = c.ref(g, 0)
        assert o.code == 0 and len(o.ts) <= 15 * 64
        spc, n_chunks, tpw, _, _ = q.rg(g, len(o.ts))
        sizes = chunk_sizes(int(q.nk[g]), spc, n_chunks)
        assert tpw == 1 and sizes[-1] < spc, (g, sizes)  # a short last chunk
        if g in want:
            assert n_chunks == want[g]
    # more than 256 spans, an int and a float group side by side: the (nk + 255) / 256 term is 2 and
    # k_group_stats strides
    for g in (3, 4):
        assert q.nk[g] > bs.GROUP_THREADS and (q.nk[g] + 255) // 256 == 2 and q.rg(g, len(c.ref(g, 0).ts))[1] > 6
    # one chunk under EXACT_ORDER and for integer dev
    assert bs.geom(c, 0, False, True).rg(2, 500)[1] == 1 and bs.geom(c, 4).rg(0, 500)[1] == 1
    assert not q.fast
    for agg in AGGS:
        for rate in (False, True):
            for ds in DS:
                assert all(c.ref(g, agg, rate, ds).code == 0 for g in range(c.G))


def test_direct_chunks_regime():
    c = bs.direct_chunks()
    assert c.ss.n_rows == c.ss.n_spans
    for rate in (False, True):
        q = bs.geom(c, 0, rate)
        assert q.fast and list(q.nk) == list(bs.DIRECT_NK)
        for g, n in zip(range(3), (2, 3, 6)):
            assert q.rg(g, len(c.ref(g, 0, rate).ts))[1] == n
            assert bs.direct_spans(c, g, rate).all()
        flags = []
        for g in range(3, 7):
            spc, n_chunks, tpw, _, _ = q.rg(g, len(c.ref(g, 0, rate).ts))
            assert (spc, n_chunks, tpw) == (16, 3, 1)
            d = bs.direct_spans(c, g, rate)
            flags.append([int((~d[k * spc:(k + 1) * spc]).any()) for k in range(n_chunks)])
            if g == 4:  # only the irregular span needs E
                assert list(np.nonzero(~d)[0]) == [bs.DIRECT_E_SPAN] and bs.DIRECT_E_SPAN // spc == 1
            if g == 6:
                assert not d.any()
        # chunk_e per group: direct only; E in chunk 1 alone; direct only; E everywhere
        assert flags == [[0, 0, 0], [0, 1, 0], [0, 0, 0], [1, 1, 1]]
        # more than 256 spans on direct rows, an int group next to a float one: 18 and 16 chunks with a
        # short last one; one E chunk in the middle of the first, the second direct only
        assert list(q.mode[7:9]) == ([1, 1] if rate else [0, 1])
        for g, chunks, e_chunks in ((7, 18, [bs.DIRECT_BIG_E_SPAN // 17]), (8, 16, [])):
            nk = int(q.nk[g])
            assert nk > bs.GROUP_THREADS and (nk + 255) // 256 == 2
            spc, n_chunks, tpw, _, _ = q.rg(g, len(c.ref(g, 0, rate).ts))
            assert (spc, n_chunks, tpw) == (17, chunks, 1)
            assert chunk_sizes(nk, spc, n_chunks)[-1] < spc
            d = bs.direct_spans(c, g, rate)
            e = [k for k in range(n_chunks) if (~d[k * spc:(k + 1) * spc]).any()]
            assert e == e_chunks and all(0 < k < n_chunks - 1 for k in e)
        for agg in AGGS:
            assert all(c.ref(g, agg, rate).code == 0 for g in range(c.G))


# ---- C: many groups ----
@pytest.mark.parametrize("G", [257, 65537])
def test_many_groups_regime(G):
    c = bs.many_groups(G)
    m = c.meta
    q = bs.geom(c)
    assert c.G == G and not q.wide
    if G > bs.STATS_BLOCKS:
        assert m["three"] == (bs.STATS_BLOCKS - 1, bs.STATS_BLOCKS)  # either side of the stride's turn
    assert G > bs.GROUP_THREADS  # k_group_init / k_group_T: more than one block
    sizes = np.diff(c.gss.astype(np.int64))
    assert sizes[0] == 0 and (sizes[list(m["empty"])] == 0).all()
    e = sorted(m["empty"])
    assert e[2] == e[1] + 1  # two empty groups in a row
    assert (sizes[list(m["three"])] == 3).all() and (sizes[m["dual"]] == 2).all()
    assert (q.nk[m["before"]] == 0).all() and (q.nk[m["after"]] == 0).all()
    assert (q.nk[m["straddle"]] == 1).all()
    for g in m["straddle"]:
        o = c.ref(int(g), 0)
        assert o.code == 0 and len(o.ts) == 0 and o.n_input_points == 2  # nk > 0, T = 0
    for g in list(m["before"]) + list(m["after"]) + list(m["empty"]):
        o = c.ref(int(g), 0)
        assert o.code == 0 and len(o.ts) == 0 and o.n_input_points == 0
    for g in m["three"]:
        o = c.ref(int(g), 0)
        assert o.code == 0 and len(o.ts) > 6  # interpolating: more grid points than a span has
    # the integer, float and dual lists are each non-contiguous
    for mode in (0, 1, 2):
        idx = np.nonzero((q.mode == mode) & (q.nk > 0) & (c.meta["role"] != 6))[0]
        assert len(idx) > 2 and (np.diff(idx) > 1).any()
    assert (q.mode[m["dual"]] == 2).all()
    # the closed form of the plain groups against the oracle on a sample
    g, ts, isint, bits = bs.plain_expect(c)
    assert len(g) > G * 0.8
    pick = np.random.default_rng(5).choice(len(g), 200, replace=False)
    for agg in (0, 4):
        for i in pick[:200 if agg == 0 else 20]:
            o = c.ref(int(g[i]), agg)
            assert o.code == 0 and o.n_input_points == 1 and list(o.ts) == [ts[i]]
            assert list(o.is_int) == [isint[i]] and list(o.bits) == [0 if agg == 4 else bits[i]]
    assert (c.capacities() >= 1).all()


# ---- D: bitmap words ----
@pytest.mark.parametrize("mono", [False, True])
def test_word_edges_regime(mono):
    c = bs.word_edges(mono)
    q = bs.geom(c)
    n = len(bs.EDGE_RANGES)
    assert list(q.hi[:n] - q.lo[:n] + 1) == list(bs.EDGE_RANGES) == [1, 31, 32, 33, 64]
    assert list(q.nw[:n]) == [1, 1, 1, 2, 2]
    pad = q.wbase + q.nw
    assert pad[n] == bs.RANK_BLOCK - 1            # a pad word that ends a rank block
    assert q.wbase[n + 1] == bs.RANK_BLOCK and q.hi[n + 1] - q.lo[n + 1] + 1 == 1024 * 32
    assert pad[n + 1] == 2 * bs.RANK_BLOCK        # a pad word that starts one
    g = n + 2
    edge = 3 * bs.RANK_BLOCK
    assert q.wbase[g] < edge < pad[g]             # a bitmap across a block edge, points on both sides
    w = q.wbase[g] + (c.ref(g, 0).ts - q.lo[g]) // 32
    assert (w == edge - 1).any() and (w == edge).any()
    assert all(c.ref(k, a).code == 0 for k in range(c.G) for a in AGGS)


@pytest.mark.parametrize("mono", [False, True])
def test_sparse_words_regime(mono):
    c = bs.sparse_words(mono)
    q = bs.geom(c)
    assert q.W > 262144 and q.nb > bs.SCAN_BLOCKS and not q.wide
    # set bits past rank block 256 (their ranks need the scan's carry): the third group has points
    # on both sides of word 262 144 and the last group lies wholly beyond it
    turn = bs.SCAN_BLOCKS * bs.RANK_BLOCK
    w = q.wbase[2] + (c.ref(2, 0).ts - q.lo[2]) // 32
    assert (w < turn).sum() > 10 and (w >= turn).sum() > 10
    assert q.wbase[3] >= turn and len(c.ref(3, 0).ts) > 0
    assert all(200 < len(c.ref(g, 0).ts) < 400 for g in range(3))
    assert q.nk[3] == 2 and len(c.ref(3, 0).ts) > 41
    assert all(c.ref(k, a).code == 0 for k in range(c.G) for a in AGGS)


# ---- E: the wide-range fallback ----
def test_wide_regime():
    c = bs.wide_fallback()
    q = bs.geom(c)
    assert q.wide and q.W * 32 >= 1 << 32 and (q.hi - q.lo + 1)[[0, 2]].sum() >= 1 << 32
    assert q.nk[1] == 2 and all(c.ref(g, a).code == 0 for g in range(3) for a in AGGS)
    s = bs.wide_segmented()
    q = bs.geom(s)
    assert not q.wide and q.W == (1 << 27) - 1  # one more word and W * 32 reaches 2^32
    assert all(s.ref(g, a).code == 0 for g in range(3) for a in AGGS)
    assert not bs.geom(bs.ordinary()).wide


# ---- F: per-group capacity ----
@pytest.mark.parametrize("lazy", [False, True])
def test_capacity_regime(lazy):
    c = bs.capacity_groups(lazy)
    clean = bs.capacity_groups(False)
    assert c.G == 6 and 0 < bs.CAP_SHORT < bs.CAP_EXACT < 5
    for agg in AGGS:
        T = len(clean.ref(bs.CAP_SHORT, agg).ts)
        assert T >= 8 and all(c.capacities()[g] >= len(clean.ref(g, agg).ts) for g in range(6))
        o = c.ref(bs.CAP_SHORT, agg, capacity=T - 1)
        if lazy:  # the lazy error's index fits the capacity: it wins
            assert o.code == _abi.E_ILLEGAL_DATA and 0 <= o.err_index == len(o.ts) < T - 1
        else:
            assert o.code == _abi.E_CAPACITY
        Te = len(c.ref(bs.CAP_EXACT, agg).ts)
        assert c.ref(bs.CAP_EXACT, agg, capacity=Te).code == 0
        for g in range(6):
            if g != bs.CAP_SHORT:
                assert c.ref(g, agg).code == 0
