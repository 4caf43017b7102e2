"""Measures tsdbhip_desc_pack with both source loaders, beside the plain
device-to-device copy of the same value bytes, and what the pack buys a query.

Shapes (source rows in tsdbhip_rows_out's placement: row r's qualifiers at the
sum of the qualifier lengths before it, its values at the sum of the value
lengths before it + r, so every value residue mod 16 occurs):

  (a) C3* class: --spans one-row spans of 3600 eight-byte cells (7200 B of
      qualifiers, 28801 B of values a row). If the source, the packed copy and
      the yardstick's destination do not fit, a tenth as many spans, and so on;
  (b) C2 class: 10,000 spans of 24 hourly rows of 360 float cells (720 B,
      1441 B a row);
  (c) small rows: 4,000,000 one-row spans of 6 four-byte cells (12 B, 25 B):
      the copy kernel's lane-per-row path.

The bytes of (a), (b), (c) are a pattern, not cells: a byte copy does not look
at them. Per shape and per desc_pack_load ("unaligned", "shift"): --warmup
calls with order = NULL, then the median (min - max) of --calls calls of
hot_ms (k_pack_copy; HIP events, tsdbhip_timing), total_ms and alg_bytes; rows
of the result are compared with the source. Yardstick, same run, same source
buffers: tsdbhip_bw_probe mode 1, the 16-byte device-to-device copy of the
value bytes. `fraction` is the pack's alg_bytes / hot_ms over mode 1's bytes /
ms. The gate: on (a) the fraction of the loader "auto" picks is at least 0.5.

The payoff: --payoff-spans one-row spans of 3600 eight-byte counters
(tsdbhip_synth_generate, moved to the placement above), the 60-s avg / sum
query over that descriptor (the general path, as on the parent commit: no
SpanGroup kernel differs), the pack, and the same query over the packed
descriptor (the direct aligned group); the two results are compared.

Writes profiles/desc_pack.json.

    python profiles/desc_pack.py [--spans 1000000] [--calls 15] [--out PATH]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from opentsdb_amd import _abi, core, synth  # noqa: E402
from opentsdb_amd._lib import Context  # noqa: E402

U32MAX = (1 << 32) - 1


def stats(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def p8(t, off=0):
    return C.cast(C.c_void_p(t.data_ptr() + off), _abi.P8)


class Foreign:
    """device memory of the library's as a torch tensor (no copy)"""

    def __init__(self, ptr, nbytes):
        self.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 2}


def pattern(torch, dev, nbytes):
    """bytes that differ from their neighbours and from row to row"""
    t = torch.empty(nbytes + 64, dtype=torch.uint8, device=dev)
    step = 1 << 28
    for lo in range(0, nbytes + 64, step):
        hi = min(lo + step, nbytes + 64)
        i = torch.arange(lo, hi, dtype=torch.int64, device=dev)
        t[lo:hi] = ((i * 2654435761) >> 7).to(torch.uint8)
        del i
    return t


def compact_desc(torch, dev, n_spans, rows_per_span, ncells, vlen, qual=None, val=None):
    """a device descriptor of n_spans * rows_per_span equal rows in tsdbhip_rows_out's placement; returns
    (desc, the tensors behind it)"""
    R = n_spans * rows_per_span
    r = torch.arange(R, dtype=torch.int64, device=dev)
    t = {
        "span_row_start": torch.arange(n_spans + 1, dtype=torch.int64, device=dev) * rows_per_span,
        "row_base": (synth.T0 + 3600 * (r % rows_per_span)).to(torch.int32),
        "row_ncells": torch.full((R,), ncells, dtype=torch.int32, device=dev),
        "row_qual_off": r * (2 * ncells),
        "row_val_off": r * (vlen + 1),
        "row_val_len": torch.full((R,), vlen, dtype=torch.int32, device=dev),
    }
    qn, vn = R * 2 * ncells, (R - 1) * (vlen + 1) + vlen
    t["qual_bytes"] = qual if qual is not None else pattern(torch, dev, qn)
    t["val_bytes"] = val if val is not None else pattern(torch, dev, vn)
    d = _abi.SgDesc()
    d.flags = _abi.DESC_DEVICE
    d.n_spans, d.n_rows = n_spans, R
    for f, pt in (("span_row_start", _abi.P64), ("row_base", _abi.P32), ("row_ncells", _abi.P32),
                  ("row_qual_off", _abi.P64), ("row_val_off", _abi.P64), ("row_val_len", _abi.P32)):
        setattr(d, f, C.cast(C.c_void_p(t[f].data_ptr()), pt))
    d.qual_bytes, d.qual_nbytes = p8(t["qual_bytes"]), qn
    d.val_bytes, d.val_nbytes = p8(t["val_bytes"]), vn
    torch.cuda.synchronize(dev)  # (the library's streams do not wait for torch's)
    return d, t


def peek(ctx, d, qo, qlen, vo, vlen):
    """qual_bytes[qo, qo + qlen) and val_bytes[vo, vo + vlen) of a device descriptor, on the host"""
    e = _abi.SgDesc()
    C.pointer(e)[0] = d
    e.n_spans = e.n_rows = 0
    e.qual_bytes = C.cast(C.c_void_p(C.cast(d.qual_bytes, C.c_void_p).value + qo), _abi.P8)
    e.val_bytes = C.cast(C.c_void_p(C.cast(d.val_bytes, C.c_void_p).value + vo), _abi.P8)
    e.qual_nbytes, e.val_nbytes = qlen, vlen
    srs, none = np.zeros(1, np.uint64), np.zeros(1, np.uint64)
    q, v = np.zeros(qlen, np.uint8), np.zeros(vlen, np.uint8)
    ctx.check(ctx._lib.tsdbhip_desc_download(ctx.handle, C.byref(e), *[x.ctypes.data_as(C.c_void_p)
                                                                       for x in (srs, none, none, none, none, none, q, v)]))
    return q, v


def check_rows(ctx, t, out, rows, ncells, vlen):
    """rows of the packed descriptor against the source's; the gap after a row and the slack are zero"""
    qsz, vsz = (2 * ncells + 7) // 8 * 8, (vlen + 15) // 16 * 16
    for r in rows:
        q, v = peek(ctx, out, r * qsz, qsz, r * vsz, vsz)
        sq = t["qual_bytes"][r * 2 * ncells:(r + 1) * 2 * ncells].cpu().numpy()
        sv = t["val_bytes"][r * (vlen + 1):r * (vlen + 1) + vlen].cpu().numpy()
        assert np.array_equal(q[:2 * ncells], sq) and not q[2 * ncells:].any(), r
        assert np.array_equal(v[:vlen], sv) and not v[vlen:].any(), r
    q, v = peek(ctx, out, out.n_rows * qsz, out.qual_nbytes + 64 - out.n_rows * qsz, out.n_rows * vsz,
                out.val_nbytes + 64 - out.n_rows * vsz)
    assert not q.any() and not v.any()


def measure(ctx, torch, dev, name, n_spans, rows_per_span, ncells, vlen, a):
    d, t = compact_desc(torch, dev, n_spans, rows_per_span, ncells, vlen)
    R = n_spans * rows_per_span
    res = {"shape": name, "n_spans": n_spans, "n_rows": R, "qual_bytes_a_row": 2 * ncells, "val_bytes_a_row": vlen,
           "source_bytes": int(d.qual_nbytes + d.val_nbytes)}
    for load in ("unaligned", "shift"):
        ctx.set_option("desc_pack_load", load)
        hot, total, tm = [], [], None
        for i in range(a.warmup + a.calls):
            with core.PackedDesc(ctx, d) as out:
                tm = ctx.timing()
                if i >= a.warmup:
                    hot.append(float(tm.hot_ms))
                    total.append(float(tm.total_ms))
                if i == 0:
                    assert (out.n_spans, out.n_rows) == (n_spans, R)
                    check_rows(ctx, t, out, [0, 1, R // 2, R - 2, R - 1], ncells, vlen)
        res[load] = {"hot_ms": stats(hot), "total_ms": stats(total), "alg_bytes": int(tm.alg_bytes),
                     "alg_GBps": tm.alg_bytes / statistics.median(hot) / 1e6}
    ctx.set_option("desc_pack_load", "auto")
    ms_l, nb = [], C.c_uint64()
    for i in range(a.warmup + a.calls):
        ms = C.c_float()
        ctx.check(ctx._lib.tsdbhip_bw_probe(ctx.handle, C.byref(d), 1, 8, C.byref(ms), C.byref(nb)))
        if i >= a.warmup:
            ms_l.append(float(ms.value))
    copy_rate = nb.value / statistics.median(ms_l) / 1e6
    res["copy_mode1"] = {"ms": stats(ms_l), "bytes": int(nb.value), "GBps": copy_rate}
    for load in ("unaligned", "shift"):
        res[load]["fraction_of_copy"] = res[load]["alg_GBps"] / copy_rate
    del t
    torch.cuda.empty_cache()
    return res


def payoff(ctx, torch, dev, n_spans, a):
    n = 3600
    s = _abi.SgDesc()
    p = _abi.SynthParams(seed=3, n_spans=n_spans, n_points=n, t0=synth.T0, step=1, kind=_abi.SYN_INT64_COUNTER, span0=0)
    ctx.check(ctx._lib.tsdbhip_synth_generate(ctx.handle, C.byref(p), C.byref(s)))
    vstride = s.val_nbytes // n_spans
    sv = torch.as_tensor(Foreign(C.cast(s.val_bytes, C.c_void_p).value, s.val_nbytes), device=dev)
    sq = torch.as_tensor(Foreign(C.cast(s.qual_bytes, C.c_void_p).value, s.qual_nbytes), device=dev)
    tail = torch.zeros(64, dtype=torch.uint8, device=dev)
    val = torch.cat([sv.view(n_spans, vstride)[:, :8 * n + 2].reshape(-1), tail])  # row r at (8 n + 2) r = 28802 r
    qual = torch.cat([sq, tail])
    torch.cuda.synchronize(dev)
    ctx._lib.tsdbhip_synth_free(ctx.handle, C.byref(s))
    d, t = compact_desc(torch, dev, n_spans, 1, n, 8 * n + 1, qual=qual, val=val)
    res = {"n_spans": n_spans, "n_points": n_spans * n}

    def query(desc, calls):
        tot, tm, r = [], None, None
        for i in range(calls):
            r = core.run_spanset(ctx, None, 0, U32MAX, _abi.AGG_SUM, False, 60, _abi.AGG_AVG, device_desc=desc, capacity=4096)
            assert r[0] == 0, ctx.last_error()
            tm = ctx.timing()
            tot.append(float(tm.total_ms))
        return r, stats(tot), int(tm.paths), int(tm.hot_kernel)

    r0, res["query_unpacked_total_ms"], res["query_unpacked_paths"], res["query_unpacked_hot_kernel"] = query(d, 3)
    with core.PackedDesc(ctx, d) as out:
        tm = ctx.timing()
        res["pack"] = {"total_ms": float(tm.total_ms), "hot_ms": float(tm.hot_ms), "alg_bytes": int(tm.alg_bytes)}
        r1, res["query_packed_total_ms"], res["query_packed_paths"], res["query_packed_hot_kernel"] = query(out, a.calls)
    assert r0[4] == r1[4] == n_spans * n
    for x, y in zip(r0[1:4], r1[1:4]):
        assert np.array_equal(x, y)
    res["results_identical"] = True
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spans", type=int, default=1_000_000)
    ap.add_argument("--payoff-spans", type=int, default=100_000)
    ap.add_argument("--shapes", default="abc")
    ap.add_argument("--calls", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "desc_pack.json"))
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    ctx = Context(0)
    shapes = []
    if "a" in a.shapes:
        n = a.spans
        while True:  # (an allocation that does not fit is an error of the call, nothing else)
            try:
                shapes.append(measure(ctx, torch, dev, "a: one-row spans of 3600 eight-byte cells", n, 1, 3600, 28801, a))
                break
            except (core.TsdbHipError, torch.cuda.OutOfMemoryError) as e:
                print(f"(a) with {n} spans did not fit: {str(e)[:200]}", file=sys.stderr)
                if n < 10000:
                    raise
            torch.cuda.empty_cache()
            n //= 10
    if "b" in a.shapes:
        shapes.append(measure(ctx, torch, dev, "b: 10,000 spans of 24 rows of 360 float cells", 10_000, 24, 360, 1441, a))
    if "c" in a.shapes:
        shapes.append(measure(ctx, torch, dev, "c: one-row spans of 6 four-byte cells", 4_000_000, 1, 6, 25, a))
    res = {"shapes": shapes,
           "method": f"{a.warmup} warm-up calls, then the median (min, max) of {a.calls} calls with order = NULL; hot_ms: "
                     "k_pack_copy alone, total_ms: the call (HIP events, tsdbhip_timing); alg_GBps = alg_bytes / hot_ms; "
                     "copy_mode1: tsdbhip_bw_probe mode 1 over the source's value bytes, bytes = read + written; "
                     "fraction_of_copy = alg_GBps / copy GBps"}
    if a.payoff_spans:
        res["payoff"] = payoff(ctx, torch, dev, a.payoff_spans, a)
    res["library"] = os.environ.get("TSDBHIP_LIB", "") or "in-tree"  # (an A/B library: e.g. built with -DTSDBHIP_PACK_NT=1)
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
