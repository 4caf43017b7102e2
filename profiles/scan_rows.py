"""Measures tsdbhip_scan_rows on a device-resident table, with both key
loaders, beside the existing pass over the same bytes and a flat read.

Table: the 4M-row table of profiles/find_spans.py (1M series x 4 h, 31-byte
keys of 4 tags, HBase order) with a second metric of equal size interleaved
behind it, row by row: 8M rows, with row_status and the four cell arrays.
Key bytes and offsets live in one device buffer. Queries:

  - no filter (every row of the metric);
  - one fixed tag (tag 2 = one of its 1,000 values: 1 row in 1000);
  - a value list of 1,024 ids on tag 1;
  - a time range that selects one hour of the four.

Per query and per scan_rows_load ("lanes", "lds"): --warmup calls, then the
medians of --calls calls of total_ms, hot_ms (k_sr_match; HIP events,
tsdbhip_timing), the host's wall clock around the call, and alg_bytes; the
selection is checked against numpy. Yardsticks, same run, same buffers:

  - k_fs_keys: tsdbhip_find_spans over the same keys, all of one metric (the
    second metric's byte rewritten in a copy), with key_nbytes one more than
    key_off ends at: the call returns after k_fs_keys and its readback, having
    checked and read every key; the host's wall clock around it (an upper
    bound: a launch and a round trip more than the kernel);
  - tsdbhip_bw_probe mode 2, the flat 16-byte read, over key bytes + offsets.

Writes profiles/scan_rows.json.

    python profiles/scan_rows.py [--series 1000000] [--calls 15] [--out PATH]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from find_spans import KLEN, T0, scan_keys, series_keys  # noqa: E402
from opentsdb_amd import _abi, core  # noqa: E402
from opentsdb_amd._lib import Context  # noqa: E402


def b3(i):
    return int(i).to_bytes(3, "big")


def med(xs):
    return statistics.median(xs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--series", type=int, default=1_000_000)
    ap.add_argument("--values", type=int, default=1000)
    ap.add_argument("--hours", type=int, default=4)
    ap.add_argument("--calls", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scan_rows.json"))
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    ctx = Context(0)

    one, _ = scan_keys(series_keys(a.series, a.values, 1), a.hours)
    n1 = len(one)
    keys = np.repeat(one, 2, axis=0)  # row 2 i: the metric, row 2 i + 1: the same key under the next metric
    keys[1::2, 2] += 1
    n = len(keys)
    metric = one[0, :3].tobytes()
    nbytes = n * KLEN
    off_at = (nbytes + 1 + 15) // 16 * 16  # (one spare byte after the keys: the k_fs_keys yardstick claims it)
    both = torch.zeros(off_at + 8 * (n + 1), dtype=torch.uint8, device=dev)
    both[:nbytes] = torch.from_numpy(keys.reshape(-1))
    both[off_at:] = torch.from_numpy((np.arange(n + 1, dtype=np.int64) * KLEN).view(np.uint8))
    same = torch.from_numpy(np.repeat(one, 2, axis=0).reshape(-1)).to(dev)  # the yardstick's keys: one metric
    same = torch.cat([same, torch.zeros(1, dtype=torch.uint8, device=dev)])
    t_status = torch.full((n,), _abi.ROW_TRIVIAL, dtype=torch.uint8, device=dev)
    rows = torch.arange(n, dtype=torch.int64, device=dev)
    t_cells = [rows * 7200, torch.full((n,), 7200, dtype=torch.int32, device=dev),
               rows * 28801, torch.full((n,), 28801, dtype=torch.int32, device=dev)]
    sizes = {"row_index": (torch.int32, n1), "key_off": (torch.int64, n1 + 1), "key_bytes": (torch.uint8, n1 * KLEN),
             "row_status": (torch.uint8, n1), "row_qual_off": (torch.int64, n1), "row_qual_len": (torch.int32, n1),
             "row_val_off": (torch.int64, n1), "row_val_len": (torch.int32, n1)}
    t_out = {f: torch.zeros(size, dtype=dt, device=dev) for f, (dt, size) in sizes.items()}
    torch.cuda.synchronize(dev)
    p_keys, p_off = both.data_ptr(), both.data_ptr() + off_at

    rng = np.random.default_rng(5)
    tag1 = (one[:, 10].astype(np.int64) << 16) | (one[:, 11].astype(np.int64) << 8) | one[:, 12]
    tag2 = (one[:, 16].astype(np.int64) << 16) | (one[:, 17].astype(np.int64) << 8) | one[:, 18]
    hour = np.repeat(np.arange(a.hours), a.series)
    ids = rng.choice(a.series, 1024, replace=False)
    queries = [
        ("no filter", {}, np.ones(n1, bool)),
        ("one fixed tag, 1 row in %d" % a.values, dict(tags=[(b3(2), b3(123))]), tag2 == 123),
        ("a 1024-id value list", dict(group_bys=[b3(1)], group_by_values={b3(1): [b3(i) for i in ids]}),
         np.isin(tag1, ids)),
        # scan_start = T0 + 3600 exactly, scan_stop = T0 + 7199 + 1: the second hour alone
        ("a time range, one hour of %d" % a.hours, dict(start_time=T0 + 3 * 3600, end_time=T0 + 3598), hour == 1),
    ]

    def call(sq):
        return core.run_scan_rows(ctx, p_off, p_keys, metric, sq, t_status.data_ptr(),
                                  [c.data_ptr() for c in t_cells], row_capacity=n1, key_capacity=n1 * KLEN,
                                  device=True, n_rows=n, key_nbytes=nbytes,
                                  outputs={f: t.data_ptr() for f, t in t_out.items()})

    results = []
    for name, q, want in queries:
        sq, keep = core.make_scan_query(q.get("tags"), q.get("group_bys"), q.get("group_by_values"),
                                        q.get("start_time", 0), q.get("end_time"), 0)
        exp = (np.nonzero(want)[0] * 2).astype(np.uint32)
        r = {"query": name, "n_rows": n, "n_selected": int(len(exp))}
        for load in ("lanes", "lds"):
            ctx.set_option("scan_rows_load", load)
            for _ in range(a.warmup):
                rc, sel = call(sq)
                ctx.check(rc)
            total, hot, wall, t = [], [], [], None
            for _ in range(a.calls):
                w0 = time.perf_counter()
                rc, sel = call(sq)
                wall.append((time.perf_counter() - w0) * 1e3)
                ctx.check(rc)
                t = ctx.timing()
                total.append(float(t.total_ms))
                hot.append(float(t.hot_ms))
            torch.cuda.synchronize(dev)
            assert (sel.n_selected, sel.key_used) == (len(exp), len(exp) * KLEN), (name, load, sel.n_selected)
            assert np.array_equal(t_out["row_index"][:len(exp)].cpu().numpy().view(np.uint32), exp), (name, load)
            got_keys = t_out["key_bytes"][:len(exp) * KLEN].cpu().numpy().reshape(-1, KLEN)
            assert np.array_equal(got_keys, keys[exp]), (name, load)
            r[load] = {"total_ms": med(total), "hot_ms": med(hot), "hot_ms_min": min(hot), "hot_ms_max": max(hot),
                       "wall_ms": med(wall), "alg_bytes": int(t.alg_bytes)}
        ctx.set_option("scan_rows_load", "auto")
        results.append(r)

    # ---- yardsticks ----
    outs = {"row_order": (torch.int32, n), "span_row_start": (torch.int64, 2), "row_base": (torch.int32, n),
            "row_ncells": (torch.int32, n), "row_qual_off": (torch.int64, n), "row_val_off": (torch.int64, n),
            "row_val_len": (torch.int32, n), "key_off": (torch.int64, 2), "key_bytes": (torch.uint8, 64)}
    f_out = {f: torch.zeros(size, dtype=dt, device=dev) for f, (dt, size) in outs.items()}
    torch.cuda.synchronize(dev)
    fk = []
    for i in range(a.warmup + a.calls):
        w0 = time.perf_counter()
        rc, _ = core.run_find_spans(ctx, p_off, same.data_ptr(), metric, None, None, span_capacity=1, key_capacity=64,
                                    device=True, n_rows=n, key_nbytes=nbytes + 1,
                                    outputs={f: t.data_ptr() for f, t in f_out.items()})
        if i >= a.warmup:
            fk.append((time.perf_counter() - w0) * 1e3)
        assert rc == _abi.E_INVALID_ARG and "key_off does not end" in ctx.last_error(), ctx.last_error()
    d = _abi.SgDesc()
    d.flags = _abi.DESC_DEVICE
    d.val_bytes = C.cast(C.c_void_p(both.data_ptr()), _abi.P8)
    d.val_nbytes = both.numel()
    flat = []
    for i in range(a.warmup + a.calls):
        ms, nb = C.c_float(), C.c_uint64()
        ctx.check(ctx._lib.tsdbhip_bw_probe(ctx.handle, C.byref(d), 2, 8, C.byref(ms), C.byref(nb)))
        if i >= a.warmup:
            flat.append(float(ms.value))
    ctx.close()
    res = {"table": f"{a.series} series x {a.hours} h x 2 metrics interleaved = {n} rows, {KLEN}-byte keys of 4 tags, "
                    f"{nbytes} key bytes + {8 * (n + 1)} offset bytes in one buffer",
           "queries": results,
           "yardsticks": {"k_fs_keys_call_wall_ms": {"median": med(fk), "min": min(fk), "max": max(fk)},
                          "flat_read_ms": {"median": med(flat), "min": min(flat), "max": max(flat),
                                           "bytes": int(both.numel())}},
           "method": f"{a.warmup} warm-up calls, then the median of {a.calls} timed calls; total_ms / hot_ms: HIP "
                     "events of tsdbhip_timing (hot_ms: k_sr_match alone; total_ms: match, scans, the host round "
                     "trip and the emit); wall_ms: the host's clock around the ctypes call; k_fs_keys: wall clock "
                     "around a tsdbhip_find_spans call that returns after k_fs_keys and its readback; flat read: "
                     "tsdbhip_bw_probe mode 2 (HIP events)"}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
