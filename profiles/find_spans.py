"""Measures tsdbhip_find_spans on device-resident scans beside the host
restatement core.find_spans.

Series: 1M row keys of 4 tags (3-byte UIDs): tag 1 has 1M distinct values,
tag 2 has 1,000 values, tags 3 and 4 are constant (the keys of
profiles/groupby_plan.py). Workloads, all TSDBHIP_DESC_DEVICE with the four
cell arrays and a row_status array:

  - 1M series x 1 hour (1M rows) and 1M series x 4 hours (4M rows) in HBase
    order (base time, then tags);
  - the same two with the rows shuffled.

Per workload: --warmup calls, then the median / min / max of --calls calls of
total_ms and hot_ms (HIP events, tsdbhip_timing), n_grid, and the host's wall
clock around the call; the result is checked against numpy (a stable argsort
of the rows' series). core.find_spans runs once per HBase-order workload.
--bench-json: a file holding bench.py's result line from the same session on the same GPU;
its ms_per_step (the C3* query step the call feeds) is recorded with the
fraction of it each workload costs. Writes profiles/find_spans.json.

    python profiles/find_spans.py [--series 1000000] [--calls 15] [--bench-json PATH] [--out PATH]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from opentsdb_amd import _abi, core  # noqa: E402
from opentsdb_amd._lib import Context  # noqa: E402

T0 = 1356998400
KLEN = 31


def series_keys(n, n_values, seed):
    """[n, 31] bytes: metric(3) base_time(4, zero) (1, i) (2, v) (3, 7) (4, 7)"""
    rng = np.random.default_rng(seed)
    k = np.zeros((n, KLEN), np.uint8)
    k[:, 2] = 9

    def put(col, name, values):
        k[:, col + 2] = name
        v = np.asarray(values, np.uint32)
        k[:, col + 3], k[:, col + 4], k[:, col + 5] = (v >> 16) & 0xFF, (v >> 8) & 0xFF, v & 0xFF

    put(7, 1, np.arange(n))
    put(13, 2, rng.integers(0, n_values, n))
    put(19, 3, np.full(n, 7))
    put(25, 4, np.full(n, 7))
    return k


def scan_keys(series, hours):
    """the rows in HBase order: hour by hour, the series in key order; -> ([rows, 31] keys, series of each row)"""
    n = len(series)
    keys = np.tile(series, (hours, 1))
    for h in range(hours):
        keys[h * n:(h + 1) * n, 3:7] = np.frombuffer((T0 + 3600 * h).to_bytes(4, "big"), np.uint8)
    return keys, np.tile(np.arange(n, dtype=np.int64), hours)


def med(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def run_workload(ctx, torch, name, keys, sid, n_series, warmup, calls, host_model):
    dev = torch.device("cuda", 0)
    n = len(keys)
    key_off = np.arange(n + 1, dtype=np.int64) * KLEN
    t_off = torch.from_numpy(key_off).to(dev)
    t_kb = torch.from_numpy(np.ascontiguousarray(keys).reshape(-1)).to(dev)
    t_status = torch.full((n,), _abi.ROW_TRIVIAL, dtype=torch.uint8, device=dev)
    rows = torch.arange(n, dtype=torch.int64, device=dev)
    t_cells = [rows * 7200, torch.full((n,), 7200, dtype=torch.int32, device=dev),
               rows * 28801, torch.full((n,), 28801, dtype=torch.int32, device=dev)]
    sizes = {"row_order": (torch.int32, n), "span_row_start": (torch.int64, n_series + 1), "row_base": (torch.int32, n),
             "row_ncells": (torch.int32, n), "row_qual_off": (torch.int64, n), "row_val_off": (torch.int64, n),
             "row_val_len": (torch.int32, n), "key_off": (torch.int64, n_series + 1),
             "key_bytes": (torch.uint8, n_series * KLEN)}
    t_out = {f: torch.zeros(size, dtype=dt, device=dev) for f, (dt, size) in sizes.items()}
    torch.cuda.synchronize(dev)

    def call():
        return core.run_find_spans(ctx, t_off.data_ptr(), t_kb.data_ptr(), keys[0, :3].tobytes(), t_status.data_ptr(),
                                   [c.data_ptr() for c in t_cells], span_capacity=n_series,
                                   key_capacity=n_series * KLEN, device=True, n_rows=n, key_nbytes=n * KLEN,
                                   outputs={f: t.data_ptr() for f, t in t_out.items()})

    for _ in range(warmup):
        rc, fs = call()
        ctx.check(rc)
    total, hot, wall, t = [], [], [], None
    for _ in range(calls):
        w0 = time.perf_counter()
        rc, fs = call()
        wall.append((time.perf_counter() - w0) * 1e3)
        ctx.check(rc)
        t = ctx.timing()
        total.append(float(t.total_ms))
        hot.append(float(t.hot_ms))
    torch.cuda.synchronize(dev)
    # the result against numpy: spans in series order, rows of a span in delivery order
    assert (fs.n_spans, fs.n_rows, fs.n_skipped, fs.key_used) == (n_series, n, 0, n_series * KLEN)
    order = np.argsort(sid, kind="stable")
    assert np.array_equal(t_out["row_order"].cpu().numpy().view(np.uint32), order.astype(np.uint32))
    counts = np.bincount(sid, minlength=n_series)
    assert np.array_equal(t_out["span_row_start"].cpu().numpy(), np.concatenate([[0], np.cumsum(counts)]))
    first = order[np.concatenate([[0], np.cumsum(counts)[:-1]])]
    assert np.array_equal(t_out["key_bytes"].cpu().numpy().reshape(n_series, KLEN), keys[first])
    res = {"workload": name, "n_rows": n, "n_spans": n_series, "sort_passes_n_grid": int(t.n_grid),
           "alg_bytes": int(t.alg_bytes), "total_ms": med(total), "hot_ms": med(hot), "wall_ms": med(wall)}
    if host_model:
        rows = [(r.tobytes(), i) for i, r in enumerate(keys)]
        w0 = time.perf_counter()
        spans = core.find_spans(rows, keys[0, :3].tobytes())
        res["host_find_spans_s"] = time.perf_counter() - w0
        assert len(spans) == n_series
        res["speedup_vs_host_find_spans"] = res["host_find_spans_s"] * 1e3 / res["total_ms"]["median"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--series", type=int, default=1_000_000)
    ap.add_argument("--values", type=int, default=1000)
    ap.add_argument("--hours", type=int, default=4)
    ap.add_argument("--calls", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--bench-json", default=None)
    ap.add_argument("--only-hours", action="store_true", help="only the --hours workloads, not the 1 h ones")
    ap.add_argument("--no-host-model", action="store_true", help="leave core.find_spans out (kernel traces)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "find_spans.json"))
    a = ap.parse_args()
    import torch

    ctx = Context(0)
    series = series_keys(a.series, a.values, 1)
    rng = np.random.default_rng(2)
    results = []
    for hours in ((a.hours,) if a.only_hours else (1, a.hours)):
        keys, sid = scan_keys(series, hours)
        results.append(run_workload(ctx, torch, f"{a.series} series x {hours} h, HBase order", keys, sid, a.series,
                                    a.warmup, a.calls, host_model=not a.no_host_model))
        p = rng.permutation(len(keys))
        results.append(run_workload(ctx, torch, f"{a.series} series x {hours} h, shuffled", keys[p], sid[p], a.series,
                                    a.warmup, a.calls, host_model=False))
    ctx.close()
    res = {"keys": f"4 tags (3-byte UIDs): {a.series} distinct values, {a.values} values, two constant",
           "workloads": results,
           "method": f"{a.warmup} warm-up calls, then {a.calls} timed calls; device times: HIP events of "
                     "tsdbhip_timing (first kernel .. last kernel, the call's two host round trips included); "
                     "wall_ms: the host's clock around the ctypes call; core.find_spans: one run"}
    if a.bench_json:
        line = [ln for ln in open(a.bench_json).read().splitlines() if ln.startswith("{")][-1]
        b = json.loads(line)
        step = float(b["ms_per_step"])
        res["query_step"] = {"config": (b.get("config") or {}).get("workload"), "ms_per_step": step}
        for r in results:
            r["frac_of_query_step"] = r["total_ms"]["median"] / step
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
