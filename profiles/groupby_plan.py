"""Measures tsdbhip_groupby_plan on 1M row keys beside the host plan.

1M keys of 4 tags: tag 1 has 1M distinct values (so the input, in SpanCmp
order, meets the grouped tag's values in random order), tag 2 has 1,000
values and is grouped by, tags 3 and 4 are constant. Runs

  - the device plan on device-resident keys (TSDBHIP_DESC_DEVICE): warmed,
    then the median of --calls calls, device times from tsdbhip_timing and
    the host's wall clock around the call;
  - the same keys host-resident (the call copies them to HBM first);
  - core.plan_groups on the same keys, once;

checks that the three agree, and writes profiles/groupby_plan.json.

    python profiles/groupby_plan.py [--n 1000000] [--calls 15] [--out PATH]
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

PEAK_GBS = 8000.0  # MI355X HBM3E


def build_keys(n, n_values, seed):
    """[n, 31] bytes: metric(3) base_time(4) (1, i) (2, v) (3, 7) (4, 7), 3-byte UIDs"""
    rng = np.random.default_rng(seed)
    k = np.zeros((n, 31), np.uint8)
    k[:, 2] = 9
    k[:, 3:7] = rng.integers(0, 256, (n, 4), dtype=np.uint8)  # base time: ignored

    def put(col, name, values):
        k[:, col + 2] = name
        v = np.asarray(values, np.uint32)
        k[:, col + 3], k[:, col + 4], k[:, col + 5] = (v >> 16) & 0xFF, (v >> 8) & 0xFF, v & 0xFF

    put(7, 1, np.arange(n))
    put(13, 2, rng.integers(0, n_values, n))
    put(19, 3, np.full(n, 7))
    put(25, 4, np.full(n, 7))
    return k


def med(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def timed_calls(ctx, call, warmup, calls):
    for _ in range(warmup):
        rc, plan = call()
        ctx.check(rc)
    total, hot, wall, t = [], [], [], None
    for _ in range(calls):
        w0 = time.perf_counter()
        rc, plan = call()
        wall.append((time.perf_counter() - w0) * 1e3)
        ctx.check(rc)
        t = ctx.timing()
        total.append(float(t.total_ms))
        hot.append(float(t.hot_ms))
    return plan, t, {"total_ms": med(total), "hot_ms": med(hot), "wall_ms": med(wall)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--values", type=int, default=1000)
    ap.add_argument("--calls", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "groupby_plan.json"))
    a = ap.parse_args()
    import torch

    n = a.n
    keys = build_keys(n, a.values, 1)
    key_off = (np.arange(n + 1, dtype=np.uint64) * np.uint64(keys.shape[1]))
    key_bytes = keys.reshape(-1)
    gbs = [(2).to_bytes(3, "big")]
    ctx = Context(0)
    dev = torch.device("cuda", 0)
    t_off = torch.from_numpy(key_off.view(np.int64)).to(dev)
    t_kb = torch.from_numpy(key_bytes).to(dev)
    torch.cuda.synchronize(dev)

    def on_device():
        return core.run_groupby_plan(ctx, t_off.data_ptr(), t_kb.data_ptr(), gbs, device=True, n_spans=n,
                                     key_nbytes=len(key_bytes))

    def on_host():
        return core.run_groupby_plan(ctx, key_off, key_bytes, gbs)

    dplan, dt, dres = timed_calls(ctx, on_device, a.warmup, a.calls)
    hplan, ht, hres = timed_calls(ctx, on_host, a.warmup, max(10, a.calls))
    key_list = [r.tobytes() for r in keys]
    w0 = time.perf_counter()
    gk, order, gss = core.plan_groups(key_list, gbs)
    host_s = time.perf_counter() - w0
    for p in (dplan, hplan):
        assert p.group_keys == gk and p.group_span_start.tolist() == gss
        assert np.array_equal(p.order, np.asarray(order, np.uint32))
    total = dres["total_ms"]["median"]
    res = {
        "workload": f"{n} row keys x 4 tags (3-byte UIDs), GROUP BY a tag of {a.values} values",
        "n_spans": n, "n_groups": dplan.n_groups, "n_dropped": dplan.n_dropped,
        "live_digit_passes": int(dt.n_grid), "digit_positions": 3,
        "alg_bytes": int(dt.alg_bytes),
        "device_resident": dres,
        "host_resident": dict(hres, h2d_bytes=int(ht.h2d_bytes)),
        "total_ms": total, "hot_ms": dres["hot_ms"]["median"],
        "alg_gbs": dt.alg_bytes / (total * 1e-3) / 1e9 if total > 0 else None,
        "frac_of_peak_8TBs": dt.alg_bytes / (total * 1e-3) / 1e9 / PEAK_GBS if total > 0 else None,
        "host_plan_groups_s": host_s,
        "speedup_vs_host_plan": host_s * 1e3 / total if total > 0 else None,
        "method": f"{a.warmup} warm-up calls, then {a.calls} timed calls (host-resident: {max(10, a.calls)}); "
                  "device times: HIP events of tsdbhip_timing (first kernel .. last kernel, the call's host round "
                  "trip included); wall_ms: the host's clock around the ctypes call; plan_groups: one run",
    }
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
