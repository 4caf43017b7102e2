"""Measures tsdbhip_desc_certify: the price of TSDBHIP_DESC_QUALS_PROVEN.

Shapes (tsdbhip_synth_generate's rows, qualifiers at 0 mod 16):

  (a) C3* class: --spans one-row spans of 3600 eight-byte cells (7200 B of
      qualifiers a row). If it does not fit, a tenth as many spans, and so on;
  (a2) the same qualifier bytes copied two bytes up (every row at 2 mod 16: the
      kernel's loads at the row's own residue);
  (b) C2 class: 10,000 spans of 24 hourly rows of 360 float cells (720 B a row).

Per shape: --warmup calls, then the median (min - max) of --calls calls of
hot_ms (k_desc_certify; HIP events, tsdbhip_timing) and total_ms; GBps is the
rows' qualifier bytes over the median hot_ms. Every call must find no unproven
row and set the flag. Yardstick, same run, shape (a)'s buffers:
tsdbhip_bw_probe mode 7, the non-temporal flat read of the value bytes.

Writes profiles/desc_certify.json.

    python profiles/desc_certify.py [--spans 1000000] [--calls 15] [--out PATH]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from opentsdb_amd import _abi, core, synth  # noqa: E402
from opentsdb_amd._lib import Context  # noqa: E402


def stats(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


class Foreign:
    """device memory of the library's as a torch tensor (no copy)"""

    def __init__(self, ptr, nbytes):
        self.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 2}


def generate(ctx, n_spans, n_points, step, kind):
    d = _abi.SgDesc()
    p = _abi.SynthParams(seed=3, n_spans=n_spans, n_points=n_points, t0=synth.T0, step=step, kind=kind, span0=0)
    ctx.check(ctx._lib.tsdbhip_synth_generate(ctx.handle, C.byref(p), C.byref(d)))
    assert d.flags & _abi.DESC_QUALS_PROVEN  # (the producer's own proof)
    return d


def measure(ctx, name, d, qual_bytes, a):
    hot, total = [], []
    for i in range(a.warmup + a.calls):
        d.flags &= ~_abi.DESC_QUALS_PROVEN
        rc, bad = core.desc_certify(ctx, d)
        assert rc == 0 and bad == 0 and d.flags & _abi.DESC_QUALS_PROVEN, (rc, bad, ctx.last_error())
        tm = ctx.timing()
        if i >= a.warmup:
            hot.append(float(tm.hot_ms))
            total.append(float(tm.total_ms))
    return {"shape": name, "n_rows": int(d.n_rows), "qual_bytes": int(qual_bytes), "hot_ms": stats(hot),
            "total_ms": stats(total), "GBps": qual_bytes / statistics.median(hot) / 1e6}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spans", type=int, default=1_000_000)
    ap.add_argument("--calls", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "desc_certify.json"))
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    ctx = Context(0)
    shapes = []
    n = a.spans
    while True:  # (an allocation that does not fit is an error of the call, nothing else)
        try:
            d = generate(ctx, n, 3600, 1, _abi.SYN_INT64_COUNTER)
            break
        except core.TsdbHipError as e:
            print(f"(a) with {n} spans did not fit: {str(e)[:200]}", file=sys.stderr)
            if n < 10000:
                raise
        n //= 10
    shapes.append(measure(ctx, "a: one-row spans of 3600 eight-byte cells", d, 7200 * n, a))
    ms_l, nb = [], C.c_uint64()
    for i in range(a.warmup + a.calls):
        ms = C.c_float()
        ctx.check(ctx._lib.tsdbhip_bw_probe(ctx.handle, C.byref(d), 7, 8, C.byref(ms), C.byref(nb)))
        if i >= a.warmup:
            ms_l.append(float(ms.value))
    probe = {"ms": stats(ms_l), "bytes": int(nb.value), "GBps": nb.value / statistics.median(ms_l) / 1e6}
    # (a2) the qualifiers two bytes up
    sq = torch.as_tensor(Foreign(C.cast(d.qual_bytes, C.c_void_p).value, d.qual_nbytes), device=dev)
    up = torch.zeros(d.qual_nbytes + 2 + 64, dtype=torch.uint8, device=dev)
    up[2:2 + d.qual_nbytes] = sq
    torch.cuda.synchronize(dev)
    e = _abi.SgDesc()
    C.pointer(e)[0] = d
    e.qual_bytes = C.cast(C.c_void_p(up.data_ptr() + 2), _abi.P8)  # (the same offsets from a base at 2 mod 16)
    shapes.append(measure(ctx, "a2: the same rows at 2 mod 16", e, 7200 * n, a))
    del up, sq
    torch.cuda.empty_cache()
    ctx._lib.tsdbhip_synth_free(ctx.handle, C.byref(d))
    d = generate(ctx, 10_000, 8640, 10, _abi.SYN_FLOAT32)
    shapes.append(measure(ctx, "b: 10,000 spans of 24 rows of 360 float cells", d, 720 * int(d.n_rows), a))
    ctx._lib.tsdbhip_synth_free(ctx.handle, C.byref(d))
    for s in shapes:
        s["fraction_of_mode7"] = s["GBps"] / probe["GBps"]
    res = {"shapes": shapes, "flat_read_nt_mode7": probe,
           "method": f"{a.warmup} warm-up calls, then the median (min, max) of {a.calls} calls; hot_ms: k_desc_certify "
                     "alone, total_ms: the call (HIP events, tsdbhip_timing); GBps = the rows' qualifier bytes / hot_ms; "
                     "flat_read_nt_mode7: tsdbhip_bw_probe mode 7 over shape (a)'s value bytes"}
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
