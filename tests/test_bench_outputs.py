"""bench.py --dump-outputs / --full: the helpers that turn a result into float
arrays (CPU), and on the GPU one small plain run whose dumped points are
checked bit for bit against the oracle on the same (seeded) input."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from opentsdb_amd import _abi, synth  # noqa: E402


def test_sample_index_is_fixed_and_sorted():
    assert bench.sample_index(10, 10, 1) is None
    a, b = bench.sample_index(1000, 100, 7), bench.sample_index(1000, 100, 7)
    assert np.array_equal(a, b) and len(a) == 100 and len(set(a.tolist())) == 100
    assert np.all(np.diff(a) > 0) and a.min() >= 0 and a.max() < 1000


def test_point_arrays_keep_every_bit():
    ts = np.array([10, 20, 30, 40], np.int64)
    isi = np.array([1, 0, 1, 0], np.uint8)
    vals = [(1 << 62) + 12345, 0.1, -3, -2.5e300]
    bits = np.array([v if i else np.float64(v).view(np.int64) for v, i in zip(vals, isi)], np.int64)
    d = bench.point_arrays(ts, isi, bits)
    assert {k: v.dtype for k, v in d.items()} == {
        "ts": np.float64, "is_int": np.float32, "value": np.float64, "value_bits_hi32": np.float64,
        "value_bits_lo32": np.float64}
    assert d["ts"].tolist() == [10, 20, 30, 40] and d["is_int"].tolist() == [1, 0, 1, 0]
    assert d["value"].tolist() == [float((1 << 62) + 12345), 0.1, -3.0, -2.5e300]
    back = (d["value_bits_hi32"].astype(np.uint64) << np.uint64(32)) | d["value_bits_lo32"].astype(np.uint64)
    assert np.array_equal(back.view(np.int64), bits)
    idx = np.array([1, 3])
    assert bench.point_arrays(ts, isi, bits, idx)["value"].tolist() == [0.1, -2.5e300]


def test_dump_outputs_writes_float_npy_within_the_budget(tmp_path, monkeypatch):
    d = tmp_path / "out"
    bench.dump_outputs(str(d), {"a": np.arange(5, dtype=np.float64), "b": np.ones(3, np.float32)})
    assert sorted(os.listdir(d)) == ["a.npy", "b.npy"]
    assert np.load(d / "a.npy").tolist() == [0, 1, 2, 3, 4] and np.load(d / "b.npy").dtype == np.float32
    with pytest.raises(TypeError):
        bench.dump_outputs(str(d), {"c": np.arange(5)})
    monkeypatch.setattr(bench, "DUMP_BUDGET", 16)
    with pytest.raises(ValueError):
        bench.dump_outputs(str(d), {"a": np.zeros(2), "b": np.zeros(1)})


@pytest.mark.gpu
def test_plain_run_dumps_the_last_steps_points(tmp_path):
    """A plain run (C1 shape, 37 series): --steps sets the timed steps, the
    line carries none of the --full legs, and the dumped points are the
    oracle's on the same input (the device generator is synth.regular)."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle
    out = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "c1", "--series", "37",
           "--steps", "2", "--warmup", "1", "--dump-outputs", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["steps"] == 2 and d["ms_per_step"] > 0 and d["value"] > 0 and d["unit"] == "input points/s"
    assert d["higher_is_better"] is True and d["dtype"] == "int64" and d["metric"] == bench.METRIC
    assert "cpu_baseline" not in d and d["roofline"]["achievable_GBs"] == {}
    files = sorted(os.listdir(out))
    assert files == ["counts.npy", "is_int.npy", "ts.npy", "value.npy", "value_bits_hi32.npy",
                     "value_bits_lo32.npy"]
    a = {f[:-4]: np.load(out / f) for f in files}
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 * 1000 * 1000
    ss = synth.regular(37, 3600, _abi.SYN_INT64_COUNTER, seed=3, step=1)
    o = oracle.spangroup(ss, 0, (1 << 32) - 1, _abi.AGG_SUM)
    assert o.code == 0 and a["counts"].tolist() == [len(o.ts), o.n_input_points] == [3600, 37 * 3600]
    assert np.array_equal(a["ts"], o.ts.astype(np.float64)) and np.array_equal(a["is_int"], o.is_int)
    bits = (a["value_bits_hi32"].astype(np.uint64) << np.uint64(32)) | a["value_bits_lo32"].astype(np.uint64)
    assert np.array_equal(bits.view(np.int64), o.bits)
    assert np.array_equal(a["value"], o.bits.astype(np.float64))
