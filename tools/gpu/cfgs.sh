#!/bin/bash
# On the GPU machine: bench lines of the given configs (with the bandwidth probes, no CPU
# baseline), one JSON each under $OUT_DIR/cfgs/ (default bench_out/cfgs/;
# suffixed _$TAG when TAG is set). Usage: cfgs.sh c3s c2 c1 ...
set -o pipefail
O=${OUT_DIR:-bench_out}/cfgs
mkdir -p $O
for c in "$@"; do
  o=$c${TAG:+_$TAG}
  timeout -k 10 300 python bench.py --config $c --steps 10 --warmup 3 --full --no-cpu > $O/$o.json 2> $O/$o.err || exit 1
  python - "$o" "$O/$o.json" <<'PY'
import json,sys
d=json.load(open(sys.argv[2]))
r=d.get("roofline",{})
print(sys.argv[1], f"{d['value']:.3e}", f"{d['ms_per_step']:.3f}ms", r.get("kernel"), f"{r.get('kernel_ms',0):.3f}ms", f"frac={r.get('frac',0):.3f}", "read_frac=", r.get("frac_of_read_stream"))
PY
done
