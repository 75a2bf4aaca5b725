#!/bin/bash
# tools/job_full.sh OUTDIR: the GPU suite, then the full bench line (--full: host-resident-tiles leg, roofline, CPU baseline) -> OUTDIR
O=${1:?usage: tools/job_full.sh OUTDIR}
mkdir -p $O
timeout 1500 python -m pytest tests -m gpu -x -q > $O/pytest.log 2>&1; echo "pytest rc=$?" >> $O/pytest.log
tail -4 $O/pytest.log
timeout 600 python bench.py --full --steps 10 > $O/bench.json 2> $O/bench.err; python - $O/bench.json <<'PY'
import json, sys
d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
print({k:d[k] for k in ('value','ms_per_step','max_abs_offset_error_px','pairs_failed','attempts_per_step','batches_per_step','value_host_resident_tiles')})
print({k:v['ms_per_launch'] for k,v in d['stages'].items()}); print(d['roofline']['frac'], d['roofline']['valu_issued_over_lower_bound'], d['cpu_baseline']['value'])
PY
