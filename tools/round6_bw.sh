#!/bin/bash
cd /root/repo; O=gpurun_out/r06bw; mkdir -p $O
timeout 1200 python -m pytest tests/test_windowed_ba_gpu.py tests/test_host_classes_gpu.py tests/test_track_to_batch_gpu.py tests/test_system_gpu.py -x -q -m gpu > $O/t.log 2>&1; tail -3 $O/t.log
VDO_BATCH_TRACE=1 timeout 600 python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-batch --no-host-inputs --no-parity 2>$O/err.txt | python -c "
import json,sys
d=json.loads([l for l in sys.stdin if l.startswith('{')][-1]); print(round(d['value'],1), round(d.get('value_full_sequence',0),1), round(d.get('value_with_windowed_ba',0),1))"
grep "partial batch" $O/err.txt | tail -9
