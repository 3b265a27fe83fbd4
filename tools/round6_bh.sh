#!/bin/bash
cd /root/repo; O=gpurun_out/r06bh; mkdir -p $O
timeout 900 python -m pytest tests/test_ba_gpu.py -x -q -m gpu -k "small_reduced or dense_mfma or static_only or non_path" > $O/t1.log 2>&1; tail -3 $O/t1.log
timeout 900 python -m pytest tests/test_windowed_ba_gpu.py tests/test_host_classes_gpu.py tests/test_track_to_batch_gpu.py -x -q -m gpu > $O/t2.log 2>&1; tail -3 $O/t2.log
for i in 1 2 3; do
VDO_BATCH_TRACE=1 timeout 600 python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-batch --no-host-inputs --no-parity 2>$O/err.txt | python -c "
import json,sys
d=json.loads([l for l in sys.stdin if l.startswith('{')][-1]); print(round(d['value'],1), round(d.get('value_full_sequence',0),1), round(d.get('value_with_windowed_ba',0),1))" | tee -a $O/ab.txt
grep "^\[batch\]" $O/err.txt | tail -2 | cut -c1-120
done
