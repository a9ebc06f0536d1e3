#!/usr/bin/env python3
"""Study: host time of RANSAC's index draw for one batch of bench.py's workload.  Times tdv_sample_triples(seed, n, count) - the
same stream the batch loop of ransac_run_dev draws from - and prints the median and the range over the repetitions, in ms.
Needs no GPU.    python tools/studies/ransac_host_draw_probe.py [n=200000] [count=65536] [reps=50]"""
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
tdv = importlib.import_module("3dvision_amd")

n = int(sys.argv[1]) if len(sys.argv) > 1 else 200000
count = int(sys.argv[2]) if len(sys.argv) > 2 else 65536
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 50
out = np.empty((count, 3), np.uint64)
fn = tdv.lib().tdv_sample_triples
import ctypes as C
ptr = out.ctypes.data_as(C.c_void_p)
ts = []
for r in range(reps + 3):
    t0 = time.perf_counter()
    fn(C.c_uint32(42 + r), C.c_uint64(n), count, ptr)
    ts.append((time.perf_counter() - t0) * 1e3)
ts = sorted(ts[3:])
print("tdv_sample_triples(n=%d, count=%d): median %.3f ms, range %.3f-%.3f ms over %d calls" % (n, count, ts[len(ts) // 2], ts[0], ts[-1], reps))
