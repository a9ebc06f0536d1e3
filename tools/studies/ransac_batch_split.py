#!/usr/bin/env python3
"""Study: where a bounded RANSAC batch's GPU time goes.  Reads the kernel trace (and, if given, the memory-copy trace) that
`rocprofv3 --kernel-trace --memory-copy-trace --output-format csv` wrote for `bench.py`, keeps the last RANSAC call (from its
last k_gather_pq on) and prints, per batch (one k_ransac_hypotheses each), the mean device time of every kernel group and the
mean wall time between two batches' k_ransac_hypotheses.
    python tools/studies/ransac_batch_split.py <kernel_trace.csv> [<memory_copy_trace.csv>]"""
import collections
import csv
import sys

rows = []
for f in sys.argv[1:]:
    for r in csv.DictReader(open(f)):
        name = r.get("Kernel_Name") or ("copy " + r.get("Direction", "?"))
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), name.split("(")[0].split("<")[0].strip()))
rows.sort()
gathers = [i for i, r in enumerate(rows) if r[2].endswith("k_gather_pq")]
rows = rows[gathers[-1]:]
hyps = [r[0] for r in rows if r[2].endswith("k_ransac_hypotheses")]
nb = len(hyps)
rows = [r for r in rows if r[0] >= hyps[0]]
groups = collections.OrderedDict()
for s, e, n in rows:
    key = n.split("::")[-1]
    g = groups.setdefault(key, [0, 0])
    g[0] += 1; g[1] += e - s
print("last RANSAC call: %d batches, %.3f ms from the first k_ransac_hypotheses to the last activity" % (nb, (rows[-1][1] - hyps[0]) / 1e6))
if nb > 2:
    print("wall per batch (k_ransac_hypotheses to k_ransac_hypotheses, batches 2..%d): %.1f us" % (nb, (hyps[-1] - hyps[1]) / (nb - 2) / 1e3))
busy = 0
for k, (c, t) in sorted(groups.items(), key=lambda kv: -kv[1][1]):
    print("  %-28s %5d calls %9.1f us/batch %9.1f us/call" % (k, c, t / nb / 1e3, t / c / 1e3))
    busy += t
print("  busy %.1f us/batch" % (busy / nb / 1e3))
