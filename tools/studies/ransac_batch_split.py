#!/usr/bin/env python3
"""Study: where a bounded RANSAC batch's GPU time goes.  Reads the kernel trace (and, if given, the memory-copy trace) that
`rocprofv3 --kernel-trace --memory-copy-trace --output-format csv` wrote for `bench.py`, keeps the last RANSAC call (from its
last k_gather_pq on) and prints, per batch (one k_ransac_hypotheses each), the mean device time of every kernel group and the
mean wall time between two batches' k_ransac_hypotheses.  A call with bail-out grows its batches late (csrc/ransac_cut.hpp), so the
batches are also grouped by size - read off k_ransac_hypotheses' grid - with a row per kernel (the two scoring dispatches apart) and
the wall per 65,536 hypotheses.
With a copy trace it also prints the batch's path: every kernel of a batch in start order with the idle time in front of it (from
the end of the kernel before it to its start, kernels only: what the compute stream waits), and per host-to-device copy its
duration, the time from the end of the last kernel that started before it to its start, and the time from its end to the start of
the next kernel.  Means over the bounded batches behind the first one (batches 3..n: the second builds the leaves).
    python tools/studies/ransac_batch_split.py [--call K] [--fine-list F --bounded B [--points N]] <kernel_trace.csv> [<memory_copy_trace.csv>]
--call K: the K-th RANSAC call of the trace instead of the last, counted over the k_gather_pq launches as Python indexes a list
(-1, the default, is the last call, -3 the third from the end; tools/studies/ransac_event_gaps.py makes four).
--fine-list F --bounded B: Context.last_ransac_bound()'s counters of the same call - hypotheses put on the fine level's list, hypotheses
bounded.  A trace holds no list lengths, and the counters are sums over the call, so a batch's list is taken as the call's share F / B
of its size; beside k_ransac_bound_fine's time the size rows then give that length, the time per listed hypothesis and its ratio
to the ideal: the list's leaf-pair walks (--points N pairs, default 200,000: ceil(N / 32) fine leaves, two per walk) at the rate of
the same batches' coarse level (every hypothesis over ceil(N / 128) coarse leaves, two per walk)."""
import collections
import csv
import sys

argv = sys.argv[1:]
call = -1                       # which RANSAC call of the trace, counted over its k_gather_pq launches (-1: the last)
fine_total = bounded_total = 0
points = 200000
while argv and argv[0] in ("--call", "--fine-list", "--bounded", "--points"):
    if argv[0] == "--call": call = int(argv[1])
    elif argv[0] == "--fine-list": fine_total = int(argv[1])
    elif argv[0] == "--bounded": bounded_total = int(argv[1])
    else: points = int(argv[1])
    argv = argv[2:]
n_lpairs = ((points + 31) // 32 + 1) // 2          # csrc/ransac.hip: leaf_alloc
n_cpairs = ((points + 127) // 128 + 1) // 2
rows = []
for f in argv:
    for r in csv.DictReader(open(f)):
        name = r.get("Kernel_Name") or ("copy " + r.get("Direction", "?"))
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), name.split("(")[0].split("<")[0].strip(), int(r.get("Grid_Size_X") or r.get("Grid_Size") or 0)))
rows.sort()
gathers = [i for i, r in enumerate(rows) if r[2].endswith("k_gather_pq")]
rows = rows[gathers[call]:gathers[call + 1] if call + 1 < 0 and call + 1 >= -len(gathers) else None]
hyps = [r[0] for r in rows if r[2].endswith("k_ransac_hypotheses")]
slots = [r[3] for r in rows if r[2].endswith("k_ransac_hypotheses")]      # the kernel's threads: the hypothesis slots its batch covers
rows = [r[:3] for r in rows]
nb = len(hyps)
rows = [r for r in rows if r[0] >= hyps[0] or r[2].startswith("copy")]
groups = collections.OrderedDict()
for s, e, n in rows:
    if s < hyps[0]:
        continue
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

# ---- batches of differing size (a call with bail-out grows its batches late: csrc/ransac_cut.hpp).  A batch's size is read off its
# k_ransac_hypotheses' grid - the slots it covers, which is the hypothesis count of every whole batch (the call's first and last
# batch, and the second, which builds the leaves, are left out).  Per size: the mean time of every kernel per batch, the wall from
# one k_ransac_hypotheses to the next, and that wall per 65,536 hypotheses.
if nb > 4 and any(slots):
    by_size = collections.OrderedDict()
    for b in range(2, nb - 1):
        by_size.setdefault(slots[b], []).append(b)
    kern = [r for r in rows if not r[2].startswith("copy") and r[0] >= hyps[0]]
    for size, bs in by_size.items():
        per = collections.OrderedDict()
        for b in bs:
            seen = collections.Counter()
            for s0, e0, n0 in kern:
                if hyps[b] <= s0 < hyps[b + 1]:
                    name = n0.split("::")[-1]
                    seen[name] += 1                              # k_ransac_score_fast runs twice per batch: phase 1, phase 2
                    per.setdefault("%s #%d" % (name, seen[name]), []).append(e0 - s0)
        walls_b = [hyps[b + 1] - hyps[b] for b in bs]
        wall = sum(walls_b) / len(walls_b) / 1e3
        # (slots, not hypotheses: a batch cut short by the call's end covers the slots of a batch of 65,536 at least and would be
        # grouped with those - today that can only be the call's last batch, which is left out)
        print("batches of %d slots (= hypotheses of a whole batch): %d (batches %s), wall %.1f us (min %.1f, max %.1f), per 65,536 hypotheses %.1f us" %
              (size, len(bs), "%d..%d" % (bs[0] + 1, bs[-1] + 1), wall, min(walls_b) / 1e3, max(walls_b) / 1e3, wall * 65536.0 / max(size, 1)))
        for k, v in per.items():
            print("    %-28s %4.1f launches/batch %9.1f us/batch %9.1f us/launch %9.1f us per 65,536" %
                  (k, len(v) / len(bs), sum(v) / len(bs) / 1e3, sum(v) / len(v) / 1e3, sum(v) / len(bs) / 1e3 * 65536.0 / max(size, 1)))
        fine_k, coarse_k = per.get("k_ransac_bound_fine #1"), per.get("k_ransac_bound #1")
        if fine_total and bounded_total and fine_k and coarse_k:
            listed = size * fine_total / bounded_total               # the call's share of a batch of this size
            fine_us, coarse_us = sum(fine_k) / len(bs) / 1e3, sum(coarse_k) / len(bs) / 1e3
            ideal_us = listed * n_lpairs / (size * n_cpairs / coarse_us)
            print("    fine list %.0f hypotheses per batch (%.4f of it): k_ransac_bound_fine %.1f us = %.2f ns per listed hypothesis; at the coarse level's "
                  "%.0f walks/us the list's %d leaf pairs take %.1f us: ratio %.2f" %
                  (listed, fine_total / bounded_total, fine_us, fine_us * 1e3 / listed, size * n_cpairs / coarse_us, n_lpairs, ideal_us, fine_us / ideal_us))


def mean(v):
    return sum(v) / len(v) / 1e3 if v else float("nan")


def spread(v):
    return "%7.1f us (min %.1f, max %.1f, n %d)" % (mean(v), min(v) / 1e3, max(v) / 1e3, len(v)) if v else "      -"


# ---- the batch's path.  A batch = the kernels from one k_ransac_hypotheses up to the next; the copy that feeds a batch is the
# last host-to-device copy that ends before the next k_ransac_hypotheses starts (the parent: it sits in front of that kernel on
# the compute stream; an upload stream: it ran somewhere under the batch before).
if nb > 3:
    kernels = [r for r in rows if not r[2].startswith("copy") and r[0] >= hyps[0]]
    copies = [r for r in rows if r[2].startswith("copy") and "HOST_TO_DEVICE" in r[2].upper().replace(" ", "_")]
    bounds = hyps + [kernels[-1][1] + 1]
    gaps = collections.OrderedDict()        # (position in the batch, kernel) -> idle times in front of it
    durs = collections.OrderedDict()
    walls, idles = [], []
    for b in range(2, nb - 1):              # batch b's kernels and the gap in front of batch b + 1's first kernel
        ks = [r for r in kernels if bounds[b] <= r[0] < bounds[b + 1]]
        nxt = [r for r in kernels if r[0] >= bounds[b + 1]][:1]
        idle = 0
        for pos, (prev, cur) in enumerate(zip(ks, ks[1:] + nxt)):
            key = (pos, prev[2].split("::")[-1], cur[2].split("::")[-1])
            gaps.setdefault(key, []).append(cur[0] - prev[1])
            durs.setdefault((pos, prev[2].split("::")[-1]), []).append(prev[1] - prev[0])
            idle += max(0, cur[0] - prev[1])
        walls.append(bounds[b + 1] - bounds[b]); idles.append(idle)
    print("the path of a bounded batch, batches 3..%d (kernel, its time, the idle time behind it up to the next kernel):" % (nb - 1))
    for (pos, a, c), v in gaps.items():
        print("  %2d %-24s %s   then idle %s -> %s" % (pos, a, spread(durs[(pos, a)]), spread(v), c))
    print("  wall %s, no kernel running %s" % (spread(walls), spread(idles)))
    cd, before, after, lead = [], [], [], []
    for s, e, n in copies:
        if not (hyps[2] <= e and s < hyps[-1]):
            continue
        prev_end = max([r[1] for r in kernels if r[0] <= s] or [s])
        nxt_h = [h for h in hyps if h >= e]
        nxt_k = [r[0] for r in kernels if r[0] >= e]
        cd.append(e - s); before.append(s - prev_end)
        if nxt_k: after.append(nxt_k[0] - e)
        if nxt_h: lead.append(nxt_h[0] - e)
    print("host-to-device copies inside the call behind batch 2: %d" % len(cd))
    print("  duration                                   %s" % spread(cd))
    print("  from the end of the last kernel started before it to its start (negative: a kernel is running) %s" % spread(before))
    print("  from its end to the next kernel's start    %s" % spread(after))
    print("  from its end to the next k_ransac_hypotheses %s" % spread(lead))
