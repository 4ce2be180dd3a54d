"""Exact per-step kernel figures from two rocprofv3 --kernel-trace --stats summaries of bench.py that differ only in --steps (same
--warmup): (calls, time) of the longer run minus the shorter one, divided by the difference in steps -- no setup or warm-up in it.
usage: python tools/kernel_stats_diff.py short_kernel_stats.csv long_kernel_stats.csv [steps_difference=20] [rows=60]"""
import csv
import sys


def load(path):
    return {r["Name"]: (int(r["Calls"]), float(r["TotalDurationNs"])) for r in csv.DictReader(open(path))}


a, b = load(sys.argv[1]), load(sys.argv[2])
dn = float(sys.argv[3]) if len(sys.argv) > 3 else 20.0
nrows = int(sys.argv[4]) if len(sys.argv) > 4 else 60
rows = []
for k in set(a) | set(b):
    ca, ta = a.get(k, (0, 0.0))
    cb, tb = b.get(k, (0, 0.0))
    rows.append(((tb - ta) / dn / 1e3, (cb - ca) / dn, k))
rows.sort(reverse=True)
print("per step: kernel time %.3f ms, %.1f launches" % (sum(r[0] for r in rows) / 1e3, sum(r[1] for r in rows)))
print("%10s %8s  %s" % ("us/step", "calls", "kernel"))
for t, c, k in rows[:nrows]:
    if abs(t) < 0.05 and abs(c) < 0.005:
        continue
    print("%10.1f %8.2f  %s" % (t, c, k.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]))
