"""Anatomy of the timed window of a bench.py run from its rocprofv3 kernel trace: trace launches, how long each lasts, how much
consecutive launches overlap, idle time with no trace kernel running, how long the blends wait, and the hardware queue of every dispatch.
usage: rocprofv3 --kernel-trace --output-format csv -d DIR -o kt -- python3 bench.py --gpus 1 --steps N --warmup 5 --no-extras --secondary none --no-cpu-baseline
       python3 tools/launch_anatomy.py DIR N
The timed window is that of the last N blends (tptResolveKernel: one per delivered frame): it starts where the blend before them ended
(the bench's fence) and ends with the last one."""
import csv
import glob
import os
import sys

d, n = sys.argv[1], int(sys.argv[2])
f = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)[0]
rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"]))
iv = lambda r: (int(r["Start_Timestamp"]), int(r["End_Timestamp"]))  # noqa: E731
res = [r for r in rows if "tptResolveKernel" in r["Kernel_Name"]]
t0, t1 = iv(res[-n - 1])[1], iv(res[-1])[1]
tr = [r for r in rows if ("tptTraceQueueKernel" in r["Kernel_Name"] or "tptFramePoolsKernel" in r["Kernel_Name"]) and iv(r)[0] >= t0]
blends = res[-n:]
span = t1 - t0
durs = [iv(r)[1] - iv(r)[0] for r in tr]
over = [max(0, min(iv(a)[1], iv(b)[1]) - iv(b)[0]) for a, b in zip(tr, tr[1:])]
busy, cur = 0, None  # union of the trace intervals
for s, e in sorted(iv(r) for r in tr):
    if cur and s <= cur[1]:
        cur = (cur[0], max(cur[1], e))
    else:
        if cur:
            busy += cur[1] - cur[0]
        cur = (s, e)
if cur:
    busy += cur[1] - cur[0]
ends = sorted(iv(r)[1] for r in tr)
waits = [iv(b)[0] - max([e for e in ends if e <= iv(b)[0]] or [t0]) for b in blends]
us = lambda v: v / 1e3  # noqa: E731
print("window %.1f us for %d frames: %.1f us per frame" % (us(span), n, us(span) / n))
print("trace launches %d (%.2f frames per launch): duration mean %.1f us, min %.1f, max %.1f; kernels %s" % (
    len(tr), n / max(len(tr), 1), us(sum(durs) / len(durs)), us(min(durs)), us(max(durs)), sorted(set(r["Kernel_Name"].split("(")[0][-30:] for r in tr))))
print("overlap of consecutive launches: mean %.1f us; trace busy %.1f us per frame of %.1f wall (%.1f %%), idle with no trace kernel %.1f us" % (
    us(sum(over) / max(len(over), 1)), us(busy) / n, us(span) / n, 100.0 * busy / span, us(span - busy)))
print("blend: start after the latest trace end before it: mean %.1f us, max %.1f; the last blend ends %.1f us after the last trace" % (
    us(sum(waits) / len(waits)), us(max(waits)), us(t1 - ends[-1])))
print("hardware queues: trace %s, blend %s" % (sorted(set(r["Queue_Id"] for r in tr)), sorted(set(r["Queue_Id"] for r in blends))))
