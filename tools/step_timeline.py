#!/usr/bin/env python3
"""One engine step of a rocprofv3 --kernel-trace CSV, launch by launch (start us, duration us, idle gap before, kernel), and the
three intervals of its DP stage: k_walk end -> sweep start, the sweep, sweep end -> k_assemble start.
usage: step_timeline.py <kernel_trace.csv> [step_index]"""
import csv
import sys

rows = list(csv.DictReader(open(sys.argv[1])))
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
ev = [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"].split("(")[0].replace("void ", "").replace("psvr::", "")) for r in rows]
# a step begins with k_run_init; the last complete one by default
starts = [i for i, e in enumerate(ev) if e[2].startswith("k_run_init")]
k = int(sys.argv[2]) if len(sys.argv) > 2 else len(starts) - 2
a, b = starts[k], starts[k + 1]
t0 = ev[a][0]
end = t0
for s, e, n in ev[a:b]:
    print("%9.1f %8.1f gap %7.1f  %s" % ((s - t0) / 1e3, (e - s) / 1e3, (s - end) / 1e3, n))
    end = max(end, e)
print("# next step starts at %.1f us" % ((ev[b][0] - t0) / 1e3))
step = ev[a:b]
walk = next(i for i, e in enumerate(step) if e[2] == "k_walk")
sweep = next((i for i, e in enumerate(step) if i > walk and e[2].startswith("extd2_team_kernel")), None)
asm = next(i for i, e in enumerate(step) if i > walk and e[2] == "k_assemble")
if sweep is not None:
    between = step[walk + 1:sweep]
    print("# k_walk end -> sweep start %.1f us (%d launches, %d idle gaps over 5 us: the host waits), sweep %.1f us, sweep end -> k_assemble start %.1f us" % (
        (step[sweep][0] - step[walk][1]) / 1e3, len(between), sum(1 for i in range(walk + 1, sweep + 1) if step[i][0] - max(e[1] for e in step[:i]) > 5000),
        (step[sweep][1] - step[sweep][0]) / 1e3, (step[asm][0] - step[sweep][1]) / 1e3))
