#!/usr/bin/env python3
"""Timeline of the headline step from a rocprofv3 --kernel-trace CSV: does the serialization of step N
overlap the plan / compute kernels of step N + 1?

  python scripts/overlap_trace.py <dir or kernel_trace.csv> [steps]

Takes the last `steps` (default 50) launches of k_pair_cu<AND> with the k_plan_balanced in front of each
and the k_serialize_agg that follows it, and prints, in microseconds: the mean duration of each kernel, the
period between compute starts (the step), how long serialization N runs together with plan or compute N + 1,
the idle time between one compute kernel's end and the next one's start, and the queues the kernels ran on.
"""
import csv
import glob
import os
import sys
from statistics import mean


def rows_of(path):
    if os.path.isdir(path):
        hits = sorted(glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True))
        if not hits:
            sys.exit(f"no *kernel_trace.csv under {path}")
        path = hits[-1]
    with open(path) as f:
        return [r for r in csv.DictReader(f)]


def main():
    rows = rows_of(sys.argv[1])
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 50
    ev = []
    for r in rows:
        n = r["Kernel_Name"]
        kind = "pair" if "k_pair_cu" in n else "plan" if "k_plan_balanced" in n else "ser" if "k_serialize_agg" in n else None
        if kind:
            ev.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), kind, r.get("Queue_Id", "?")))
    ev.sort()
    pairs = [i for i, e in enumerate(ev) if e[2] == "pair"]
    pairs = pairs[-(steps + 1):]
    us = lambda ns: ns / 1e3
    dur = {"plan": [], "pair": [], "ser": []}
    period, overlap, idle, ser_lag = [], [], [], []
    queues = {"plan": set(), "pair": set(), "ser": set()}
    for a, b in zip(pairs, pairs[1:]):
        p0, p1 = ev[a], ev[b]
        period.append(us(p1[0] - p0[0]))
        idle.append(us(max(0, p1[0] - p0[1])))
        dur["pair"].append(us(p0[1] - p0[0]))
        queues["pair"].add(p0[3])
        # the serialization that belongs to compute a: the first one that starts at or after its end
        ser = next((e for e in ev[a + 1:] if e[2] == "ser" and e[0] >= p0[1]), None)
        plan = next((e for e in ev[a + 1:b + 1] if e[2] == "plan"), None)
        if plan:
            dur["plan"].append(us(plan[1] - plan[0]))
            queues["plan"].add(plan[3])
        if ser:
            dur["ser"].append(us(ser[1] - ser[0]))
            queues["ser"].add(ser[3])
            ser_lag.append(us(ser[0] - p0[1]))
            nxt0 = plan[0] if plan else p1[0]
            overlap.append(us(max(0, min(ser[1], p1[1]) - max(ser[0], nxt0))))
    print(f"steps {len(period)}")
    for k in ("plan", "pair", "ser"):
        if dur[k]:
            print(f"  {k:5s} mean {mean(dur[k]):8.1f} us   queues {sorted(queues[k])}")
    print(f"  step period (compute start to compute start)        {mean(period):8.1f} us")
    print(f"  compute N end -> serialization N start              {mean(ser_lag) if ser_lag else 0:8.1f} us")
    print(f"  serialization N running with plan / compute N + 1   {mean(overlap) if overlap else 0:8.1f} us")
    print(f"  compute N end -> compute N + 1 start                {mean(idle):8.1f} us")


if __name__ == "__main__":
    main()
