"""Point-query timings on the C2 operand (65,536 mixed containers, resident), for rocprofv3 --kernel-trace:
2^24 seeded random queries per call through the device entry point, per op ms per call and queries per
second; the rank directory's build time; and, alternating in one run, RANK on uniform against sorted queries.
(The variant without the bitmap directory this script also alternated was removed from the engine; its numbers
are in profiles/point_query/point_perf.txt.)"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from roaringbitmap_amd import Engine  # noqa: E402

N = 1 << 24
WINDOW = 0.5  # seconds, at least, per timed window

eng = Engine(0)
dev = torch.device("cuda", 0)
a = eng.synth(0, 0xC2A0)
st = eng.batch_stats(a)
card = st["cardinality"]
print(f"operand: {st['containers']} containers (A {st['array']} / B {st['bitmap']} / R {st['run']}), "
      f"{st['payload_bytes']} payload bytes, cardinality {card}")


def u32(t):  # int64 values below 2^32 -> uint32 tensor (the low little-endian words)
    return t.contiguous().view(torch.int32)[::2].contiguous().view(torch.uint32)


g = torch.Generator(device=dev)
g.manual_seed(0xC2A0)
xs = torch.randint(0, 1 << 32, (N,), generator=g, device=dev, dtype=torch.int64)
js = torch.randint(0, card, (N,), generator=g, device=dev, dtype=torch.int64)
xs_sorted = torch.sort(xs).values
q_uniform, q_sorted, q_select = u32(xs), u32(xs_sorted), u32(js)
torch.cuda.synchronize()

t0 = time.perf_counter()
eng.point_query("rank", a, q_uniform[:1])
eng.sync()
print(f"first query (rank directory build + 1 query): {(time.perf_counter() - t0) * 1e3:.3f} ms")


def timed(op, q):
    eng.point_query(op, a, q)  # warm-up
    eng.sync()
    reps, dt = 4, 0.0
    while True:
        t0 = time.perf_counter()
        for _ in range(reps):
            eng.point_query(op, a, q)
        eng.sync()
        dt = time.perf_counter() - t0
        if dt >= WINDOW:
            return dt / reps
        reps *= 4


for op in ("rank", "select", "contains", "next", "prev"):
    ms = timed(op, q_select if op == "select" else q_uniform) * 1e3
    print(f"{op}: {ms:.3f} ms per call of {N} queries, {N / ms / 1e6:.2f} G queries/s")

print("RANK variants, alternating (ms per call):")
rows = {"dir uniform": q_uniform, "dir sorted": q_sorted}
got = {k: [] for k in rows}
for rnd in range(3):
    for k, q in rows.items():
        got[k].append(timed("rank", q) * 1e3)
for k, v in got.items():
    print(f"  {k}: " + " ".join(f"{x:.3f}" for x in v))
