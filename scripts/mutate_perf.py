"""Batches of values added to or removed from a resident bitmap on the device, timed
(profiles/mutate/mutate_perf.txt).

Operands (Engine.from_values):
  dense256    three values of every four below 2^24 (low & 3 != 3): 256 keys of bitmap containers of 49,152
              values, run-free.  (Not arange(2^24): its containers are full, an add changes nothing and the
              yardstick's or turns every one into RunContainer.full(), so no add row could be byte-checked.)
  sparse64k   2^24 values, 256 in each of the 65,536 keys (stride 256): array containers, run-free
  runs512     2^24 values in runs of 64 values every 128, run-optimized: 512 keys of run containers (512 runs each)
Deltas of 2^10, 2^16 and 2^20 uniform random values as device tensors, in two shapes:
  clustered   inside 8 neighbouring keys in the middle of the operand's keys
  scattered   over every key of the operand and (where there is room) as many keys above it
Both ops.  Timed: ms per Engine.mutate_values + release (csrc/mutate.hip), a host clock around calls that end in
a synchronise, windows of at least 0.25 s, three rounds alternating with the yardstick, medians and the spread
between rounds.  Yardstick: the only route that exists without the call -- Engine.from_values(delta), the
pairwise or / andNot of the two resident batches, its result fetched and loaded as a batch -- in the same
process on the same input.  On the run-free operands its bytes are asserted equal to the call's once per row;
on runs512 they differ by design (RunContainer.or(ArrayContainer) goes through toEfficientContainer,
RunContainer.add returns this) and only the time is reported.  Most of the yardstick's time is the round
trip that makes its result a batch (device to host, host to device, decode), not the or / andNot kernel.
cells: the touched keys, one 8 KiB cell each.  model MB: the launch table's bytes: the values
read twice, three passes over the cells, the operand's payload read once and the result's written once, as an
upper bound (a touched key's source container is read in place of copied).
Arguments: [largest log2 n of a delta] [operands, comma separated]."""
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from roaringbitmap_amd import Engine  # noqa: E402

WINDOW = 0.25  # seconds, at least, per timed window
ROUNDS = 3
SIZES = [1 << 10, 1 << 16, 1 << 20]
if len(sys.argv) > 1:
    SIZES = [n for n in SIZES if n <= 1 << int(sys.argv[1])]
OPERANDS = sys.argv[2].split(",") if len(sys.argv) > 2 else ["dense256", "sparse64k", "runs512"]

eng = Engine(0)
dev = torch.device("cuda", 0)
g = torch.Generator(device=dev)
g.manual_seed(0xADD)


def window(f):
    """seconds per call of f over a window of at least WINDOW seconds (f is synchronous)"""
    reps = 1
    while True:
        t0 = time.perf_counter()
        for _ in range(reps):
            f()
        eng.sync()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if dt >= WINDOW or reps >= 4096:
            return dt / reps
        reps *= 4


def operand(name):
    """-> (batch, number of keys)"""
    i = torch.arange(1 << 24, device=dev, dtype=torch.int64)
    if name == "dense256":
        return eng.from_values(i[(i & 3) != 3]), 256
    if name == "sparse64k":
        return eng.from_values(i * 256), 65536
    return eng.from_values((i >> 6) * 128 + (i & 63), run_optimize=True), 512


def delta(n, shape, keys):
    if shape == "clustered":
        return ((keys // 2 - 4) << 16) + torch.randint(0, 8 << 16, (n,), generator=g, device=dev, dtype=torch.int64)
    return torch.randint(0, min(2 * keys, 65536) << 16, (n,), generator=g, device=dev, dtype=torch.int64)


for name in OPERANDS:
    op, keys = operand(name)
    so = eng.batch_stats(op)
    present = torch.zeros(65536, dtype=torch.bool, device=dev)
    present[torch.unique(eng.to_values(op, dtype=torch.int64) >> 16)] = True
    print(f"operand {name}: {so['containers']} containers (A {so['array']} / B {so['bitmap']} / R {so['run']}), "
          f"{so['payload_bytes'] / 1e6:.1f} MB", flush=True)
    for n in SIZES:
        for shape in ("clustered", "scattered"):
            v = delta(n, shape, keys)
            vkeys = torch.unique(v >> 16)
            for remove in (False, True):
                pair_op = "andnot" if remove else "or"

                def call():
                    eng.release(eng.mutate_values(op, v, remove)[0])

                def yardstick(keep=False):
                    d = eng.from_values(v)
                    eng.pairwise(pair_op, op, d)
                    r = eng.load([eng.fetch().serialize()])
                    eng.release(d)
                    if keep:
                        return r
                    eng.release(r)

                r, changed = eng.mutate_values(op, v, remove)  # the bytes, once; also the warm-up
                y = yardstick(keep=True)
                same = eng.batch_fetch(r).serialize() == eng.batch_fetch(y).serialize()
                assert same or name == "runs512", (name, n, shape, remove)
                st = eng.batch_stats(r)
                cells = int((present[vkeys]).sum()) if remove else int(vkeys.numel())
                model = 8 * n + 3 * 8192 * cells + so["payload_bytes"] + st["payload_bytes"]
                eng.release(r)
                eng.release(y)
                ms = {"call": [], "yard": []}
                for _ in range(ROUNDS):
                    ms["call"].append(window(call) * 1e3)
                    ms["yard"].append(window(yardstick) * 1e3)
                s, yd = statistics.median(ms["call"]), statistics.median(ms["yard"])
                print(f"{name} n=2^{n.bit_length() - 1} {shape} {'remove' if remove else 'add'}: changed {changed}, "
                      f"cells {cells}, C'={st['containers']} (A {st['array']} / B {st['bitmap']} / R {st['run']}), "
                      f"model {model / 1e6:.1f} MB; mutate_values {s:.3f} ms, from_values + {pair_op} + fetch + load "
                      f"{yd:.3f} ms ({yd / s:.1f}x){'' if same else ' [yardstick bytes differ: its run containers]'}; "
                      f"spread call {(max(ms['call']) - min(ms['call'])) / s * 100:.0f} % yard "
                      f"{(max(ms['yard']) - min(ms['yard'])) / yd * 100:.0f} %; rounds call "
                      + " ".join(f"{x:.3f}" for x in ms["call"]) + " yard " + " ".join(f"{x:.3f}" for x in ms["yard"]),
                      flush=True)
    eng.release(op)
