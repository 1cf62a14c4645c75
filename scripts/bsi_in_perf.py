"""WHERE value IN (...) over a resident bit-sliced index, timed (profiles/bsi_in/bsi_in_perf.txt).

Rows: the 2^24 arange index and the 2^20 uniform-2^26 index (columns spread by an odd multiplier) of DESIGN
§3.10, uniform 31-bit values, resident (Engine.bsi_from_columns), each with lists of 1, 20, 4,096 and 2^20
values drawn from the index's own values, no foundSet.  Timed: ms per Engine.bsi_in + release
(csrc/bsiin.hip; the host list, int32, is uploaded, sorted and de-duplicated inside the call), a host clock around
calls that end in a synchronise, windows of at least 0.25 s, three rounds alternating with the yardstick,
medians.  Yardstick: the only earlier device route to the same resident result, in the same process on the
same index -- Engine.bsi_to_pairs -> torch.isin against the list already on the device -> Engine.from_values
(the pairwise and with a foundSet in front is skipped: there is none); its bytes are asserted equal to the
fused result once per row where the result holds no run container (the full-container exception of DESIGN
§3.12 does not apply).
Arguments: [largest log2 n] [quick: the fused path alone]."""
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from roaringbitmap_amd import Engine  # noqa: E402

WINDOW = 0.25  # seconds, at least, per timed window
ROUNDS = 3
SHAPES = [("arange", 1 << 24), ("uniform 2^26", 1 << 20)]
LISTS = [1, 20, 4096, 1 << 20]
if len(sys.argv) > 1:  # a smaller run: the largest log2(n)
    SHAPES = [(s, min(n, 1 << int(sys.argv[1]))) for s, n in SHAPES]
QUICK = "quick" in sys.argv[2:]

eng = Engine(0)
dev = torch.device("cuda", 0)
g = torch.Generator(device=dev)
g.manual_seed(0x1A)


def window(f):
    """seconds per call of f over a window of at least WINDOW seconds (f is synchronous)"""
    reps = 1
    while True:
        t0 = time.perf_counter()
        for _ in range(reps):
            f()
        eng.sync()
        dt = time.perf_counter() - t0
        if dt >= WINDOW or reps >= 4096:
            return dt / reps
        reps *= 4


for shape, n in SHAPES:
    i = torch.arange(n, device=dev, dtype=torch.int64)
    cols = i if shape == "arange" else (i * 0x9E3779B1) & ((1 << 26) - 1)
    vals = torch.randint(0, 1 << 31, (n,), generator=g, device=dev, dtype=torch.int64)
    idx, nbits, _, _ = eng.bsi_from_columns(cols, vals)
    K = int(eng.batch_counts(idx)[0])
    for n_list in LISTS:
        pick = torch.randint(0, n, (n_list,), generator=g, device=dev)
        list_dev = vals[pick]
        list_host = list_dev.cpu().numpy().astype(np.int32)  # as the C entry point takes it

        def fused():
            eng.release(eng.bsi_in(idx, nbits, list_host))

        def yardstick(keep=False):
            c, v = eng.bsi_to_pairs(idx, nbits, dtype=torch.int64)
            b = eng.from_values(c[torch.isin(v, list_dev)])
            if keep:
                return b
            eng.release(b)

        r = eng.bsi_in(idx, nbits, list_host)  # the bytes, once; also the warm-up
        stats = eng.batch_stats(r)
        if not QUICK:
            y = yardstick(keep=True)
            if stats["run"] == 0:
                assert eng.batch_fetch(r).serialize() == eng.batch_fetch(y).serialize(), (shape, n_list)
            eng.release(y)
        eng.release(r)
        ms = {"fused": [], "yardstick": []}
        for _ in range(ROUNDS):
            ms["fused"].append(window(fused) * 1e3)
            ms["yardstick"].append(float("inf") if QUICK else window(yardstick) * 1e3)
        m, y = statistics.median(ms["fused"]), statistics.median(ms["yardstick"])
        verdict = ""
        if not QUICK:
            verdict = f", yardstick {y:.3f} ms ({y / m:.1f}x" + (", FUSED IS SLOWER" if m > y else "") + ")"
        print(f"n=2^{n.bit_length() - 1} {shape}, {nbits} slices, K={K} keys, list {n_list}: "
              f"{stats['cardinality']} columns match, C={stats['containers']} (A {stats['array']} / "
              f"B {stats['bitmap']} / R {stats['run']}); fused {m:.3f} ms{verdict}, {n / m / 1e6:.3f} G columns/s; "
              "rounds fused " + " ".join(f"{v:.3f}" for v in ms["fused"])
              + "; yardstick " + " ".join(f"{v:.3f}" for v in ms["yardstick"]), flush=True)
    eng.release(idx)
    del cols, vals
