"""Two resident bit-sliced indexes added on the device, timed (profiles/bsi_add/bsi_add_perf.txt).

Rows: n = 2^20, 2^24 columns over two column shapes (arange; 2^26 columns spread by an odd multiplier), index
a with uniform 31-bit values and index b with uniform 16-bit values over the same columns, both resident
(Engine.bsi_from_columns).  Timed: ms per Engine.bsi_add + release (csrc/bsiadd.hip), a host clock around
calls that end in a synchronise, windows of at least 0.25 s, three rounds alternating with the yardstick,
medians.  Yardstick: the only earlier route to the same resident result -- RoaringBitmapSliceIndex.add's
composed route (RBG_BSI_ADD_COMPOSED=1: one pairwise and + one in-place xor per addDigit, the carry's
isEmpty() on the host) on the same bitmaps followed by Engine.load, in the same process, its bytes asserted
equal to the fused result once per row; timed in every round at 2^20 and once at 2^24.
Bytes per sum: both indexes' payloads read once, the workspace of K (2 + max(na, nb)) bitmaps of 8 KiB
written once and read three times (min / max descent, plan, write), the payload written.
Arguments: [largest log2 n] [quick: the fused path alone]."""
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from roaringbitmap_amd import Engine, RoaringBitmap, RoaringBitmapSliceIndex  # noqa: E402

WINDOW = 0.25  # seconds, at least, per timed window
ROUNDS = 3
SIZES = [1 << 20, 1 << 24]
if len(sys.argv) > 1:  # a smaller run: the largest log2(n)
    SIZES = [n for n in SIZES if n <= 1 << int(sys.argv[1])]
QUICK = "quick" in sys.argv[2:]
BUDGET = int(os.environ.get("RBG_BSI_BUILD_WS", 1 << 30))

eng = Engine(0)
dev = torch.device("cuda", 0)
g = torch.Generator(device=dev)
g.manual_seed(0xADD)


def inputs(n):
    i = torch.arange(n, device=dev, dtype=torch.int64)
    return {"arange": i, "uniform 2^26": (i * 0x9E3779B1) & ((1 << 26) - 1)}


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


def med(v):
    return statistics.median(v)


def fetch(b):
    return [x.serialize() for x in eng.batch_fetch_range(b)]


for n in SIZES:
    va = torch.randint(0, 1 << 31, (n,), generator=g, device=dev, dtype=torch.int64)
    vb = torch.randint(0, 1 << 16, (n,), generator=g, device=dev, dtype=torch.int64)
    for name, cols in inputs(n).items():
        ia, na, mna, mxa = eng.bsi_from_columns(cols, va)
        ib, nb, mnb, mxb = eng.bsi_from_columns(cols, vb)
        bytes_a, bytes_b = fetch(ia), fetch(ib)
        in_payload = eng.batch_stats(ia)["payload_bytes"] + eng.batch_stats(ib)["payload_bytes"]

        def fused():
            eng.release(eng.bsi_add(ia, na, ib, nb, mna, mxa)[0])

        def composed():
            x = RoaringBitmapSliceIndex(RoaringBitmap(bytes_a[0]), [RoaringBitmap(s) for s in bytes_a[1:]], mna, mxa)
            y = RoaringBitmapSliceIndex(RoaringBitmap(bytes_b[0]), [RoaringBitmap(s) for s in bytes_b[1:]], mnb, mxb)
            os.environ["RBG_BSI_ADD_COMPOSED"] = "1"
            try:
                x.add(y)
            finally:
                del os.environ["RBG_BSI_ADD_COMPOSED"]
            eng.release(eng.load([x.ebM] + x.bA))
            return x

        ms = {"fused": [], "composed+load": []}
        r, nbits, mn, mx = eng.bsi_add(ia, na, ib, nb, mna, mxa)  # the bytes, once; also the warm-up
        stats = eng.batch_stats(r)
        K = int(eng.batch_counts(r)[0])
        if not QUICK:
            t0 = time.perf_counter()
            x = composed()
            eng.sync()
            ms["composed+load"].append((time.perf_counter() - t0) * 1e3)
            assert fetch(r) == [x.ebM.serialize()] + [s.serialize() for s in x.bA], (n, name)
            assert (nbits, mn, mx) == (x.bitCount(), x.minValue, x.maxValue), (n, name)
        eng.release(r)
        for _ in range(ROUNDS):
            ms["fused"].append(window(fused) * 1e3)
            if QUICK or n > 1 << 20:
                continue
            t0 = time.perf_counter()
            composed()
            eng.sync()
            ms["composed+load"].append((time.perf_counter() - t0) * 1e3)
        if QUICK:
            ms["composed+load"] = [float("inf")]
        m_in = 2 + max(na, nb)
        ws = 8192 * K * m_in
        passes = -(-K // max(1, min(K, BUDGET // (8192 * m_in))))
        moved = (1 if passes == 1 else 2) * in_payload + (4 if passes == 1 else 6) * ws + stats["payload_bytes"]
        m, c = med(ms["fused"]), med(ms["composed+load"])
        print(f"n=2^{n.bit_length() - 1} {name}: {na} + {nb} -> {nbits} slices, K={K} keys x {m_in} cells, "
              f"C={stats['containers']} (A {stats['array']} / B {stats['bitmap']} / R {stats['run']}), workspace "
              f"{ws / 2**20:.0f} MiB in {passes} pass(es); fused {m:.3f} ms, composed+load {c:.1f} ms ({c / m:.1f}x, "
              f"{len(ms['composed+load'])} run(s)); {moved / 1e6:.1f} MB moved, {moved / m / 1e6:.1f} GB/s, "
              f"{n / m / 1e6:.3f} G columns/s; rounds fused " + " ".join(f"{v:.3f}" for v in ms["fused"]), flush=True)
        eng.release(ia)
        eng.release(ib)
        del cols
