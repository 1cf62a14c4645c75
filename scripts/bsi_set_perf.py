"""(column, value) pairs written into a resident bit-sliced index on the device, timed
(profiles/bsi_set/bsi_set_perf.txt).

Operand: the resident index of 2^24 arange columns with uniform 31-bit values (256 keys, 31 slices of bitmap
containers; Engine.bsi_from_columns).  Batches of 2^10, 2^16 and 2^20 pairs with uniform 31-bit values, as
device tensors, in three mixes over two column shapes:
  updates   columns of the operand: arange (the first n) or scattered (i * 0x9E3779B1 mod 2^24)
  inserts   the same shapes shifted above the operand (+ 2^24): new columns in new keys
  mixed     0.45 n updates, 0.45 n inserts and 0.1 n repeats of the batch's first columns with other values
Timed: ms per Engine.bsi_set_values + release (csrc/bsiset.hip), a host clock around calls that end in a
synchronise, windows of at least 0.25 s, three rounds alternating with the yardstick, medians.  Yardstick: the
only route that exists without the call -- Engine.bsi_to_pairs into device tensors, the batch appended, a
stable device sort by column that keeps each column's last pair (torch), then Engine.bsi_from_columns --
in the same process on the same input, its bitmaps asserted byte-equal to the call's once per row.
Arguments: [largest log2 n of a batch] [mixes, comma separated]."""
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from roaringbitmap_amd import Engine  # noqa: E402

WINDOW = 0.25  # seconds, at least, per timed window
ROUNDS = 3
N_OPERAND = 1 << 24
SIZES = [1 << 10, 1 << 16, 1 << 20]
if len(sys.argv) > 1:
    SIZES = [n for n in SIZES if n <= 1 << int(sys.argv[1])]
MIXES = sys.argv[2].split(",") if len(sys.argv) > 2 else ["updates", "inserts", "mixed"]

eng = Engine(0)
dev = torch.device("cuda", 0)
g = torch.Generator(device=dev)
g.manual_seed(0x5E7)


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


def fetch(b):
    return [x.serialize() for x in eng.batch_fetch_range(b)]


def columns(n, shape):
    i = torch.arange(n, device=dev, dtype=torch.int64)
    return i if shape == "arange" else (i * 0x9E3779B1) & (N_OPERAND - 1)


def batch(n, mix, shape):
    if mix == "updates":
        return columns(n, shape)
    if mix == "inserts":
        return columns(n, shape) + N_OPERAND
    k = (n * 45) // 100
    c = columns(n, shape)
    head = torch.cat([c[:k], c[k:2 * k] + N_OPERAND])
    return torch.cat([head, head[:n - 2 * k]])


ocols = torch.arange(N_OPERAND, device=dev, dtype=torch.int64)
ovals = torch.randint(0, 1 << 31, (N_OPERAND,), generator=g, device=dev, dtype=torch.int64)
op, nbits, mn, mx = eng.bsi_from_columns(ocols, ovals)
del ocols, ovals
print(f"operand: 2^24 arange columns, {nbits} slices, {eng.batch_stats(op)['containers']} containers, "
      f"{eng.batch_stats(op)['payload_bytes'] / 1e6:.0f} MB", flush=True)

for n in SIZES:
    for mix in MIXES:
        for shape in ("arange", "scattered"):
            bc = batch(n, mix, shape)
            bv = torch.randint(0, 1 << 31, (n,), generator=g, device=dev, dtype=torch.int64)

            def call():
                eng.release(eng.bsi_set_values(op, nbits, bc, bv, mn, mx)[0])

            def yardstick(keep=False):
                pc, pv = eng.bsi_to_pairs(op, nbits, dtype=torch.int64)
                c, v = torch.cat([pc, bc]), torch.cat([pv, bv])
                c, order = torch.sort(c, stable=True)
                last = torch.ones_like(c, dtype=torch.bool)
                last[:-1] = c[1:] != c[:-1]
                r = eng.bsi_from_columns(c[last], v[order][last])
                if keep:
                    return r
                eng.release(r[0])

            r, nb2, mn2, mx2 = eng.bsi_set_values(op, nbits, bc, bv, mn, mx)  # the bytes, once; also the warm-up
            y, nby, _, _ = yardstick(keep=True)
            assert nb2 == nby and fetch(r) == fetch(y), (n, mix, shape)
            st = eng.batch_stats(r)
            K = int(torch.unique(torch.cat([bc >> 16, torch.arange(N_OPERAND >> 16, device=dev)])).numel())
            eng.release(r)
            eng.release(y)
            ms = {"set": [], "yard": []}
            for _ in range(ROUNDS):
                ms["set"].append(window(call) * 1e3)
                ms["yard"].append(window(yardstick) * 1e3)
            s, yd = statistics.median(ms["set"]), statistics.median(ms["yard"])
            print(f"n=2^{n.bit_length() - 1} {mix} {shape}: K={K} keys x {1 + nb2} cells + table, "
                  f"C={st['containers']} (A {st['array']} / B {st['bitmap']} / R {st['run']}); set_values {s:.3f} ms, "
                  f"to_pairs + merge + from_columns {yd:.3f} ms ({yd / s:.1f}x); {n / s / 1e6:.4f} G pairs/s; rounds set "
                  + " ".join(f"{v:.3f}" for v in ms["set"]) + " yard " + " ".join(f"{v:.3f}" for v in ms["yard"]),
                  flush=True)
eng.release(op)
