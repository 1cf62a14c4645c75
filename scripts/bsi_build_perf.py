"""A bit-sliced index built from (column, value) pairs and read back on the device, timed
(profiles/bsi_build/bsi_build_perf.txt).

Build: n = 2^20, 2^24 pairs with uniform 31-bit values, device-resident, over three column shapes (arange,
2^26 columns spread by an odd multiplier, 2^32 columns spread the same way: every key, so the workspace
goes through the pass scheme); ms per Engine.bsi_from_columns + release, with and without run_optimize, and
the route the engine had before: RoaringBitmapSliceIndex.from_columns on the host (one host sort per
slice) followed by Engine.load, on the same pairs in the same process, its bytes asserted equal.  The device
build alternates with itself in three rounds of windows of at least 0.25 s and the medians are reported;
the host route is timed in every round at 2^20 and once at 2^24 (tens of seconds each).
Bytes per build: the pairs read (8 n: keys and min / max, then 8 n per pass and sweep), the workspace of
K (nbits + 1) bitmaps of 8 KiB zeroed and read once per sweep (one pass: zeroed once, read twice), and the
payload written.

Values out: Engine.bsi_get_values of 2^20 device-resident columns and Engine.bsi_to_pairs of the 2^24
arange index, against the host getValues / toPairList of the same index.
Arguments: [largest log2 n] [quick: the device paths alone]."""
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from roaringbitmap_amd import Engine, RoaringBitmapSliceIndex  # noqa: E402

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
g.manual_seed(0xB51)


def inputs(n):
    i = torch.arange(n, device=dev, dtype=torch.int64)
    return {  # an odd multiplier is a bijection of the low bits: distinct columns in a scattered order
        "arange": i,
        "uniform 2^26": (i * 0x9E3779B1) & ((1 << 26) - 1),
        "uniform 2^32": (i * 0x9E3779B1) & ((1 << 32) - 1),
    }


def window(f):
    """seconds per call of f over a window of at least WINDOW seconds (f is synchronous or synced here)"""
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


print("== build ==", flush=True)
for n in SIZES:
    vals = torch.randint(0, 1 << 31, (n,), generator=g, device=dev, dtype=torch.int64)
    hvals = vals.cpu().numpy()
    for name, cols in inputs(n).items():
        hcols = cols.cpu().numpy()

        def gpu_build(ro):
            eng.release(eng.bsi_from_columns(cols, vals, ro)[0])

        def old_route(ro=False):
            x = RoaringBitmapSliceIndex.from_columns(hcols, hvals, ro)
            eng.release(eng.load([x.ebM] + x.bA))
            return x

        ms = {"gpu": [], "gpu ro": [], "host+load": []}
        # the bytes, once, before any timing (this is also the warm-up of every path)
        stats = None
        for ro in (False, True):
            x = None
            if not QUICK and (not ro or n <= 1 << 20):
                t0 = time.perf_counter()
                x = old_route(ro)
                eng.sync()
                if not ro:
                    ms["host+load"].append((time.perf_counter() - t0) * 1e3)
            b, nbits, mn, mx = eng.bsi_from_columns(cols, vals, ro)
            if x is not None:
                assert fetch(b) == [x.ebM.serialize()] + [s.serialize() for s in x.bA], (n, name, ro)
                assert (nbits, mn, mx) == (x.bitCount(), x.minValue, x.maxValue)
            if not ro:
                stats = eng.batch_stats(b)
                K = int(eng.batch_counts(b)[0])
            eng.release(b)
        for r in range(ROUNDS):
            ms["gpu"].append(window(lambda: gpu_build(False)) * 1e3)
            ms["gpu ro"].append(window(lambda: gpu_build(True)) * 1e3)
            if QUICK or n > 1 << 20:
                continue
            t0 = time.perf_counter()
            old_route(False)
            eng.sync()
            ms["host+load"].append((time.perf_counter() - t0) * 1e3)
        if QUICK:
            ms["host+load"] = [float("inf")]
        m_in = nbits + 1
        ws = 8192 * K * m_in
        passes = -(-K // max(1, min(K, BUDGET // (8192 * m_in))))
        moved = 8 * n + (8 * n + 3 * ws if passes == 1 else 2 * passes * 8 * n + 4 * ws) + stats["payload_bytes"]
        m = med(ms["gpu"])
        print(f"n=2^{n.bit_length() - 1} {name}: K={K} keys x {m_in} inputs, C={stats['containers']} (A {stats['array']} / "
              f"B {stats['bitmap']}), workspace {ws / 2**20:.0f} MiB in {passes} pass(es); gpu {m:.3f} ms, "
              f"gpu+runOptimize {med(ms['gpu ro']):.3f} ms, host from_columns+load {med(ms['host+load']):.1f} ms "
              f"({med(ms['host+load']) / m:.0f}x, {len(ms['host+load'])} run(s)); {moved / 1e6:.1f} MB moved, "
              f"{moved / m / 1e6:.1f} GB/s, {n / m / 1e6:.3f} G pairs/s; rounds gpu "
              + " ".join(f"{x:.3f}" for x in ms["gpu"]), flush=True)
        assert m <= med(ms["host+load"]), "the device build is slower than the host route"
        del cols, hcols

print("== values out ==", flush=True)
n = SIZES[-1]
vals = torch.randint(0, 1 << 31, (n,), generator=g, device=dev, dtype=torch.int64)
cols = torch.arange(n, device=dev, dtype=torch.int64)
b, nbits, mn, mx = eng.bsi_from_columns(cols, vals)
nq = 1 << 20
q = torch.randint(0, 2 * n, (nq,), generator=g, device=dev, dtype=torch.int64)  # about half are absent
hq = q.cpu().numpy()
got = eng.bsi_get_values(b, nbits, q).cpu().numpy()
hv = vals.cpu().numpy()
want = np.where(hq < n, hv[np.minimum(hq, n - 1)], -1)
assert (got == want).all()
pc, pv = eng.bsi_to_pairs(b, nbits, dtype=torch.int64)
assert bool((pc == cols).all()) and bool((pv == vals).all())
host_get = host_pairs = float("inf")
if not QUICK:
    x = RoaringBitmapSliceIndex.from_columns(np.arange(n), hv)
    t0 = time.perf_counter()
    hg = x.getValues(hq)
    host_get = (time.perf_counter() - t0) * 1e3
    assert (hg == want).all()
    t0 = time.perf_counter()
    hc, hp = x.toPairList()
    host_pairs = (time.perf_counter() - t0) * 1e3
    assert (hc == np.arange(n)).all() and (hp == hv).all()
rows = {"get": [], "pairs u32": [], "pairs i64": []}
for _ in range(ROUNDS):
    rows["get"].append(window(lambda: eng.bsi_get_values(b, nbits, q)) * 1e3)
    rows["pairs u32"].append(window(lambda: eng.bsi_to_pairs(b, nbits, dtype=torch.uint32)) * 1e3)
    rows["pairs i64"].append(window(lambda: eng.bsi_to_pairs(b, nbits, dtype=torch.int64)) * 1e3)
st = eng.batch_stats(b)
mg, mp, mp64 = med(rows["get"]), med(rows["pairs u32"]), med(rows["pairs i64"])
print(f"index of 2^{n.bit_length() - 1} arange columns, {nbits} slices, {st['containers']} containers (A {st['array']} / "
      f"B {st['bitmap']} / R {st['run']}), payload {st['payload_bytes'] / 1e6:.1f} MB")
print(f"bsi_get_values, 2^20 queries: {mg:.3f} ms = {nq / mg / 1e6:.3f} G queries/s; host getValues {host_get:.1f} ms "
      f"({host_get / mg:.0f}x); rounds " + " ".join(f"{v:.3f}" for v in rows["get"]))
print(f"bsi_to_pairs, 2^{n.bit_length() - 1} pairs: uint32 / int32 {mp:.3f} ms = {8 * n / mp / 1e6:.1f} GB/s written, "
      f"{n / mp / 1e6:.3f} G pairs/s; int64 / int64 {mp64:.3f} ms = {16 * n / mp64 / 1e6:.1f} GB/s written; host toPairList "
      f"{host_pairs:.1f} ms ({host_pairs / mp:.0f}x); rounds " + " ".join(f"{v:.3f}" for v in rows["pairs u32"]), flush=True)
assert mg <= host_get and mp <= host_pairs
eng.release(b)
