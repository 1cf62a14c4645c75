"""Construction from values and expansion to values on the device, timed (profiles/from_values/build_perf.txt).

Build: n = 2^20, 2^24, 2^27 values, device-resident, in four distributions (uniform over 2^32, uniform
over 2^26, sorted arange, all in one key); ms per Engine.from_values with and without run_optimize, and
the route the engine had before: the host builder (rbg_from_values: one thread's sort) followed by
Engine.load (upload + device decode), on the same values in the same process, its bytes asserted equal.
All of them alternate in every round; medians are reported (the host route runs once at 2^27).  (The
scatter kernel without the read in front of every atomic, which this script also alternated, was removed
from the engine; its numbers are in profiles/from_values/build_perf.txt.)
Bytes per build: the two reads of the input (4 n each), the workspace of C 8 KiB bitmaps zeroed once and
read twice, and the payload written.  Arguments: [largest log2 n] [quick: the device builds alone].

Expand: the C2 synthetic operand and a 2^24-value array-only bitmap through Engine.to_values into a
device tensor, against the host rbg_to_values (RoaringBitmap.toArray) of the same bitmap."""
import ctypes
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from roaringbitmap_amd import Engine, RoaringBitmap, _lib  # noqa: E402

WINDOW = 0.25  # seconds, at least, per timed window
ROUNDS = 3
SIZES = [1 << 20, 1 << 24, 1 << 27]
if len(sys.argv) > 1:  # a smaller run: the largest log2(n)
    SIZES = [n for n in SIZES if n <= 1 << int(sys.argv[1])]
QUICK = "quick" in sys.argv[2:]  # the device builds alone: no host route, no expansion

eng = Engine(0)
dev = torch.device("cuda", 0)
g = torch.Generator(device=dev)
g.manual_seed(0xB11D)


def u32(t):  # int64 values below 2^32 -> uint32 tensor (the low little-endian words)
    return t.contiguous().view(torch.int32)[::2].contiguous().view(torch.uint32)


def inputs(n):
    return {
        "uniform 2^32": u32(torch.randint(0, 1 << 32, (n,), generator=g, device=dev, dtype=torch.int64)),
        "uniform 2^26": u32(torch.randint(0, 1 << 26, (n,), generator=g, device=dev, dtype=torch.int64)),
        "sorted arange": u32(torch.arange(n, device=dev, dtype=torch.int64)),
        "one key": u32((9 << 16) + torch.randint(0, 1 << 16, (n,), generator=g, device=dev, dtype=torch.int64)),
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


print("== build ==")
for n in SIZES:
    ratio = {}
    for name, t in inputs(n).items():
        host = t.cpu().view(torch.int32).numpy().view(np.uint32)

        def gpu_build(ro):
            eng.release(eng.from_values(t, ro))

        kept = {}

        def old_route(ro=False):
            bm = RoaringBitmap.from_values(host, ro)
            eng.release(eng.load([bm]))
            kept[ro] = bm

        # the bytes, once, before any timing (this is also the warm-up of every path)
        stats = None
        for ro in (False, True):
            if QUICK:
                kept[ro] = RoaringBitmap.from_values(host, ro) if n <= 1 << 20 else None
            else:
                old_route(ro)
            b = eng.from_values(t, ro)
            assert kept[ro] is None or eng.batch_fetch(b).serialize() == kept[ro].serialize(), (n, name, ro)
            if not ro:
                stats = eng.batch_stats(b)
            eng.release(b)
        kept.clear()
        ms = {"gpu": [], "gpu ro": [], "host+load": []}
        for _ in range(ROUNDS):
            ms["gpu"].append(window(lambda: gpu_build(False)) * 1e3)
            ms["gpu ro"].append(window(lambda: gpu_build(True)) * 1e3)
            if QUICK or (n > 1 << 24 and ms["host+load"]):  # 6 to 9 s each at 2^27: one round
                continue
            t0 = time.perf_counter()
            old_route(False)
            eng.sync()
            ms["host+load"].append((time.perf_counter() - t0) * 1e3)
        if QUICK:
            ms["host+load"] = [float("inf")]
        C = stats["containers"]
        moved = 2 * 4 * n + 3 * 8192 * C + stats["payload_bytes"]
        m = med(ms["gpu"])
        ratio[name] = m
        print(f"n=2^{n.bit_length() - 1} {name}: C={C} (A {stats['array']} / B {stats['bitmap']}) "
              f"gpu {m:.3f} ms, gpu+runOptimize {med(ms['gpu ro']):.3f} ms, host from_values+load "
              f"{med(ms['host+load']):.1f} ms ({med(ms['host+load']) / m:.0f}x); {moved / 1e6:.1f} MB moved, "
              f"{moved / m / 1e6:.1f} GB/s, {n / m / 1e6:.2f} G values/s; rounds gpu "
              + " ".join(f"{x:.3f}" for x in ms["gpu"]), flush=True)
        assert m <= med(ms["host+load"]), "the device build is slower than the host route"
        del t, host
    print(f"n=2^{n.bit_length() - 1} one key / uniform 2^32: {ratio['one key'] / ratio['uniform 2^32']:.2f}")

if QUICK:
    sys.exit(0)
print("== expand ==")


def expand_case(tag, batch):
    st = eng.batch_stats(batch)
    card = st["cardinality"]
    t0 = time.perf_counter()
    out = eng.to_values(batch, dtype=torch.uint32)
    eng.sync()
    first = (time.perf_counter() - t0) * 1e3
    buf = eng.batch_fetch(batch).serialize()
    hb = _lib.rbg_buffer()
    t0 = time.perf_counter()  # the host rbg_to_values itself, without the binding's copies
    _lib.check(_lib.lib().rbg_to_values(buf, len(buf), ctypes.byref(hb)))
    host_ms = (time.perf_counter() - t0) * 1e3
    hv = np.ctypeslib.as_array(ctypes.cast(hb.data, ctypes.POINTER(ctypes.c_uint32)), shape=(hb.len // 4,))
    got = out.cpu().view(torch.int32).numpy().view(np.uint32)
    same = got.shape == hv.shape and bool((got == hv).all())
    del hv, got
    _lib.lib().rbg_free(ctypes.byref(hb))
    rows = {"uint32": [], "int64": []}
    for _ in range(ROUNDS):
        rows["uint32"].append(window(lambda: eng.to_values(batch, dtype=torch.uint32)) * 1e3)
        rows["int64"].append(window(lambda: eng.to_values(batch, dtype=torch.int64)) * 1e3)
    m = med(rows["uint32"])
    print(f"{tag}: {st['containers']} containers (A {st['array']} / B {st['bitmap']} / R {st['run']}), "
          f"cardinality {card}, payload {st['payload_bytes'] / 1e6:.1f} MB; first call (directory build) "
          f"{first:.3f} ms; uint32 {m:.3f} ms = {4 * card / m / 1e6:.1f} GB/s written, "
          f"{st['payload_bytes'] / m / 1e6:.1f} GB/s payload read; int64 {med(rows['int64']):.3f} ms = "
          f"{8 * card / med(rows['int64']) / 1e6:.1f} GB/s written; host toArray {host_ms:.1f} ms "
          f"({host_ms / m:.0f}x); equal {same}; rounds " + " ".join(f"{x:.3f}" for x in rows["uint32"]), flush=True)
    assert same and m <= host_ms


c2 = eng.synth(0, 0xC2A0)
expand_case("C2 operand", c2)
eng.release(c2)
arr = eng.from_values(u32(torch.randint(0, 1 << 32, (1 << 24,), generator=g, device=dev, dtype=torch.int64)))
expand_case("2^24 uniform values, arrays alone", arr)
eng.release(arr)
