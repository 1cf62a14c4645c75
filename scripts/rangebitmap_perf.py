"""Range-encoded index queries, timed (profiles/rangebitmap/rangebitmap_perf.txt).

One index: 2^26 rows of uniform 27-bit values (seeded), 1,024 blocks of 27 slices, every slice a bitmap
record: about 226 MB of container payload.  The stream is the package's Appender's (numpy, on the host, outside
every timed region).  Forms: lte, eq and between, each as a bitmap (rangebitmap_query: the kernel, then the
dense-bitset builder over its workspace) and as a cardinality (rangebitmap_count: the kernel and one 8-byte
read-back), without a context and with a half-dense one (every other row).  Next to them Engine.bsi
compare(LE) over a bit-sliced index of the same values (27 slices + ebM), which moves a similar number of bytes.

Call times by the host clock around calls that end in a synchronise, windows of at least 0.25 s, the forms
alternating in one process, three rounds, medians and the spread (max - min over the median).  "index MB" is
the model of what the query kernel has to read: the payload of the slices it does not skip (all 27, or 26
when the threshold's bit 0 is set and slice 0 is only skipped; eq reads all), plus the context's containers.
The GB/s of a count form is that over the WHOLE call (launch, kernel, read-back), a lower bound of the kernel's
rate; the kernel's own time comes from a rocprofv3 --kernel-trace --stats run of `... once`.
Arguments: [log2 rows, default 26] [once]."""
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from roaringbitmap_amd import Engine, RangeBitmap, RoaringBitmap  # noqa: E402

WINDOW = 0.25
ROUNDS = 3
LOG_ROWS = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 26
ONCE = "once" in sys.argv[1:]
BITS = 27

eng = Engine(0)
rng = np.random.default_rng(0x2A27)
n = 1 << LOG_ROWS
values = rng.integers(0, 1 << BITS, n, dtype=np.uint64)

t0 = time.perf_counter()
app = RangeBitmap.appender((1 << BITS) - 1)
app.add_many(values)
stream = app.serialize()
print(f"index: 2^{LOG_ROWS} rows, {BITS} slices, stream {len(stream) / 1e6:.1f} MB, built on the host in "
      f"{time.perf_counter() - t0:.1f} s", flush=True)
idx = eng.rangebitmap_load(stream)
info = eng.rangebitmap_info(idx)
payload = info["payload_bytes"]
print(f"resident: {info['blocks']} blocks, container payload {payload / 1e6:.1f} MB", flush=True)

ctx_bm = RoaringBitmap.from_values(np.arange(0, n, 2, dtype=np.uint32), run_optimize=True)
ctx = eng.load_pair(ctx_bm)[0]
ctx_bytes = eng.batch_stats(ctx)["payload_bytes"]

cols = np.arange(n, dtype=np.uint32)
bsi, nbits, mn, mx = eng.bsi_from_columns(cols, values.astype(np.int32))
bsi_bytes = eng.batch_stats(bsi)["payload_bytes"]

T = int(values[12345]) | 1  # bit 0 set: lte skips slice 0
LO, HI = (1 << 25) + 12345, (1 << 26) + 54321
per_slice = payload / BITS


def check():
    """the answers, once, against numpy (also the warm-up of every path)"""
    want = {"lte": values <= T, "eq": values == T, "between": (values >= LO) & (values <= HI)}
    half = (np.arange(n) & 1) == 0
    for op, a, b in (("lte", T, 0), ("eq", T, 0), ("between", LO, HI)):
        assert eng.rangebitmap_count(idx, op, a, b) == int(want[op].sum()), op
        assert eng.rangebitmap_count(idx, op, a, b, ctx) == int((want[op] & half).sum()), op
        out = eng.rangebitmap_query(idx, op, a, b)
        assert eng.batch_stats(out)["cardinality"] == int(want[op].sum()), op
        eng.release(out)
    eng.bsi(bsi, "LE", nbits, T, 0, mn, mx)
    assert eng.fetch().getLongCardinality() == int(want["lte"].sum())


def window(f):
    reps = 1
    while True:
        eng.sync()
        t = time.perf_counter()
        for _ in range(reps):
            f()
        eng.sync()
        dt = time.perf_counter() - t
        if ONCE or dt >= WINDOW or reps >= 4096:
            return dt / reps
        reps *= 4


def q(op, a, b=0, c=None):
    eng.release(eng.rangebitmap_query(idx, op, a, b, c))


forms = {
    "lteCardinality": (lambda: eng.rangebitmap_count(idx, "lte", T), 26 * per_slice),
    "lteCardinality+ctx": (lambda: eng.rangebitmap_count(idx, "lte", T, 0, ctx), 26 * per_slice + ctx_bytes),
    "eqCardinality": (lambda: eng.rangebitmap_count(idx, "eq", T), 27 * per_slice),
    "eqCardinality+ctx": (lambda: eng.rangebitmap_count(idx, "eq", T, 0, ctx), 27 * per_slice + ctx_bytes),
    "betweenCardinality": (lambda: eng.rangebitmap_count(idx, "between", LO, HI), 27 * per_slice),
    "betweenCardinality+ctx": (lambda: eng.rangebitmap_count(idx, "between", LO, HI, ctx), 27 * per_slice + ctx_bytes),
    "lte": (lambda: q("lte", T), 26 * per_slice),
    "lte+ctx": (lambda: q("lte", T, 0, ctx), 26 * per_slice + ctx_bytes),
    "eq": (lambda: q("eq", T), 27 * per_slice),
    "eq+ctx": (lambda: q("eq", T, 0, ctx), 27 * per_slice + ctx_bytes),
    "between": (lambda: q("between", LO, HI), 27 * per_slice),
    "bsi compare(LE)": (lambda: eng.bsi(bsi, "LE", nbits, T, 0, mn, mx), bsi_bytes),
}

check()
ms = {k: [] for k in forms}
for _ in range(1 if ONCE else ROUNDS):
    for k, (f, _) in forms.items():
        ms[k].append(window(f) * 1e3)
for k, (_, moved) in forms.items():
    m = statistics.median(ms[k])
    sp = (max(ms[k]) - min(ms[k])) / m
    print(f"{k:24s} {m:8.3f} ms per call (spread {100 * sp:.0f} %), index {moved / 1e6:6.1f} MB -> "
          f"{moved / m / 1e6:6.0f} GB/s over the whole call", flush=True)
