"""GROUP BY value / COUNT(*) over a resident bit-sliced index, timed (profiles/bsi_transpose/bsi_transpose_perf.txt).

Rows: (a) 2^24 arange columns with uniform 16-bit values (one full result key), (b) uniform values
below 2^20 (16 result keys), (c) below 2^26 (1,024 keys), (d) three distinct values, (e) 2^20 arange columns with
uniform 31-bit values (32,768 result keys, several passes).  The index is resident (Engine.bsi_from_columns).
Timed: ms per Engine.bsi_transpose + release (csrc/bsitr.hip), a host clock around calls that end in a
synchronise, windows of at least 0.25 s, three rounds alternating with the yardstick, medians, the spread between
the rounds reported.  Yardstick: the only earlier device route to the same resident result, in the same process on
the same index -- Engine.bsi_to_pairs (torch tensors) -> torch.unique(return_counts=True) -> Engine.bsi_from_columns.
parallelism = columns / 4096, so batchSize <= 4096 and no run container can appear: the fused bytes and bit count
are asserted equal to the yardstick's once per row (min / max are not compared: from_columns' follow
ensureCapacityInternal's order quirk).
Arguments: [rows, e.g. "abe"] [trace: 20 fused calls per row and nothing else, for a kernel trace] [quick: the
fused path alone, as a build variant is timed (RBG_LIB=<library>)] [par=<parallelism>: another parallelism, e.g.
par=1 on row (a), where the full result key's run flag is evaluated; a result with a run container is not compared
with the yardstick's bytes]."""
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from roaringbitmap_amd import Engine  # noqa: E402

WINDOW = 0.25  # seconds, at least, per timed window
ROUNDS = 3
ROWS = {  # columns, values
    "a": (1 << 24, "uniform 2^16"),
    "b": (1 << 24, "uniform 2^20"),
    "c": (1 << 24, "uniform 2^26"),
    "d": (1 << 24, "three values"),
    "e": (1 << 20, "uniform 2^31"),
}
PICK = sys.argv[1] if len(sys.argv) > 1 else "abcde"
TRACE = "trace" in sys.argv[2:]
QUICK = "quick" in sys.argv[2:]
PAR = [int(a[4:]) for a in sys.argv[2:] if a.startswith("par=")]

eng = Engine(0)
dev = torch.device("cuda", 0)
g = torch.Generator(device=dev)
g.manual_seed(0x7C)


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


def budget():
    v = int(os.environ.get("RBG_BSI_BUILD_WS", "0") or 0)
    return min(v or 1 << 30, 4 << 30)


for row in PICK:
    n, shape = ROWS[row]
    cols = torch.arange(n, device=dev, dtype=torch.int64)
    if shape == "three values":
        vals = torch.tensor([5, 1 << 20, (1 << 30) + 1], device=dev)[torch.randint(0, 3, (n,), generator=g, device=dev)]
    else:
        vals = torch.randint(0, 1 << int(shape.split("^")[1]), (n,), generator=g, device=dev, dtype=torch.int64)
    idx, nbits, _, _ = eng.bsi_from_columns(cols, vals)
    parallelism = PAR[0] if PAR else n // 4096

    def fused():
        eng.release(eng.bsi_transpose(idx, nbits, parallelism)[0])

    def yardstick(keep=False):
        _, v = eng.bsi_to_pairs(idx, nbits, dtype=torch.int64)
        u, cnt = torch.unique(v, return_counts=True)
        b = eng.bsi_from_columns(u, cnt)
        if keep:
            return b
        eng.release(b[0])

    if TRACE:
        for _ in range(20):
            fused()
        eng.release(idx)
        continue
    r, rbits, mn, mx = eng.bsi_transpose(idx, nbits, parallelism)  # the bytes, once; also the warm-up
    stats = eng.batch_stats(r)
    keys = int(eng.batch_counts(r)[0])  # containers of ebM': the result keys
    if not QUICK:
        y = yardstick(keep=True)
        assert rbits == y[1], (row, rbits, y[1])
        if stats["run"] == 0:
            assert [x.serialize() for x in eng.batch_fetch_range(r)] == [x.serialize() for x in eng.batch_fetch_range(y[0])], row
        eng.release(y[0])
    eng.release(r)
    route = os.environ.get("RBG_BSI_TR_ROUTE", "sort" if n < 256 * keys else "count")  # the engine's kBsitSparse
    if route.startswith("s"):  # the values, their sorted copy, the distinct values and the counts; no passes
        work, passes = f"sort route, {4 * 4 * n / 2**20:.1f} MiB of value buffers", 0
    else:
        m = 1 + n.bit_length()  # cells per result key: ebM' and one per bit of the column count
        per_key = 4 * 65536 + 8192 * m
        per_pass = max(1, min(keys, budget() // per_key))
        passes = -(-keys // per_pass)
        work = f"count tables, workspace {per_key * per_pass / 2**20:.1f} MiB"
    ms = {"fused": [], "yardstick": []}
    for _ in range(ROUNDS):
        ms["fused"].append(window(fused) * 1e3)
        ms["yardstick"].append(float("inf") if QUICK else window(yardstick) * 1e3)
    f, yd = statistics.median(ms["fused"]), statistics.median(ms["yardstick"])
    spread = max(max(v) / min(v) - 1 for v in ms.values() if max(v) != float("inf"))
    print(f"({row}) n=2^{n.bit_length() - 1} arange, values {shape}, {nbits} slices, parallelism {parallelism} -> "
          f"K'={keys} result keys, "
          f"nbits'={rbits}, counts {mn}..{mx}, C={stats['containers']} (A {stats['array']} / B {stats['bitmap']} / "
          f"R {stats['run']}); {work}, passes {passes}; fused {f:.3f} ms, "
          f"yardstick {yd:.3f} ms ({yd / f:.2f}x" + (", FUSED IS SLOWER" if f > yd else "") + f"); "
          f"{n / f / 1e6:.3f} G columns/s; spread between rounds {100 * spread:.1f} %; rounds fused "
          + " ".join(f"{v:.3f}" for v in ms["fused"]) + "; yardstick " + " ".join(f"{v:.3f}" for v in ms["yardstick"]),
          flush=True)
    eng.release(idx)
    del cols, vals
