"""A range-encoded index built on the device from a value tensor, timed
(profiles/rangebitmap_build/rangebitmap_build_perf.txt).

Shapes: 2^26 rows of uniform 27-bit values (seeded; §3.16's shape: 1,024 blocks of 27 slices, every record a
bitmap) and a smaller one, 2^22 rows of the same values.  The values sit in a torch int64 tensor on the device.
The answers are checked before anything is timed: rangebitmap_serialize(rangebitmap_build(values)) against the
package Appender's stream (the whole stream at the smaller shape, the first two blocks and 100 rows at the
larger one), and lteCardinality over the whole index against numpy at both.

Timed, by the host clock around calls that end in a synchronise, ROUNDS rounds, medians and the spread
(max - min over the median):
  build          Engine.rangebitmap_build of the device tensor (the new call), the index released after each
  parent path    what the parent commit offers for the same input: the tensor to the host, the host Appender,
                 Engine.rangebitmap_load of its stream.  Three rounds.
Modelled bytes per stage of the build: 8 n read by the max reduction, 8 n read and the workspace
(blocks x slices x 8 KiB) written by the transpose, the workspace read by the plan, the workspace read and the
arena written by the write stage.  bytes / time of a stage needs the kernel's own time, which comes from a
rocprofv3 --kernel-trace --stats run of `... once` (one build per shape, nothing else timed).
Arguments: [log2 rows of the larger shape, default 26] [once]."""
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from roaringbitmap_amd import Engine, RangeBitmap  # noqa: E402

ROUNDS = 5
LOG_ROWS = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 26
ONCE = "once" in sys.argv[1:]
BITS = 27
COPY_TBS = 6.29  # the plain-copy rate this project has recorded

eng = Engine(0)
dev = torch.device("cuda", 0)


def host_stream(values):
    app = RangeBitmap.appender((1 << BITS) - 1)
    app.add_many(values)
    return app.serialize()


def timed(f):
    eng.sync()
    torch.cuda.synchronize()
    t = time.perf_counter()
    f()
    eng.sync()
    torch.cuda.synchronize()
    return time.perf_counter() - t


def shape(log_rows, parent_rounds):
    n = 1 << log_rows
    rng = np.random.default_rng(0x2A27)
    values = rng.integers(0, 1 << BITS, n, dtype=np.uint64)
    t = torch.from_numpy(values.view(np.int64)).to(dev)
    mx = (1 << BITS) - 1
    # the answers first (also the warm-up of every path)
    h = eng.rangebitmap_build(t, mx)
    info = eng.rangebitmap_info(h)
    thr = int(values[12345]) | 1
    assert eng.rangebitmap_count(h, "lte", thr) == int((values <= thr).sum())
    if log_rows <= 22:
        assert eng.rangebitmap_serialize(h) == host_stream(values), "the stream is not the Appender's"
    else:
        part = min(n, 2 * 65536 + 100)
        hp = eng.rangebitmap_build(t[:part], mx)
        assert eng.rangebitmap_serialize(hp) == host_stream(values[:part]), "the stream is not the Appender's"
        eng.rangebitmap_release(hp)
    eng.rangebitmap_release(h)
    blocks, slices = info["blocks"], info["slices"]
    ws = blocks * slices * 8192
    arena = info["payload_bytes"]  # every record a bitmap: the slots are the payload
    print(f"shape 2^{log_rows}: {blocks} blocks x {slices} slices, workspace {ws / 1e6:.1f} MB, payload "
          f"{arena / 1e6:.1f} MB", flush=True)
    stages = {"k_rbb_max": 8 * n, "k_rbb_transpose": 8 * n + ws, "k_rbb_plan": ws, "k_rbb_write": ws + arena}
    for k, b in stages.items():
        print(f"  modelled bytes {k:16s} {b / 1e6:8.1f} MB  ({b / (COPY_TBS * 1e12) * 1e6:6.1f} us at the "
              f"{COPY_TBS} TB/s of a plain copy)", flush=True)
    total = sum(stages.values())

    def build():
        eng.rangebitmap_release(eng.rangebitmap_build(t, mx))

    def parent():
        v = t.cpu().numpy().view(np.uint64)
        eng.rangebitmap_release(eng.rangebitmap_load(host_stream(v)))

    if ONCE:
        build()
        return
    bt = [timed(build) * 1e3 for _ in range(ROUNDS)]
    pt = [timed(parent) * 1e3 for _ in range(parent_rounds)]
    bm, pm = statistics.median(bt), statistics.median(pt)
    print(f"  build        {bm:10.3f} ms per call (median of {len(bt)}, spread {100 * (max(bt) - min(bt)) / bm:.0f} %), "
          f"{total / 1e6:.1f} MB modelled -> {total / bm / 1e9:.2f} TB/s over the whole call", flush=True)
    print(f"  parent path  {pm:10.1f} ms per call (median of {len(pt)}, spread {100 * (max(pt) - min(pt)) / pm:.0f} %)",
          flush=True)
    print(f"  parent path / build = {pm / bm:.0f}x", flush=True)


shape(22, 3)
shape(LOG_ROWS, 3)
