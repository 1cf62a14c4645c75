"""Dense bitsets and masks to resident bitmaps and back, timed (profiles/bitset/bitset_perf.txt).

Shapes: 2^24, 2^27 and 2^32 bits, each at densities 2^-10, 2^-4 and 1/2 (random bits, every key present).
At 2^32 bits the packed forms alone are timed (512 MiB of words; the mask would be 4 GiB).  torch.nonzero
refuses a mask of 2^32 elements, so the yardstick there takes it in four slices of 2^30 and concatenates; at
density 1/2 (2^31 indices, 16 GiB of int64 before from_values narrows them) it is not run.

Build: Engine.from_words (int64 tensor) and Engine.from_mask (bool tensor) against the only route the engine
had before, torch.nonzero(mask).flatten() -> Engine.from_values, on the same data, the fetched bytes asserted
equal before any timing.  For the packed form the yardstick runs on the mask of those words; the unpacking is
outside the timed region.
Expansion: Engine.to_words / to_mask into device tensors against Engine.to_values(dtype=torch.int64) ->
mask.zero_(); mask[idx] = True, the masks asserted equal.

Call times by the host clock around calls that end in a synchronise; windows of at least 0.25 s; the new form
and its yardstick alternate in the same process; three rounds, medians, and the spread (max - min over the
median) stated.  Bytes moved are the launch table's: a whole-call figure, not a kernel's share
of peak.  Arguments: [largest log2 bits] [min=<smallest log2 bits>] [once: every form once per shape, for a
kernel trace]."""
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from roaringbitmap_amd import Engine  # noqa: E402

WINDOW = 0.25
ROUNDS = 3
SIZES = [24, 27, 32]
if len(sys.argv) > 1:
    SIZES = [s for s in SIZES if s <= int(sys.argv[1])]
for a in sys.argv[2:]:
    if a.startswith("min="):
        SIZES = [s for s in SIZES if s >= int(a[4:])]
ONCE = "once" in sys.argv[2:]
DENSITIES = [("2^-10", 10), ("2^-4", 4), ("1/2", 1)]

eng = Engine(0)
dev = torch.device("cuda", 0)
g = torch.Generator(device=dev)
g.manual_seed(0xB175)


def random_words(n_words, ands):
    """random 64-bit words whose bits are set with probability 2^-ands"""
    w = None
    for _ in range(ands):
        r = (torch.randint(0, 1 << 32, (n_words,), generator=g, device=dev, dtype=torch.int64) << 32) \
            | torch.randint(0, 1 << 32, (n_words,), generator=g, device=dev, dtype=torch.int64)
        w = r if w is None else w & r
    return w


def unpack(words):
    """the mask of packed words (bool, 64 elements per word), a chunk at a time"""
    out = torch.empty(words.numel() * 64, dtype=torch.bool, device=dev)
    sh = torch.arange(64, device=dev, dtype=torch.int64)
    step = 1 << 20
    for o in range(0, words.numel(), step):
        c = words[o:o + step]
        out[64 * o:64 * (o + c.numel())] = ((c[:, None] >> sh) & 1).bool().reshape(-1)
    return out


def window(f):
    """seconds per call of f over a window of at least WINDOW seconds"""
    reps = 1
    while True:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            f()
        eng.sync()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if ONCE or dt >= WINDOW or reps >= 4096:
            return dt / reps
        reps *= 4


def timed(forms):
    """forms: name -> callable; alternating, ROUNDS rounds -> name -> (median ms, spread)"""
    ms = {k: [] for k in forms}
    for _ in range(1 if ONCE else ROUNDS):
        for k, f in forms.items():
            ms[k].append(window(f) * 1e3)
    return {k: (statistics.median(v), (max(v) - min(v)) / statistics.median(v)) for k, v in ms.items()}


def line(tag, res, yard, moved):
    y = res.get(yard)
    parts = []
    for k, (m, sp) in res.items():
        s = f"{k} {m:.3f} ms (spread {100 * sp:.0f} %)"
        if k in moved:
            s += f", {moved[k] / 1e6:.1f} MB moved = {moved[k] / m / 1e6:.0f} GB/s"
        if y and k != yard:
            s += f", {y[0] / m:.2f}x the yardstick's speed"
        parts.append(s)
    print(tag + ": " + "; ".join(parts), flush=True)


for lg in SIZES:
    N = 1 << lg
    for dname, ands in DENSITIES:
        tag = f"2^{lg} bits, density {dname}"
        words = random_words(N // 64, ands)
        big = lg > 30
        yard_ok = not big or ands > 1
        mask = unpack(words) if yard_ok else None  # outside every timed region

        def positions():
            if not big:
                return torch.nonzero(mask).flatten()
            step = 1 << 30
            return torch.cat([torch.nonzero(mask[o:o + step]).flatten() + o for o in range(0, N, step)])

        def yard_build():
            eng.release(eng.from_values(positions()))

        # the bytes, once (also the warm-up of every path)
        b = eng.from_words(words)
        st = eng.batch_stats(b)
        want = eng.batch_fetch(b).serialize() if not big else None
        if yard_ok:
            y = eng.from_values(positions())
            assert eng.batch_stats(y) == st, tag
            assert big or eng.batch_fetch(y).serialize() == want, tag
            eng.release(y)
        if not big:
            m = eng.from_mask(mask)
            assert eng.batch_fetch(m).serialize() == want, tag
            eng.release(m)
        pay = st["payload_bytes"]
        forms = {"from_words": lambda: eng.release(eng.from_words(words))}
        moved = {"from_words": 3 * N // 8 + pay}
        if not big:
            forms["from_mask"] = lambda: eng.release(eng.from_mask(mask))
            moved["from_mask"] = N + N // 8 + 3 * N // 8 + pay
        if yard_ok:
            forms["nonzero+from_values"] = yard_build
        line(f"build  {tag}: C={st['containers']} (A {st['array']} / B {st['bitmap']}), cardinality "
             f"{st['cardinality']}", timed(forms), "nonzero+from_values", moved)

        # expansion
        out_mask = torch.empty(N, dtype=torch.bool, device=dev) if yard_ok else None

        def yard_expand():
            idx = eng.to_values(b, dtype=torch.int64)
            out_mask.zero_()
            out_mask[idx] = True

        w = eng.to_words(b, n_words=N // 64, dtype=torch.int64)
        assert bool(torch.equal(w, words)), tag
        del w
        if yard_ok:
            yard_expand()
            assert bool(torch.equal(out_mask, mask)), tag
        if not big:
            assert bool(torch.equal(eng.to_mask(b, n=N, dtype=torch.bool), mask)), tag
        forms = {"to_words": lambda: eng.to_words(b, n_words=N // 64, dtype=torch.int64)}
        moved = {"to_words": pay + N // 8}
        if not big:
            forms["to_mask"] = lambda: eng.to_mask(b, n=N, dtype=torch.bool)
            moved["to_mask"] = pay + N
        if yard_ok:
            forms["to_values+index_put"] = yard_expand
        line(f"expand {tag}", timed(forms), "to_values+index_put", moved)
        eng.release(b)
        del words, mask, out_mask
        torch.cuda.empty_cache()
