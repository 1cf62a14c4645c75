"""Seeded random bitmaps whose containers sit on the reference's type thresholds.

Thresholds exercised (RB/ = RoaringBitmap/src/main/java/org/roaringbitmap/):
  4096 array/bitmap boundary (RB/ArrayContainer.java:27), the run-vs-array
  threshold of 32 (RB/RunContainer.java:576,2412), toEfficientContainer ties
  (RB/RunContainer.java:2326-2335), full containers (RB/RunContainer.java:1663),
  run containers that are not space-efficient, and the 2047-run bitmap limit.
"""
import numpy as np

from _fmt import A, B, R, encode

MODES = ["a_tiny", "a_32", "a_small", "a_mid", "a_edge", "b_edge", "b_mid", "b_dense", "full_b", "full_r",
         "r_few", "r_mid", "r_many", "r_tiny", "r_tie", "r_single", "r_dense", "b_sparse_runs"]


def _choice(rng, n, k):
    return np.sort(rng.choice(n, size=k, replace=False)).astype(np.uint16)


def _runs(rng, nr, min_len=1, max_len=None, span=65536):
    """nr disjoint, non-adjacent runs inside [0, span)."""
    seg = span // nr
    vals = []
    for i in range(nr):
        hi = (i + 1) * seg - 1  # leave a gap before the next segment
        s = i * seg + int(rng.integers(0, max(1, seg // 2)))
        room = max(1, hi - s)
        ml = room if max_len is None else min(room, max_len)
        ln = int(rng.integers(min(min_len, ml), ml + 1)) if ml > 1 else 1
        vals.append(np.arange(s, min(s + ln, hi)))
    v = np.unique(np.concatenate(vals)).astype(np.uint16)
    return v


def container(rng, mode):
    """-> (kind, sorted unique uint16 values)"""
    if mode == "a_tiny":
        return A, _choice(rng, 65536, int(rng.integers(1, 32)))
    if mode == "a_32":
        return A, _choice(rng, 65536, int(rng.integers(32, 41)))
    if mode == "a_small":
        return A, _choice(rng, 65536, int(rng.integers(1, 200)))
    if mode == "a_mid":
        return A, _choice(rng, 65536, int(rng.integers(200, 4097)))
    if mode == "a_edge":
        return A, _choice(rng, 65536, int(rng.integers(4080, 4097)))
    if mode == "b_edge":
        return B, _choice(rng, 65536, int(rng.integers(4097, 4121)))
    if mode == "b_mid":
        return B, _choice(rng, 65536, int(rng.integers(4097, 60000)))
    if mode == "b_dense":
        return B, np.setdiff1d(np.arange(65536), rng.choice(65536, int(rng.integers(1, 40)), replace=False)).astype(
            np.uint16)
    if mode == "full_b":
        return B, np.arange(65536, dtype=np.uint16)
    if mode == "full_r":
        return R, np.arange(65536, dtype=np.uint16)
    if mode == "r_few":
        return R, _runs(rng, int(rng.integers(1, 9)), min_len=100)
    if mode == "r_mid":
        return R, _runs(rng, int(rng.integers(100, 600)), max_len=40)
    if mode == "r_many":  # > 2047 runs: never space-efficient as a run container
        return R, _runs(rng, int(rng.integers(2048, 3000)), max_len=6)
    if mode == "r_tiny":  # few short runs, small cardinality
        return R, _runs(rng, int(rng.integers(1, 8)), max_len=4)
    if mode == "r_tie":  # runs of exactly 2 values: 2+4r == 2+2c (toEfficientContainer keeps R)
        nr = int(rng.integers(1, 40))
        starts = np.sort(rng.choice(65536 // 4, nr, replace=False)) * 4
        return R, np.unique(np.concatenate([starts, starts + 1])).astype(np.uint16)
    if mode == "r_single":  # singleton runs: array is smaller than runs
        nr = int(rng.integers(1, 60))
        return R, (np.sort(rng.choice(65536 // 2, nr, replace=False)) * 2).astype(np.uint16)
    if mode == "r_dense":  # long runs separated by small gaps
        gaps = np.sort(rng.choice(65536, int(rng.integers(1, 30)), replace=False))
        return R, np.setdiff1d(np.arange(65536), gaps).astype(np.uint16)
    if mode == "b_sparse_runs":  # bitmap whose content has ~1000 runs
        return B, _runs(rng, 1000, min_len=6, max_len=30)
    raise ValueError(mode)


def bitmap(rng, keys, modes=None, p_present=0.8):
    ctrs = []
    for k in keys:
        if rng.random() > p_present:
            continue
        m = modes[int(rng.integers(len(modes)))] if modes else MODES[int(rng.integers(len(MODES)))]
        kind, vals = container(rng, m)
        ctrs.append((int(k), kind, vals))
    return encode(ctrs)


def perturbed_pair(rng, keys):
    """Two bitmaps whose shared keys hold identical or near-identical containers
    (empty XOR/ANDNOT results, results landing exactly on thresholds)."""
    c1, c2 = [], []
    for k in keys:
        kind, vals = container(rng, MODES[int(rng.integers(len(MODES)))])
        c1.append((int(k), kind, vals))
        r = rng.random()
        if r < 0.3:
            c2.append((int(k), kind, vals))  # identical
        elif r < 0.6:
            drop = rng.choice(vals.size, size=min(vals.size - 1, int(rng.integers(1, 40))), replace=False) \
                if vals.size > 1 else []
            v2 = np.delete(vals, drop)
            k2 = kind if not (kind == B and v2.size <= 4096) else A
            c2.append((int(k), k2 if kind != R else R, v2))
        else:
            kind2, v2 = container(rng, MODES[int(rng.integers(len(MODES)))])
            c2.append((int(k), kind2, v2))
    return encode(c1), encode(c2)


def sparse_keys(rng):
    """9,000 to 10,000 sorted keys: more tasks than the 8,192 waves an MI355X holds, so some wave of every
    one-wave-per-task kernel takes a second task.  0..299 dense (result tiles 64, 128, 192, 256 and the plan
    workgroup 0 / 1 border), a dense block of 6,000 keys in the middle, blocks of 1, 2, 3 and 5 adjacent
    keys at random places, keys 65534 and 65535, and a hole of 316 keys around one whole 256-key plan
    workgroup (2 or 3) with a key on either side of the hole."""
    g = int(rng.integers(2, 4))
    hole_lo, hole_hi = 256 * g - 30, 256 * (g + 1) + 30  # [hole_lo, hole_hi) holds no key
    mid = int(rng.integers(26000, 34000))
    have = np.zeros(65536, dtype=bool)
    have[:300] = True
    have[mid:mid + 6000] = True
    have[[hole_lo - 1, hole_hi, 65534, 65535]] = True
    target = int(rng.integers(9300, 9700))
    while int(have.sum()) < target:
        n = (1, 2, 3, 5)[int(rng.integers(4))]
        k = int(rng.integers(0, 65536 - n))
        if k + n <= hole_lo or k >= hole_hi:
            have[k:k + n] = True
    return np.nonzero(have)[0]


def empty_workgroup(keys):
    """The first 256-key plan workgroup without a key that has keys on both sides, or None."""
    per = np.bincount(np.asarray(keys) >> 8, minlength=256)
    busy = np.nonzero(per)[0]
    for w in range(int(busy[0]) + 1, int(busy[-1])):
        if per[w] == 0:
            return w
    return None


def tiny_values(rng, r):
    """1 to 8 values: below 2,000 only (r < 1/3), above 63,000 only (r < 2/3), or both"""
    n = int(rng.integers(1, 9))
    if r < 1 / 3:
        v = rng.integers(0, 2000, n)
    elif r < 2 / 3:
        v = rng.integers(63000, 65536, n)
    else:
        n = max(n, 2)
        nl = int(rng.integers(1, n))
        v = np.concatenate([rng.integers(0, 2000, nl), rng.integers(63000, 65536, n - nl)])
    return np.unique(v).astype(np.uint16)


def sparse_bitmap(rng, keys, heavy_every=97, run_every=0):
    """A many-key bitmap of tiny array containers (see tiny_values: an addOffset of a few hundred leaves one part
    empty, a whole output key empty, or both parts live); every heavy_every-th key holds a random MODES
    container, so bitmaps, run containers above 2,047 runs and full containers land on late tasks too.
    run_every: every run_every-th tiny container is a run container of one or two short runs."""
    ctrs = []
    for i, k in enumerate(keys):
        if i % heavy_every == heavy_every - 1:
            kind, vals = container(rng, MODES[int(rng.integers(len(MODES)))])
        elif run_every and i % run_every == 0:
            s = int(rng.integers(0, 2000))
            vals = np.arange(s, s + int(rng.integers(1, 7)))
            if rng.random() < 0.5:
                s = int(rng.integers(63000, 65500))
                vals = np.concatenate([vals, np.arange(s, s + int(rng.integers(1, 7)))])
            kind, vals = R, vals.astype(np.uint16)
        else:
            kind, vals = A, tiny_values(rng, rng.random())
        ctrs.append((int(k), kind, vals))
    return encode(ctrs)


def sparse_bsi(rng, n_keys=6000, nbits=20):
    """(keys, cols, vals) of a many-key bit-sliced index: ascending distinct columns and their values.

    Keys in the style of sparse_keys: 0..299 dense, a hole of 316 keys around one whole 256-key plan workgroup
    (2 or 3) with a key on either side, a dense middle block of n_keys // 2 keys, blocks of 1, 2, 3 and 5
    adjacent keys at random places up to n_keys in all, and keys 65534 and 65535.
    Columns per key (ebM's containers): the union of two tiny_values draws (2 to 16 values, low, high or both,
    so that a mid-range predicate usually splits a key); every third key 4 to 11 adjacent values below 2,000
    and 1 to 6 above 63,000 (a two-run run container once run-optimized); every 97th key a random MODES
    container (bitmaps, run containers above 2,047 runs, full containers).
    Values: uniform in [0, 2^nbits), but under keys with key % 3 == 1 the clustered
    (low // 3000 + 37 * (key % 7)) % 2^nbits: long runs in the low slices, no container at all in the high
    ones, and a few values that thousands of columns share; under every other two-run key the uniform values
    ascend with the column, so that < and > select a prefix or suffix of the runs (a run result that is no
    clone of an input once the index is run-optimized)."""
    g = int(rng.integers(2, 4))
    hole_lo, hole_hi = 256 * g - 30, 256 * (g + 1) + 30  # [hole_lo, hole_hi) holds no key
    mid = int(rng.integers(26000, 34000))
    have = np.zeros(65536, dtype=bool)
    have[:300] = True
    have[mid:mid + n_keys // 2] = True
    have[[hole_lo - 1, hole_hi, 65534, 65535]] = True
    while int(have.sum()) < n_keys:
        n = (1, 2, 3, 5)[int(rng.integers(4))]
        k = int(rng.integers(0, 65536 - n))
        if k + n <= hole_lo or k >= hole_hi:
            have[k:k + n] = True
    keys = np.nonzero(have)[0]
    cols, vals = [], []
    for i, k in enumerate(keys):
        k = int(k)
        if i % 97 == 96:
            low = container(rng, MODES[int(rng.integers(len(MODES)))])[1].astype(np.int64)
        elif i % 3 == 0:
            s, t = int(rng.integers(0, 1989)), int(rng.integers(63000, 65530))
            low = np.concatenate([np.arange(s, s + int(rng.integers(4, 12))), np.arange(t, t + int(rng.integers(1, 7)))])
        else:
            low = np.union1d(tiny_values(rng, rng.random()), tiny_values(rng, rng.random())).astype(np.int64)
        if k % 3 == 1:
            v = (low // 3000 + 37 * (k % 7)) % (1 << nbits)
        else:
            v = rng.integers(0, 1 << nbits, low.size)
            if i % 6 == 0:  # ascending with the column: < and > select a prefix / suffix of the two runs
                v = np.sort(v)
        cols.append((k << 16) + low)
        vals.append(v)
    return keys, np.concatenate(cols).astype(np.int64), np.concatenate(vals).astype(np.int64)


def random_values(rng, n, universe=1 << 32):
    return rng.integers(0, universe, size=n, dtype=np.int64).astype(np.uint32)


# Cardinalities around the 8 values of a 16 B vector: an array slot is padded to 16 B with copies of its last
# value, and ops read whole vectors of it.  One container per cardinality, keys 0..7.
PAD_CARDS = (1, 2, 7, 8, 9, 15, 16, 17)


def pad_lows(rng, shifted=False):
    """-> per key of PAD_CARDS, that many sorted low halves in [100, 60100), at least 3 apart (away from 0 and
    65535, never adjacent: such a set is an array container under every type rule); shifted: every second
    value of a key moved up by one, which keeps them at least 2 apart"""
    out = []
    for c in PAD_CARDS:
        lows = np.sort(rng.choice(20000, c, replace=False)).astype(np.int64) * 3 + 100
        if shifted:
            lows[1::2] += 1
        out.append(lows)
    return out
