"""Result placement when run containers far larger than 8 KiB pass through an op unchanged.

OR, XOR and ANDNOT clone a container whose key only one operand holds (RB/RoaringBitmap.java:864-896,
:1076-1113, :449-471).  The deserializer accepts run containers of up to 32,768 runs (131,074 B
serialized), so a kept record can be sixteen times a result slot.  The placement code sums kept bytes per
tile of 64 records (agg_pack, k_serialize_agg), scans them (k_place) and writes wide bitmap results
speculatively at 8192 t (OutCtx::spec, k_spec_fix).  The cases sit on the byte sums' limits:

  a7 / a8      7 / 8 maximal clones in one tile: 917,518 B / 1,048,592 B, either side of 2^20;
  b4095 / b4096  64 clones of 4,095 / 4,096 runs fill a tile: 1,048,448 B / 1,048,704 B, 128 B either side;
  c64          64 maximal clones fill a tile, the most it can hold: 8,388,736 B > 2^23, and a second tile of
               small arrays and runs whose offsets, run flags and cookie depend on the first tile's sum;
  d            8 maximal clones on records 60..67 (4 in each of two tiles) among computed and dropped records.

Every case runs in the planned form (whole key space) and the balanced form (key range set tightly), for the
cloning ops with the large containers in either operand, and for AND as the control that keeps nothing large.
All comparisons are byte-exact against the CPU oracle.
"""
import functools
import struct

import numpy as np
import pytest

import _oracle as O
from _fmt import A, B, R, encode

MAX_RUNS = 32768
TILE = 64  # records per tile of the fused placement + serialization
# (op, large containers in operand A?)
VARIANTS = [("or", True), ("xor", True), ("andnot", True), ("or", False), ("xor", False), ("and", True)]


# ---------------------------------------------------------------------------------------------------
# inputs: containers as (key, kind, cardinality, payload bytes), assembled without a pass over values
# ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _singleton_runs(nruns, first):
    """R container of `nruns` one-value runs first, first + 2, ...: -> (kind, cardinality, payload)."""
    assert 0 < nruns <= MAX_RUNS and first + 2 * (nruns - 1) <= 65535
    pairs = np.zeros(2 * nruns, dtype="<u2")
    pairs[0::2] = first + 2 * np.arange(nruns)
    return R, nruns, struct.pack("<H", nruns) + pairs.tobytes()


def _large(key, nruns):
    """The large container of a key: the even or the odd values for the maximal one (the only two containers
    of 32,768 runs), a key-dependent first value otherwise, so that neighbours differ in their bytes."""
    first = key % 2 if nruns == MAX_RUNS else (37 * key) % (65536 - 2 * nruns)
    return (key,) + _singleton_runs(nruns, first)


def _small(key, kind, vals):
    """A small container through the value-level encoder's payload rules."""
    vals = np.asarray(vals, dtype=np.uint16)
    if kind == A:
        return key, A, vals.size, vals.astype("<u2").tobytes()
    if kind == B:
        bits = np.zeros(65536, dtype=np.uint8)
        bits[vals] = 1
        return key, B, vals.size, np.packbits(bits, bitorder="little").tobytes()
    brk = np.nonzero(np.diff(vals.astype(np.int64)) != 1)[0]
    s = np.concatenate([[0], brk + 1])
    e = np.concatenate([brk, [vals.size - 1]])
    pairs = np.zeros(2 * s.size, dtype="<u2")
    pairs[0::2], pairs[1::2] = vals[s], vals[e] - vals[s]
    return key, R, vals.size, struct.pack("<H", s.size) + pairs.tobytes()


def assemble(ctrs):
    """Portable serialization (RB/RoaringArray.java:896-940) of (key, kind, cardinality, payload) containers."""
    ctrs = sorted(ctrs, key=lambda c: c[0])
    n = len(ctrs)
    has_run = any(c[1] == R for c in ctrs)
    if has_run:
        fl = bytearray((n + 7) // 8)
        for i, c in enumerate(ctrs):
            if c[1] == R:
                fl[i // 8] |= 1 << (i % 8)
        head = struct.pack("<I", 12347 | ((n - 1) << 16)) + bytes(fl)
    else:
        head = struct.pack("<II", 12346, n)
    desc = b"".join(struct.pack("<HH", c[0], c[2] - 1) for c in ctrs)
    offs = b""
    if not has_run or n >= 4:
        at = len(head) + 8 * n
        for c in ctrs:
            offs += struct.pack("<I", at)
            at += len(c[3])
    return head + desc + offs + b"".join(c[3] for c in ctrs)


def _matched(key, j):
    """Containers of operands A and B on a key both hold, by a pattern index j: results that are computed
    (array with array, array with run, run with run) and results that XOR and ANDNOT drop (identical ones)."""
    rng = np.random.default_rng(1000 + key)
    arr = np.sort(rng.choice(65536, size=int(rng.integers(1, 60)) | 1, replace=False))
    run1 = np.concatenate([np.arange(100 + key, 160 + key), np.arange(300, 340 + j)])
    run2 = np.concatenate([np.arange(130 + key, 200 + key), np.arange(20000, 20010 + j)])
    j %= 5
    if j == 0:
        return _small(key, A, arr), _small(key, A, np.sort(rng.choice(65536, size=40, replace=False)))
    if j == 1:
        return _small(key, A, np.union1d(arr, run1[::3])), _small(key, R, run1)  # A with R
    if j == 2:
        return _small(key, R, run1), _small(key, R, run2)                        # R with R
    if j == 3:
        return _small(key, A, arr), _small(key, A, arr)                          # x andnot x: dropped
    return _small(key, R, run2), _small(key, R, run2)                            # dropped, a run container


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (bitmap with the large containers, the other bitmap, key_hi of the tight key range).
    Keys are dense from 0, so a record's index is its key in both task forms (for the ops with a task per
    key of either operand), and the other bitmap holds enough keys that 2 * ub >= nkeys for every op."""
    if name in ("a7", "a8"):
        nlarge, nruns, nmatched = int(name[1]), MAX_RUNS, 8
    elif name in ("b4095", "b4096"):
        nlarge, nruns, nmatched = TILE, int(name[1:]), TILE
    elif name == "c64":
        nlarge, nruns, nmatched = TILE, MAX_RUNS, TILE
    else:
        assert name == "d"
        return _case_boundary()
    x = [_large(k, nruns) for k in range(nlarge)]
    y = []
    for j in range(nmatched):  # (b), (c): the large containers fill tile 0 exactly, these are tile 1
        ca, cb = _matched(nlarge + j, j)
        x.append(ca)
        y.append(cb)
    last = nlarge + nmatched  # a key of the other bitmap alone: a small clone after everything else
    y.append(_small(last, A, [1, 5, 9]))
    return assemble(x), assemble(y), last + 1


def _case_boundary():
    x, y = [], []
    for k in range(60):
        ca, cb = _matched(k, k)
        x.append(ca)
        y.append(cb)
    x += [_large(k, MAX_RUNS) for k in range(60, 68)]  # records 60..63 and 64..67
    for k in range(68, 82):
        ca, cb = _matched(k, k + 2)
        x.append(ca)
        y.append(cb)
    y.append(_small(82, R, np.arange(7, 90)))
    return assemble(x), assemble(y), 83


CASES = ["a7", "a8", "b4095", "b4096", "c64", "d"]


def _first_diff(got, exp):
    n = min(len(got), len(exp))
    d = np.nonzero(np.frombuffer(got, np.uint8, n) != np.frombuffer(exp, np.uint8, n))[0]
    return f"{len(got)} B vs the oracle's {len(exp)} B, first difference at byte {int(d[0]) if d.size else n}"


# ---------------------------------------------------------------------------------------------------
# the inputs themselves (no GPU)
# ---------------------------------------------------------------------------------------------------
def test_assembled_inputs_are_what_the_cases_claim():
    """assemble() agrees with the value-level encoder, the oracle reads every input back unchanged
    (or(empty, x) == x), and the tiles hold the byte counts the cases are named for."""
    small = [(3, A, np.array([1, 2, 70], dtype=np.uint16)), (5, R, np.arange(10, 500, dtype=np.uint16)),
             (9, B, np.arange(0, 20000, 3, dtype=np.uint16)), (11, R, np.arange(0, 8190, 2, dtype=np.uint16))]
    assert assemble([_small(*c) for c in small[:3]] + [(11,) + _singleton_runs(4095, 0)]) == encode(small)
    assert assemble([_small(*c) for c in small[:1]]) == encode(small[:1])
    empty = encode([])
    tile0 = {"a7": 7 * 131074, "a8": 8 * 131074, "b4095": 64 * 16382, "b4096": 64 * 16386, "c64": 64 * 131074}
    assert tile0["a7"] < 1 << 20 <= tile0["a8"] and tile0["b4095"] < 1 << 20 <= tile0["b4096"]
    assert 1 << 23 <= tile0["c64"] < 1 << 24
    for name in CASES:
        x, y, hi = case(name)
        for buf in (x, y):
            assert O.pairwise("or", empty, buf) == buf, name
            assert O.pairwise("xor", buf, empty) == buf, name
        if name in tile0:
            st = O.stats(x)
            nlarge = 7 if name == "a7" else 8 if name == "a8" else 64
            big = tile0[name]
            assert st["run"] >= nlarge and st["payload"] >= big
            # records 0 .. nlarge - 1 are the large containers: the clone-only result keeps them all
            kept = O.pairwise("andnot", x, y)
            assert O.stats(kept)["payload"] >= big
        assert len(x) <= 8_500_000


# ---------------------------------------------------------------------------------------------------
# pairwise ops
# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def engine(gpu):
    from roaringbitmap_amd import Engine
    e = Engine(0)
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def expected(name, op, large_in_a):
    x, y, _ = case(name)
    return O.pairwise(op, x, y) if large_in_a else O.pairwise(op, y, x)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["planned", "balanced"])
@pytest.mark.parametrize("name", CASES)
def test_large_clones_pairwise(engine, name, form):
    """pairwise + fetch (the fused placement + serialization, k_serialize_agg) gives the oracle's bytes."""
    e = engine
    x, y, hi = case(name)
    bx, by = e.load_pair(x, y)
    try:
        for op, large_in_a in VARIANTS:
            p, q = (bx, by) if large_in_a else (by, bx)
            if form == "planned":
                e.pairwise(op, p, q)
            else:
                e.pairwise(op, p, q, key_lo=0, key_hi=hi)
            got = e.fetch().serialize()
            exp = expected(name, op, large_in_a)
            assert got == exp, f"{name} {form} {op} large_in_a={large_in_a}: {_first_diff(got, exp)}"
    finally:
        e.release(bx)
        e.release(by)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["planned", "balanced"])
@pytest.mark.parametrize("name", ["a8", "c64"])
def test_large_clones_placement_users(engine, name, form):
    """After pairwise + serialize() (k_serialize_agg) the result statistics and the key-shard fetch, which read
    the records' placement, agree with the oracle; the same op with the statistics first (k_place, then
    k_serialize) gives the same bytes, which tells the tile sums apart from the compute kernel."""
    e = engine
    x, y, hi = case(name)
    bx, by = e.load_pair(x, y)
    rng = {} if form == "planned" else {"key_lo": 0, "key_hi": hi}
    try:
        for op in ("or", "xor", "andnot"):
            exp = expected(name, op, True)
            st_exp = O.stats(exp)
            n = st_exp["array"] + st_exp["bitmap"] + st_exp["run"]
            has_run = int((struct.unpack("<I", exp[:4])[0] & 0xFFFF) == 12347)
            assert has_run and n >= 4
            desc_base = 4 + (n + 7) // 8
            head = desc_base + 8 * n
            # statistics first: k_place + k_serialize
            e.pairwise(op, bx, by, **rng)
            st = e.result_stats()
            assert (st["containers"], st["has_run"], st["cardinality"]) == (n, has_run, st_exp["card"]), (name, op)
            assert st["payload_bytes"] == len(exp) - head
            e.serialize()
            placed = e.fetch().serialize()
            assert placed == exp, f"{name} {form} {op} k_place route: {_first_diff(placed, exp)}"
            # serialization first: k_serialize_agg
            e.pairwise(op, bx, by, **rng)
            e.serialize()
            assert e.result_stats() == st, (name, form, op)
            got = e.fetch().serialize()
            assert got == exp, f"{name} {form} {op} k_serialize_agg route: {_first_diff(got, exp)}"
            d, o, p = e.fetch_shard(n, has_run, 0, 0)
            assert d == exp[desc_base:desc_base + 4 * n], (name, form, op)
            assert o == exp[desc_base + 4 * n:head], (name, form, op)
            assert p == exp[head:], f"{name} {form} {op} shard payload: {_first_diff(p, exp[head:])}"
    finally:
        e.release(bx)
        e.release(by)


# ---------------------------------------------------------------------------------------------------
# wide ops: bitmap results written speculatively at 8192 t beside large clones
# ---------------------------------------------------------------------------------------------------
WIDE = ["horizontal_or", "buffer_or_mutable", "parallel_xor", "horizontal_xor", "xor", "or", "parallel_or"]


@functools.lru_cache(maxsize=None)
def wide_inputs(order):
    """6 bitmaps over 24 consecutive keys.  "mixed": every third key is held by one bitmap alone, as a maximal
    run container; "large_last": those 8 keys come after all the others (then no bitmap result is placed above
    8192 t).  The other keys are held by several bitmaps: arrays and bitmaps whose union passes 4,096 values
    (a bitmap result), or a few small arrays whose union stays an array."""
    rng = np.random.default_rng(6)
    nb, nkeys = 6, 24
    single = set(range(0, nkeys, 3)) if order == "mixed" else set(range(nkeys - 8, nkeys))
    bms = [[] for _ in range(nb)]
    for j, k in enumerate(range(nkeys)):
        if k in single:
            bms[(5 * j + 1) % nb].append(_large(k, MAX_RUNS))
            continue
        holders = [i for i in range(nb) if (i + j) % 3 != 0] if j % 4 else [j % nb, (j + 2) % nb]
        for i in holders:
            if j % 4 == 0:    # the union stays an array
                bms[i].append(_small(k, A, np.sort(rng.choice(65536, size=100 + 2 * i + 1, replace=False))))
            elif (i + j) % 5 == 0:
                bms[i].append(_small(k, B, np.sort(rng.choice(65536, size=4200 + 111 * i, replace=False))))
            else:
                bms[i].append(_small(k, A, np.sort(rng.choice(65536, size=1500 + 301 * i, replace=False))))
    return tuple(assemble(c) for c in bms)


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["mixed", "large_last"])
def test_large_clones_wide(engine, order):
    """Wide ops whose bitmap results are written at 8192 t before their place is known (OutCtx::spec: or,
    parallel_or, buffer_or_mutable, horizontal_or) and the XOR forms, with 131,074 B clones between them: a
    clone earlier in task order puts a later bitmap result above 8192 t, the direction k_spec_fix meets only
    then (RB/FastAggregation.java:183-289, 586-666, 823-836; RB/ParallelAggregation.java:153-214)."""
    e = engine
    bufs = list(wide_inputs(order))
    # the mix the case is about; horizontal_or (speculative placement) and the XORs keep the 8 large clones,
    # the other ORs repair them to bitmaps
    kinds = [O.stats(O.wide("horizontal_or", bufs))[k] for k in ("array", "bitmap", "run")]
    assert kinds[0] >= 2 and kinds[1] >= 8 and kinds[2] == 8, kinds
    b = e.load(bufs)
    try:
        for op in WIDE:
            exp = O.wide(op, bufs)
            e.wide(op, b)
            got = e.fetch().serialize()
            assert got == exp, f"{order} {op}: {_first_diff(got, exp)}"
    finally:
        e.release(b)
