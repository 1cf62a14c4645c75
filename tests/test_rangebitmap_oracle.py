"""The range-encoded index on the CPU: the oracle (_rangebitmap.py, RB/RangeBitmap.java restated) against the
reference's own known answers, against brute force over the values, and against the claim the device code
rests on, that a result's bytes are a function of its row set alone: O.from_values(rows, True).  The
package's vectorised Appender is held to the oracle's byte for byte.  No GPU.
"""
import gzip
import json
import os

import numpy as np
import pytest

import _fmt
import _oracle as O
import _rangebitmap as RBO
import roaringbitmap_amd as rb

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rangebitmap")
M64 = (1 << 64) - 1
MIN_VALUE = 1 << 63  # Long.MIN_VALUE as an unsigned pattern
OPS1 = ("lte", "lt", "gt", "gte", "eq", "neq")


def j(x):
    """a Java long as its unsigned 64-bit pattern"""
    return int(x) & M64


def pkg_stream(values, max_value):
    app = rb.RangeBitmap.appender(max_value)
    app.add_many(np.array([j(v) for v in values], dtype=np.uint64))
    return app.serialize()


def rows_of_bytes(buf):
    return O.to_values(buf).astype(np.int64)


def regression_values():
    with gzip.open(os.path.join(GOLDEN, "regression_values_u32le.gz"), "rb") as f:
        return np.frombuffer(f.read(), dtype="<u4").astype(np.uint64)


# ---------------------------------------------------------------------------------------------------------
# typing: the replayed chain gives the bytes of the row set
# ---------------------------------------------------------------------------------------------------------
def ctx_bytes(kind, rows_by_key):
    """a context with one container of the given kind per key"""
    return _fmt.encode([(k, kind, np.asarray(v)) for k, v in rows_by_key.items()])


def typing_cases():
    alt = np.arange(8194) % 2  # eq(0): 4,097 scattered rows, a bitmap; the first 8,192 rows: 4,096, an array
    out = [
        ("4096", alt[:8192], 1, [("eq", 0, 0), ("neq", 0, 0), ("lte", 0, 0), ("gt", 0, 0)]),
        ("4097", alt, 1, [("eq", 0, 0), ("neq", 1, 0), ("lte", 0, 0), ("between", 1, 1)]),
        ("full", np.zeros(65536 + 100, dtype=np.int64), 3, [("eq", 0, 0), ("lte", 2, 0), ("neq", 1, 0), ("gte", 0, 0),
                                                            ("between", 1, 2), ("gt", 0, 0)]),
        ("cut", np.arange(65536 + 100) % 7, 6, [("lte", 3, 0), ("gt", 3, 0), ("eq", 6, 0), ("neq", 6, 0),
                                                ("between", 2, 4), ("between", 1, 6), ("lte", 6, 0)]),
        # 2 c against 2 + 4 r: rows {0, 1, 2} in one run tie at 6 and stay an array, {0 .. 3} become a run
        ("tie", [5, 5, 5, 9, 5, 9], 9, [("eq", 5, 0), ("lte", 5, 0), ("between", 5, 5), ("neq", 9, 0)]),
        ("tie4", [5, 5, 5, 5, 9], 9, [("eq", 5, 0), ("between", 4, 6)]),
    ]
    return out


@pytest.mark.parametrize("name,values,max_value,queries", typing_cases(), ids=[c[0] for c in typing_cases()])
def test_typed_replay_is_from_values(name, values, max_value, queries):
    """new BitmapContainer(bits, -1)[.iand(context)].repairAfterLazy().runOptimize() per key, replayed type by
    type, serializes to O.from_values(rows, True): with no context and with array, bitmap and run contexts."""
    idx = RBO.Index(RBO.build(values, max_value))
    n = idx.max
    half = np.arange(0, min(n, 65536), 2)
    contexts = [None,
                ctx_bytes(_fmt.A, {0: half[:3000]}),
                ctx_bytes(_fmt.B, {0: np.arange(0, min(n, 65536), 1 if n < 20000 else 3)} if n > 4096 * 3 else {0: half}),
                ctx_bytes(_fmt.R, {0: np.arange(0, min(n, 40000))}),
                ctx_bytes(_fmt.R, {0: np.arange(65536), 1: np.arange(65536)})]  # full containers, past the cut
    seen = set()
    for op, a, b in queries:
        for cb in contexts:
            if op == "between" and cb is not None:
                continue
            if cb is not None and op in ("gte", "lte") and RBO.nlz(a) < RBO.nlz(idx.mask):
                continue  # a clone of the context, not typed by the chain
            got = RBO.query_typed(idx, op, a, b, cb)
            rows = rows_of_bytes(got)
            if op == "gte" and a == 0:
                continue  # bitmapOfRange / clone
            assert got == O.from_values(rows, True), (name, op, a, b)
            seen.update(_fmt.kinds(got))
    if name in ("4096", "tie"):
        assert _fmt.A in seen
    if name == "4097":
        assert _fmt.B in seen
    if name in ("full", "tie4"):
        assert _fmt.R in seen


def test_typing_lands_on_the_boundaries():
    idx = RBO.Index(RBO.build(np.arange(8194) % 2, 1))
    assert [(c[1], c[2]) for c in _fmt.decode(RBO.query_typed(idx, "eq", 0))] == [(_fmt.B, 4097)]
    idx = RBO.Index(RBO.build(np.arange(8192) % 2, 1))
    assert [(c[1], c[2]) for c in _fmt.decode(RBO.query_typed(idx, "eq", 0))] == [(_fmt.A, 4096)]
    idx = RBO.Index(RBO.build(np.zeros(65536 + 100, dtype=np.int64), 3))
    assert [(c[0], c[1], c[2], c[4]) for c in _fmt.decode(RBO.query_typed(idx, "eq", 0))] == \
        [(0, _fmt.R, 65536, 1), (1, _fmt.R, 100, 1)]  # a full block, and the cut last block as one run
    idx = RBO.Index(RBO.build([5, 5, 5, 9, 5, 9], 9))
    assert _fmt.kinds(RBO.query_typed(idx, "eq", 5)) == [_fmt.A]  # {0, 1, 2, 4}: 8 > 2 + 4 * 2 is false
    idx = RBO.Index(RBO.build([5, 5, 5, 9], 9))
    assert _fmt.kinds(RBO.query_typed(idx, "eq", 5)) == [_fmt.A]  # the tie 2 c == 2 + 4 r
    idx = RBO.Index(RBO.build([5, 5, 5, 5, 9], 9))
    assert _fmt.kinds(RBO.query_typed(idx, "eq", 5)) == [_fmt.R]


def test_shortcuts_keep_their_own_types():
    """a threshold above the mask: bitmapOfRange(0, max) (run containers, also for 2 rows), the context's own
    bytes (not run-optimised), or empty (:427-429, :459-461, :552-554, :583-585); gte(0) alike (:294-308)"""
    idx = RBO.Index(RBO.build([1, 2], 3))
    assert RBO.query_typed(idx, "lte", 4) == O.bitmap_of_range(0, 2) != O.from_values([0, 1], True)
    assert RBO.query_typed(idx, "neq", 100) == O.bitmap_of_range(0, 2)
    assert RBO.query_typed(idx, "gte", 0) == O.bitmap_of_range(0, 2)
    ctx = O.from_values(np.arange(0, 50), False)  # an array that runOptimize would turn into a run
    for op, a in (("lte", 4), ("neq", 9), ("gte", 0), ("lt", M64)):
        assert RBO.query_typed(idx, op, a, 0, ctx) == ctx, op
    for op, a in (("gt", 4), ("eq", 4), ("lt", 0)):
        assert RBO.query_typed(idx, op, a, 0, ctx) == O.from_values([], False), op
        assert RBO.query_typed(idx, op, a) == O.from_values([], False), op
    assert RBO.query_count(idx, "lte", 4, 0, ctx) == 50 and RBO.query_count(idx, "gte", 0, 0, ctx) == 50
    assert RBO.query_count(idx, "lte", 4) == 2 and RBO.query_count(idx, "gt", 4) == 0


# ---------------------------------------------------------------------------------------------------------
# the reference's known answers (RangeBitmapTest.java)
# ---------------------------------------------------------------------------------------------------------
def check(idx, op, a, b, rows, count=True):
    got = rows_of_bytes(RBO.query_typed(idx, op, j(a), j(b)))
    assert got.tolist() == sorted(rows), (op, a, b)
    if count:
        assert RBO.query_count(idx, op, j(a), j(b)) == len(rows), (op, a, b)


def test_extreme_values():
    """testExtremeValues (:659-701), every line: the compare is unsigned"""
    idx = RBO.Index(RBO.build([0, MIN_VALUE, j(-1)], j(-1)))
    assert idx.slice_count == 64
    for op, a, rows in [("gt", -1, []), ("gte", -1, [2]), ("lte", -1, [0, 1, 2]), ("lte", -2, [0, 1]),
                        ("lt", -1, [0, 1]), ("lt", -2, [0, 1]), ("lte", MIN_VALUE, [0, 1]), ("lt", MIN_VALUE, [0]),
                        ("gt", MIN_VALUE, [2]), ("gte", MIN_VALUE, [1, 2]), ("lte", 0, [0]), ("lt", 0, []),
                        ("gte", 0, [0, 1, 2]), ("gt", 0, [1, 2])]:
        check(idx, op, a, 0, rows)
    for op, a, rows in [("eq", 2, []), ("neq", 2, [0, 1, 2]), ("eq", 0, [0]), ("eq", MIN_VALUE, [1]), ("eq", -1, [2]),
                        ("neq", 0, [1, 2]), ("neq", MIN_VALUE, [0, 2]), ("neq", -1, [0, 1])]:
        check(idx, op, a, 0, rows, count=False)


def test_between_1_and_2():
    """testBetween1 (:480-497), testBetween2 (:500-520)"""
    idx = RBO.Index(RBO.build(range(10), 10))
    for a, b, lo, hi in [(0, 10, 0, 10), (1, 10, 1, 10), (1, 9, 1, 10), (2, 8, 2, 9), (3, 7, 3, 8)]:
        check(idx, "between", a, b, list(range(lo, hi)))
    idx = RBO.Index(pkg_stream(range(10 + 0x10000), 10 + 0x10000))
    for a, b, lo, hi in [(0, 10, 0, 11), (1, 10, 1, 11), (1, 9, 1, 10), (2, 8, 2, 9), (3, 7, 3, 8),
                         (0x10000 - 5, 0x10000 + 5, 0x10000 - 5, 0x10000 + 6)]:
        check(idx, "between", a, b, list(range(lo, hi)))


def test_between_3():
    """testBetween3 (:523-553): four extreme values, then 2^20 sequential ones, 64 slices"""
    head = [-4616189618054758400, 4601552919265804287, -4586634745500139520, 4571364728013586431]
    n = 1 << 20
    idx = RBO.Index(pkg_stream(head + list(range(n)), -4586634745500139520))
    seq = list(range(4, n + 4))
    max_long = (1 << 63) - 1
    for a, b, rows in [(-4620693217682128896, -4616189618054758400, [0]), (1, 42, list(range(5, 47))),
                       (0, 4571364728013586431, [3] + seq), (0, 4601552919265804287, [1, 3] + seq),
                       (max_long, -4616189618054758400, [0]), (max_long, -4586634745500139520, [0, 2]),
                       (0, -1, list(range(n + 4))), (4571364728013586431, -4586634745500139520, [0, 1, 2, 3]),
                       (max_long, -1, [0, 2]), (0, max_long, [1, 3] + seq), (-42, -1, [])]:
        check(idx, "between", a, b, rows)


def test_between_4():
    """testBetween4 (:556-613)"""
    with open(os.path.join(GOLDEN, "between4_values.json")) as f:
        values = json.load(f)["values"]
    idx = RBO.Index(RBO.build(values, M64))
    check(idx, "between", -4620693217682128896, -4616189618054758400, [0])


def test_regression_586_and_588():
    """regressionTestIssue586 (:790-798, :812-818): one value under a 64-slice mask; between(low, high) is
    gte(low, lte(high)) and holds the row.  regressionTestIssue588 (:801-810) is about
    RoaringBitmap.intersects(min, sup) and has no RangeBitmap in it: the same fact through the range selection."""
    for low, high, value in [(0x0FFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFF0, 0xFFFFFFFFFFFFFF0),
                             (0x0FFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFF0, 0xFFFFFFFFFFFFFFF0),
                             (0x0FFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFF1, 0xFFFFFFFFFFFFFFF0),
                             (0, 10_000_000_000, 10_000_000)]:
        idx = RBO.Index(RBO.build([value], M64))
        lte = RBO.query_typed(idx, "lte", high)
        assert rows_of_bytes(RBO.query_typed(idx, "gte", low, 0, lte)).tolist() == [0]
        check(idx, "between", low, high, [0])
    one = O.from_values([27470832], False)
    for lo in (27459584, 27459583):
        assert O.to_values(O.range_op("select", [one], lo, 27597418)).size == 1


def test_between_regression_fixture():
    """betweenRegressionTest (:50-65) on rangebitmap_regression.txt: between(x, x + 1) is eq(x) | eq(x + 1)"""
    values = regression_values()
    assert values.size == 66085
    idx = RBO.Index(pkg_stream(values, 2175288))
    assert idx.max_key == 2
    for i in range(4):
        lo = 263501 + i
        want = np.union1d(rows_of_bytes(RBO.query_typed(idx, "eq", lo)), rows_of_bytes(RBO.query_typed(idx, "eq", lo + 1)))
        got = rows_of_bytes(RBO.query_typed(idx, "between", lo, lo + 1))
        assert got.tolist() == want.tolist() == RBO.brute_rows(values, idx.max, "between", lo, lo + 1).tolist()
        assert RBO.query_count(idx, "between", lo, lo + 1) == want.size


@pytest.mark.parametrize("max_value", [1, 0xF, 0xFF, 0xFFF, 0xFFFF, 0xFFFFF, 0xFFFFFF, 0xFFFFFFF, 0xFFFFFFFF,
                                       0xFFFFFFFFF, 0xFFFFFFFFFF, 0xFFFFFFFFFFF, 0xFFFFFFFFFFFF, 0xFFFFFFFFFFFFF,
                                       0xFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF])
def test_serialize_empty(max_value):
    """testSerializeEmpty (:291-299): an index without rows is its 10 header bytes and answers empty"""
    a, p = RBO.Appender(max_value), rb.RangeBitmap.appender(max_value)
    assert a.serialized_size() == p.serializedSizeInBytes() == 10
    buf = a.serialize()
    assert buf == p.serialize() and len(buf) == 10 and buf[3] == max_value.bit_length()
    idx = RBO.Index(buf)
    assert rows_of_bytes(RBO.query_typed(idx, "lte", MIN_VALUE)).size == 0
    assert RBO.query_count(idx, "lte", MIN_VALUE) == 0


@pytest.mark.parametrize("value", [1, 2, 3, 4, 7, 8, 15, 16, 31, 32, 63, 64])
def test_extremely_small_and_modulo_65536(value):
    """extremelySmallBitmapTest (:763-772), testModulo65536 (:776-787)"""
    for count in (1, 65537):
        idx = RBO.Index(pkg_stream([value] * count, value))
        for op, a, b in (("gte", value, 0), ("lte", value, 0), ("between", value, value)):
            assert rows_of_bytes(RBO.query_typed(idx, op, a, b)).size == count
            assert RBO.query_count(idx, op, a, b) == count


@pytest.mark.parametrize("size", [0, 0xFFFF, 0x10001])
def test_insert_contiguous_values(size):
    """testInsertContiguousValues (:69-93) at the sizes 0, 0xFFFF and 0x10001"""
    idx = RBO.Index(pkg_stream(range(size), size))
    assert rows_of_bytes(RBO.query_typed(idx, "lte", size)).tolist() == list(range(size))
    upper = 1
    while upper < size:
        check(idx, "lte", upper, 0, list(range(upper + 1)))
        check(idx, "lt", upper, 0, list(range(upper)))
        check(idx, "eq", upper, 0, [upper], count=False)
        check(idx, "gte", upper, 0, list(range(upper, size)))
        check(idx, "gt", upper, 0, list(range(upper + 1, size)))
        upper *= 10


def test_contextual_evaluation_on_empty_range():
    """testContextualEvaluationOnEmptyRange (:644-656)"""
    idx = RBO.Index(RBO.Appender(10_000_000).serialize())
    ctx = O.bitmap_of_range(0, 100_000)
    for op in ("lte", "lt", "gt", "gte"):
        assert rows_of_bytes(RBO.query_typed(idx, op, 10, 0, ctx)).size == 0
        assert RBO.query_count(idx, op, 10, 0, ctx) == 0


# ---------------------------------------------------------------------------------------------------------
# the flag-faithful replay against brute force
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_replay_against_brute_force(seed):
    """Every op with and without a context on random values; the `empty` / `full` flags carried across blocks
    never change a row; each cardinality is the size of its bitmap.  The context keeps to rows below maxRid in
    the last block and, for betweenCardinality, to one container: the two places where the reference's counts
    are not the sizes of its bitmaps are pinned in the tests below."""
    rng = np.random.default_rng(seed)
    bits = [3, 9, 17][seed - 1]
    n = 2 * 65536 + 1000 * seed
    values = rng.integers(0, 1 << bits, n).astype(np.uint64)
    values[65536:65536 + 30000] |= np.uint64(1)  # a block whose mask lacks slice 0
    if seed == 3:
        values[:65536] = (1 << bits) - 1  # a block with no container at all
    idx = RBO.Index(pkg_stream(values, (1 << bits) - 1))
    assert np.array_equal(idx.values(), values)
    ctx_rows = np.unique(np.concatenate([rng.integers(0, 65536, 3000), np.arange(2 * 65536, 2 * 65536 + 500),
                                         np.arange(5 * 65536, 5 * 65536 + 70000)]))  # skips key 1, runs past the index
    ctx = O.from_values(ctx_rows, True)
    one = O.from_values(np.arange(65536 + 10, 65536 + 40000), True)
    stored = int(values[7])
    thresholds = [0, 1, stored, max(stored - 1, 0), stored + 1, (1 << bits) - 1, 1 << bits, M64]
    for op in OPS1:
        for t in thresholds:
            for cb, crows in ((None, None), (ctx, ctx_rows), (one, np.arange(65536 + 10, 65536 + 40000))):
                want = RBO.brute_rows(values, n, op, t, 0, crows)
                top = 1 << bits
                if cb is not None and ((op == "gte" and t == 0) or (op in ("lte", "neq") and t >= top) or
                                       (op == "lt" and t > top)):
                    want = np.asarray(crows)  # context.clone(): rows past maxRid included, as the reference has it
                got = rows_of_bytes(RBO.query_typed(idx, op, t, 0, cb))
                assert np.array_equal(got, want), (op, t, cb is not None)
                assert RBO.query_count(idx, op, t, 0, cb) == want.size, (op, t, cb is not None)
    for a, b in [(0, stored), (stored, stored), (stored, stored + 5), (1, (1 << bits) - 1), (5, 2), (2, 1 << bits),
                 (1 << bits, M64), (stored, M64)]:
        want = RBO.brute_rows(values, n, "between", a, b)
        if a >= 1 << bits:  # a minimum above the mask falls to lte(max) (:112-114), not to the empty bitmap
            want = RBO.brute_rows(values, n, "lte", b)
        assert np.array_equal(rows_of_bytes(RBO.query_typed(idx, "between", a, b)), want), (a, b)
        assert RBO.query_count(idx, "between", a, b) == want.size
        wc = np.intersect1d(want, np.arange(65536 + 10, 65536 + 40000))
        assert RBO.query_count(idx, "between", a, b, one) == wc.size, (a, b)


def test_counts_that_are_not_the_bitmaps_size():
    """Two divergences of the reference's *Cardinality forms from its bitmap forms, found by the replay and
    followed by the device code:
    gtCardinality / gteCardinality with a context count container.andNot(bits) (:659-661), which keeps the
    context's rows at or past maxRid inside the last block, while gt(t, context) flips rows [0, limit) only;
    DoubleEvaluation.count(lower, upper, context) (:977-1014) never advances contextPos, so every key from the
    context's first to its last is intersected with the context's FIRST container."""
    values = np.arange(100) % 8
    idx = RBO.Index(RBO.build(values, 7))
    ctx = O.from_values([1, 2, 3, 150, 151], False)  # 150, 151: past maxRid = 100, inside block 0
    assert rows_of_bytes(RBO.query_typed(idx, "gt", 1, 0, ctx)).tolist() == [2, 3]
    assert RBO.query_count(idx, "gt", 1, 0, ctx) == 4
    assert RBO.query_count(idx, "gte", 2, 0, ctx) == 4
    assert RBO.query_count(idx, "lte", 1, 0, ctx) == 1  # andCardinality: the bits end at maxRid

    values = np.concatenate([np.zeros(65536, dtype=np.int64), np.full(65536, 5), np.full(10, 5)])
    idx = RBO.Index(pkg_stream(values, 7))
    ctx = O.from_values([7, 8, 65536 + 1, 2 * 65536 + 3], False)  # first container {7, 8}
    assert RBO.brute_rows(values, idx.max, "between", 4, 6, [7, 8, 65537, 131075]).size == 2
    assert RBO.query_count(idx, "between", 4, 6, ctx) == 0 + 2 + 2  # {7, 8} against blocks 0, 1, 2
    assert RBO.query_count(idx, "between", 4, 6, O.from_values([65536 + 9], False)) == 1  # one container: exact


# ---------------------------------------------------------------------------------------------------------
# the package's Appender
# ---------------------------------------------------------------------------------------------------------
def appender_inputs():
    rng = np.random.default_rng(7)
    n = 65536 + 300
    dense = rng.integers(0, 1 << 9, n)
    sparse = np.where(rng.random(n) < 0.02, rng.integers(0, 1 << 9, n), (1 << 9) - 1)  # arrays in slices >= 5
    few = np.full(n, (1 << 9) - 1)
    few[rng.choice(65536, 3000, replace=False)] = 0  # bitmap records of 3,000 scattered rows in slices 0-4
    runs = (np.arange(n) // 700) % 512
    full = np.zeros(n, dtype=np.int64)  # every slice full in block 0: cardinality field 0
    return {"dense": (dense, 511), "sparse": (sparse, 511), "few": (few, 511), "runs": (runs, 511), "full": (full, 511),
            "one_slice": (rng.integers(0, 2, 70000), 1), "wide": (rng.integers(0, 1 << 62, 500) * 4, M64),
            "masks": (np.where(np.arange(n) < 65536, 3, 12), 15)}


@pytest.mark.parametrize("name", list(appender_inputs()))
def test_package_appender_is_the_oracles(name):
    values, max_value = appender_inputs()[name]
    want = RBO.build(values, max_value)
    got = pkg_stream(values, max_value)
    assert got == want
    one = rb.RangeBitmap.appender(max_value)
    for v in values[:300]:
        one.add(int(v))
    assert one.serialize() == RBO.build(values[:300], max_value)
    if name == "few":  # the trap: a bitmap record of at most 4,096 values; "full": the wrapped cardinality
        assert any(t == RBO.BITMAP and s == 3000 for t, s, _ in RBO.Index(want).records)
    if name == "full":
        assert any(t == RBO.RUN and s == 1 for t, s, _ in RBO.Index(want).records)


def test_bitmap_record_of_a_full_block_stores_zero():
    """slices 0-4 of 65,536 rows in 2,048 runs or more stay bitmaps (2 + 4 r >= 8192); none is full here, but a
    cardinality of 65,536 would be cast to 0 (:1565): forced through a hand-written record in the host tests.
    Here: the size field is the cardinality mod 65,536 for the bitmaps the Appender does write."""
    values = np.arange(65536) % 2  # slice 0: 32,768 runs -> a bitmap of 32,768
    idx = RBO.Index(pkg_stream(values, 1))
    assert [(t, s) for t, s, _ in idx.records] == [(RBO.BITMAP, 32768)]


def test_appender_refuses_values_outside_the_mask():
    app = rb.RangeBitmap.appender(10)  # mask 15
    app.add(15)
    with pytest.raises(rb.IllegalArgumentException, match="16 too large"):
        app.add(16)
    with pytest.raises(rb.IllegalArgumentException, match="too large"):
        app.add_many(np.array([1, 2, 99, 3], dtype=np.uint64))
    assert app.serialize() == RBO.build([15, 1, 2], 10)  # the values before the refused one were added
    with pytest.raises(ValueError):
        RBO.Appender(10).add(16)


def test_appender_flush_then_add_and_clear():
    """serializedSizeInBytes() appends the unfinished block (flush, :1535-1541): rows added afterwards start a
    new key while rid goes on, as the reference has it; clear() starts over"""
    a, p = RBO.Appender(255), rb.RangeBitmap.appender(255)
    for v in range(10):
        a.add(v)
    p.add_many(np.arange(10))
    assert a.serialized_size() == p.serializedSizeInBytes()
    for v in range(20, 30):
        a.add(v)
    p.add_many(np.arange(20, 30))
    assert a.serialize() == p.serialize()
    p.clear()
    p.add_many(np.arange(5))
    assert p.serialize() == RBO.build(range(5), 255)


# ---------------------------------------------------------------------------------------------------------
# the fast model of the GPU tests
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [4, 5])
def test_fast_model_is_the_replay(seed):
    """model_bytes / model_count (from the values, what the GPU tests compare with) against the typed,
    flag-faithful replay: contexts that lack blocks, end below the last block, reach past maxRid, inside
    the last block too, with array, bitmap and run containers"""
    rng = np.random.default_rng(seed)
    bits = 6 if seed == 4 else 12
    n = 3 * 65536 + 100
    values = rng.integers(0, 1 << bits, n).astype(np.uint64)
    values[65536:2 * 65536] = (1 << bits) - 1  # no container at all
    values[2 * 65536:2 * 65536 + 40000] &= np.uint64(~1 & M64)
    buf = pkg_stream(values, (1 << bits) - 1)
    idx = RBO.Index(buf)
    top = (1 << bits) - 1
    ctxs = [None, O.from_values([], False),
            O.from_values(np.concatenate([rng.choice(65536, 3000, replace=False), 2 * 65536 + np.arange(0, 65536, 2)]), True),
            O.from_values(np.concatenate([np.arange(100, 60000), 65536 + rng.choice(65536, 9000, replace=False)]), True),
            O.from_values(np.concatenate([np.arange(0, 6 * 65536, 3)]), False),
            O.from_values(3 * 65536 + np.arange(50, 200), True)]
    stored = int(values[5])
    for cb in ctxs:
        for op in OPS1:
            for t in (0, 1, stored, stored + 1, top, top + 1, M64):
                assert RBO.model_bytes(values, idx.mask, op, t, 0, cb) == RBO.query_typed(idx, op, t, 0, cb), (op, t)
                assert RBO.model_count(values, idx.mask, op, t, 0, cb) == RBO.query_count(idx, op, t, 0, cb), (op, t)
        for a, b in ((0, stored), (stored, stored + 3), (5, 2), (1, top), (stored, M64), (top + 1, M64)):
            if cb is None:
                assert RBO.model_bytes(values, idx.mask, "between", a, b) == RBO.query_typed(idx, "between", a, b), (a, b)
            assert RBO.model_count(values, idx.mask, "between", a, b, cb) == RBO.query_count(idx, "between", a, b, cb), (a, b)
