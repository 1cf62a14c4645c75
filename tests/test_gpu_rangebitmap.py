"""Range-encoded index queries on the MI355X (rbg_ctx_rangebitmap_*, rbg_rangebitmap_*; RB/RangeBitmap.java).
Acceptance: a fetched result is byte for byte the oracle's, a count equals the oracle's.  The oracle is
_rangebitmap.py's fast model over the values, which test_rangebitmap_oracle.py holds to the typed,
flag-faithful replay of the reference; the streams are the oracle Appender's or hand-written."""
import gzip
import os
import struct

import numpy as np
import pytest

import _fmt
import _oracle as O
import _rangebitmap as RBO

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
OPS1 = ("lte", "lt", "gt", "gte", "eq", "neq")
ROWS = (0, 1, 65535, 65536, 65537, 3 * 65536 + 100)
SLICES = (1, 5, 6, 8, 9, 24, 25, 33, 64)  # smallest; slice types; masks of 1 -> 2, 3 -> 4 and 5 bytes; largest
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rangebitmap")


@pytest.fixture(scope="module")
def eng(gpu):
    import roaringbitmap_amd as rb
    e = rb.Engine(0)
    yield e
    e.close()


def stream_of(values, slices):
    import roaringbitmap_amd as rb
    app = rb.RangeBitmap.appender((1 << slices) - 1)  # byte-equal to the oracle's (test_rangebitmap_oracle.py)
    app.add_many(np.asarray(values, dtype=np.uint64))
    return app.serialize()


def layout(n, slices, seed):
    """n values under `slices` bits that make, where n and slices allow it: random (bitmap) low slices, array
    slices (few rows with a high bit clear), run slices (long stretches), a block with no container at all
    (block 1), a bitmap record of 3,000 scattered rows in slices 0-4 (block 2), a block whose mask lacks most
    slices and is cut (block 3).  A bitmap record of a full block is not something the Appender writes (one
    run makes a run container): test_hand_written_records has it."""
    rng = np.random.default_rng(seed)
    mask = (1 << slices) - 1
    v = np.full(n, mask, dtype=np.uint64)
    lo = min(n, 65536)
    r = rng.integers(0, 1 << 63, lo, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, lo, dtype=np.uint64)
    keep_high = rng.random(lo) < 0.97  # the bits above 8 clear in 3 % of the rows: arrays in the high slices
    r = np.where(keep_high, r | np.uint64(mask & ~0xFF), r)
    v[:lo] = r & np.uint64(mask)
    v[30000:min(n, 40000)] = ((1 << (slices - 1)) | 5) & mask  # one value over 10,000 rows: runs
    if n > 65536:
        v[65536:min(n, 2 * 65536)] = mask  # no container
    if n > 2 * 65536:
        v[2 * 65536:2 * 65536 + 30000] = 0x1F & mask  # slices 5 and up: one long run
        # slices 0-4: 3,000 isolated rows and nothing else, a bitmap record of 3,000 values
        v[2 * 65536 + 30000 + 2 * rng.choice(17000, 3000, replace=False)] = np.uint64(mask & ~0x1F)
    if n > 3 * 65536:
        v[3 * 65536:] = rng.integers(0, 4, n - 3 * 65536, dtype=np.uint64) & np.uint64(mask)  # mask lacks the high slices
    return v


def thresholds(values, slices):
    mask = (1 << slices) - 1
    stored = int(values[len(values) // 3]) if len(values) else 5 & mask
    t = [0, 1, stored, max(stored - 1, 0), min(stored + 1, M64), mask, M64]
    if slices < 64:
        t.append(mask + 1)
    return sorted(set(t)), stored


class Resident:
    """an index resident on the engine, with the oracle's view of it"""

    def __init__(self, eng, buf, values=None):
        self.eng, self.buf = eng, buf
        self.h = eng.rangebitmap_load(buf)
        info = eng.rangebitmap_info(self.h)
        self.mask = info["mask"]
        self.values = RBO.Index(buf).values() if values is None else np.asarray(values, dtype=np.uint64)
        assert info["rows"] == len(self.values)

    def check(self, op, a, b=0, ctx=None, ctx_buf=None, bitmap=True):
        if bitmap:
            out = self.eng.rangebitmap_query(self.h, op, a, b, ctx)
            got = self.eng.batch_fetch(out).serialize()
            self.eng.release(out)
            assert got == RBO.model_bytes(self.values, self.mask, op, a, b, ctx_buf), (op, a, b)
        got = self.eng.rangebitmap_count(self.h, op, a, b, ctx)
        assert got == RBO.model_count(self.values, self.mask, op, a, b, ctx_buf), (op, a, b, "count")

    def release(self):
        self.eng.rangebitmap_release(self.h)


@pytest.mark.parametrize("slices", SLICES)
def test_rows_by_slice_count(eng, slices):
    """every op and cardinality, no context: rows 0 .. 3 x 65536 + 100 under every mask width; thresholds 0, 1,
    a stored value and its neighbours, mask, mask + 1, 2^64 - 1; between with min == 0, min > max, both ends
    inside one block's values, and ends outside the mask"""
    kinds = set()
    for n in ROWS:
        values = layout(n, slices, 1000 * slices + n % 997)
        buf = stream_of(values, slices)
        if n == ROWS[-1]:
            kinds = {t for t, _, _ in RBO.Index(buf).records}
            assert any(t == RBO.BITMAP and s == 3000 for t, s, _ in RBO.Index(buf).records)  # at most 4,096 values
        r = Resident(eng, buf, values)
        ts, stored = thresholds(values, slices)
        for op in OPS1:
            for t in ts:
                r.check(op, t)
        top = (1 << slices) - 1
        for a, b in ((0, stored), (min(stored + 1, M64), stored), (max(stored, 1), stored), (1, top), (2 & top, 3 & top),
                     (stored, M64), (top, top), (M64, M64)):
            r.check("between", a, b)
        r.release()
    assert RBO.RUN in kinds and (slices < 9 or kinds == {RBO.BITMAP, RBO.RUN, RBO.ARRAY})


def contexts(rng):
    """name -> serialized context over an index of 3 x 65536 + 100 rows"""
    a = rng.choice(65536, 3000, replace=False)  # an array
    b = rng.choice(65536, 30000, replace=False)  # a bitmap
    run = np.arange(500, 42000)  # a run
    return {
        "empty": O.from_values([], False),
        "lacks_blocks": O.from_values(np.concatenate([a, 2 * 65536 + b]), True),  # keys 0 and 2: 1 and 3 skipped
        "ends_early": O.from_values(np.concatenate([run, 65536 + a]), True),  # last key 1 < last block 3
        "past_the_rows": O.from_values(np.concatenate([b, 65536 + run, 2 * 65536 + a, 3 * 65536 + np.arange(50, 300),
                                                       5 * 65536 + a, 9 * 65536 + run]), True),  # keys 5, 9; rows >= maxRid
        "not_optimised": O.from_values(np.concatenate([np.arange(65536), 65536 + np.arange(0, 9000)]), False),
        "last_block_only": O.from_values(3 * 65536 + np.arange(0, 65536, 2), True),
    }


@pytest.mark.parametrize("slices", [9, 33])
def test_contexts(eng, slices):
    """none is covered above; here: empty, lacking blocks (the skip path), ending below the last block, keys and
    rows past maxRid, array / bitmap / run containers.  gtCardinality / gteCardinality count the context's
    rows past maxRid inside the last block and betweenCardinality intersects with the context's first
    container, as the reference does (the model has both)."""
    rng = np.random.default_rng(77 + slices)
    n = ROWS[-1]
    values = layout(n, slices, 5 + slices)
    r = Resident(eng, stream_of(values, slices), values)
    ts, stored = thresholds(values, slices)
    top = (1 << slices) - 1
    seen = set()
    for name, cbuf in contexts(rng).items():
        seen.update(_fmt.kinds(cbuf))
        cid = eng.load_pair(cbuf)[0]
        for op in OPS1:
            for t in ts:
                r.check(op, t, 0, cid, cbuf)
        for a, b in ((0, stored), (stored, stored), (1, top), (stored, M64), (min(stored + 1, M64), stored), (2, 3)):
            r.check("between", a, b, cid, cbuf, bitmap=False)
        with pytest.raises(ValueError, match="does not exist"):
            eng.rangebitmap_query(r.h, "between", 1, 2, cid)
        eng.release(cid)
    assert seen == {_fmt.A, _fmt.B, _fmt.R}
    r.release()


def test_results_on_the_type_boundaries(eng):
    """4,096 values (an array), 4,097 (a bitmap), a full block and the cut last block as one run each"""
    alt = np.arange(8194) % 2
    for vals, want in ((alt[:8192], [(0, _fmt.A, 4096)]), (alt, [(0, _fmt.B, 4097)])):
        r = Resident(eng, stream_of(vals, 1), vals)
        out = eng.rangebitmap_query(r.h, "eq", 0)
        got = eng.batch_fetch(out).serialize()
        assert [(c[0], c[1], c[2]) for c in _fmt.decode(got)] == want
        assert got == RBO.model_bytes(r.values, 1, "eq", 0)
        eng.release(out)
        r.check("neq", 1)
        r.check("lte", 0)
        r.release()
    vals = np.zeros(65536 + 100, dtype=np.uint64)
    r = Resident(eng, stream_of(vals, 2), vals)
    for op, a, b in (("eq", 0, 0), ("lte", 2, 0), ("neq", 1, 0), ("between", 1, 3), ("gt", 0, 0), ("between", 0, 0)):
        out = eng.rangebitmap_query(r.h, op, a, b)
        got = eng.batch_fetch(out).serialize()
        eng.release(out)
        assert got == RBO.model_bytes(vals, 3, op, a, b)
        if op != "gt" and (a, b) != (1, 3):
            assert [(c[0], c[1], c[2], c[4]) for c in _fmt.decode(got)] == [(0, _fmt.R, 65536, 1), (1, _fmt.R, 100, 1)]
    # the tie 2 c == 2 + 4 r stays an array; one more value in the run makes a run container
    for rows, kind in (([0, 1, 2, 65586], _fmt.A), ([0, 1, 2, 3, 65586], _fmt.R)):
        cbuf = O.from_values(rows, False)
        ctx = eng.load_pair(cbuf)[0]
        out = eng.rangebitmap_query(r.h, "eq", 0, 0, ctx)
        got = eng.batch_fetch(out).serialize()
        assert got == RBO.model_bytes(vals, 3, "eq", 0, 0, cbuf) and _fmt.kinds(got) == [kind, _fmt.A]
        eng.release(out)
        eng.release(ctx)
    r.release()


def test_hand_written_records(eng):
    """records the Appender cannot write but the format allows and a mapped file may hold: a bitmap record of a
    full block (cardinality field 0), a bitmap record of 5 values, an array in slice 0, an empty run record"""
    full = b"\x00" + struct.pack("<H", 0) + b"\xff" * 8192
    few_rows = np.array([1, 64, 4097, 40000, 65535])
    few = b"\x00" + struct.pack("<H", 5) + np.packbits(np.isin(np.arange(65536), few_rows), bitorder="little").tobytes()
    arr_rows = np.arange(7, 30000, 11)
    arr = b"\x02" + struct.pack("<H", arr_rows.size) + arr_rows.astype("<u2").tobytes()
    empty_run = b"\x01" + struct.pack("<H", 0)
    n = 2 * 65536 + 40
    head = struct.pack("<HBBHI", 0xF00D, 2, 3, 3, n)
    masks = bytes([0b111, 0b011, 0b100])
    empty_array = b"\x02" + struct.pack("<H", 0)
    buf = head + masks + full + few + arr + empty_array + full + empty_run
    idx = RBO.Index(buf)
    assert idx.consumed == len(buf) and [(t, s) for t, s, _ in idx.records] == \
        [(0, 0), (0, 5), (2, arr_rows.size), (2, 0), (0, 0), (1, 0)]
    r = Resident(eng, buf)
    assert eng.rangebitmap_info(r.h)["payload_bytes"] == 3 * 8192 + 2 * arr_rows.size
    for op in OPS1:
        for t in range(0, 9):
            r.check(op, t)
    for a, b in ((1, 3), (2, 2), (4, 7), (1, 7), (3, 1), (0, 5), (6, 9)):
        r.check("between", a, b)
    r.release()


def test_between_over_the_regression_fixture(eng):
    """betweenRegressionTest (RangeBitmapTest.java:50-65): 66,085 values in two blocks under maxValue 2,175,288"""
    import roaringbitmap_amd as rb
    with gzip.open(os.path.join(GOLDEN, "regression_values_u32le.gz"), "rb") as f:
        values = np.frombuffer(f.read(), dtype="<u4").astype(np.uint64)
    app = rb.RangeBitmap.appender(2175288)
    app.add_many(values)
    r = Resident(eng, app.serialize(), values)
    assert r.mask == (1 << 22) - 1
    for i in range(4):
        lo = 263501 + i
        r.check("between", lo, lo + 1)
        r.check("eq", lo)
        e0, e1, bt = (eng.rangebitmap_query(r.h, "eq", lo), eng.rangebitmap_query(r.h, "eq", lo + 1),
                      eng.rangebitmap_query(r.h, "between", lo, lo + 1))
        eng.pairwise("or", e0, e1)
        assert np.array_equal(eng.fetch().toArray(), eng.to_values(bt))
        for b in (e0, e1, bt):
            eng.release(b)
    r.release()


def test_session_behaviour(eng):
    """a query result is a batch like any other (pairwise, to_values); two indexes are resident at once; an
    index is released and another loaded; a released handle is refused"""
    import roaringbitmap_amd as rb
    va, vb = layout(65537, 9, 1), layout(3 * 65536 + 100, 25, 2)
    ra, rb_ = Resident(eng, stream_of(va, 9), va), Resident(eng, stream_of(vb, 25), vb)
    assert ra.h != rb_.h
    qa = eng.rangebitmap_query(ra.h, "lte", 200)
    qb = eng.rangebitmap_query(rb_.h, "gt", 5)
    want_a = RBO.brute_rows(va, va.size, "lte", 200)
    want_b = RBO.brute_rows(vb, vb.size, "gt", 5)
    assert np.array_equal(eng.to_values(qa), want_a) and np.array_equal(eng.to_values(qb), want_b)
    eng.pairwise("and", qa, qb)
    assert eng.fetch().serialize() == O.pairwise("and", O.from_values(want_a, True), O.from_values(want_b, True))
    # a result is a context of the next query: gte(low, lte(high)) is between(low, high) (regressionTestIssue586)
    lte = eng.rangebitmap_query(rb_.h, "lte", 1000)
    both = eng.rangebitmap_query(rb_.h, "gte", 3, 0, lte)
    assert np.array_equal(eng.to_values(both), RBO.brute_rows(vb, vb.size, "between", 3, 1000))
    assert eng.rangebitmap_count(rb_.h, "gte", 3, 0, lte) == eng.rangebitmap_count(rb_.h, "between", 3, 1000)
    for b in (qa, qb, lte, both):
        eng.release(b)
    ra.check("eq", int(va[3]))
    ra.release()
    with pytest.raises(rb.IllegalArgumentException, match="no such index"):
        eng.rangebitmap_count(ra.h, "lte", 1)
    rb_.check("neq", int(vb[3]))  # the other index is untouched
    vc = layout(65536, 6, 3)
    rc = Resident(eng, stream_of(vc, 6), vc)  # takes the freed handle
    assert rc.h == ra.h
    rc.check("between", 3, 40)
    rb_.check("between", 3, 40)
    rc.release()
    rb_.release()


def test_one_shot_forms(eng):
    """RangeBitmap.map(...).lte / ... (rbg_rangebitmap_query, rbg_rangebitmap_count): one case each"""
    import roaringbitmap_amd as rb
    values = layout(65537, 9, 4)
    app = rb.RangeBitmap.appender(511)
    app.add_many(values)
    r = app.build()
    ctx = rb.RoaringBitmap(O.from_values(np.arange(0, 70000, 3), True))
    stored = int(values[11])
    assert r.lte(stored).serialize() == RBO.model_bytes(values, 511, "lte", stored)
    assert r.gt(stored, ctx).serialize() == RBO.model_bytes(values, 511, "gt", stored, 0, ctx.serialize())
    assert r.between(3, stored).serialize() == RBO.model_bytes(values, 511, "between", 3, stored)
    assert r.neq(stored).serialize() == RBO.model_bytes(values, 511, "neq", stored)
    assert r.lte(1 << 40).serialize() == O.bitmap_of_range(0, 65537)
    assert r.gte(0, ctx).serialize() == ctx.serialize()
    assert r.eqCardinality(stored) == RBO.model_count(values, 511, "eq", stored)
    assert r.betweenCardinality(3, stored, ctx) == RBO.model_count(values, 511, "between", 3, stored, ctx.serialize())
    assert r.ltCardinality(stored, ctx) == RBO.model_count(values, 511, "lt", stored, 0, ctx.serialize())
    assert r.gteCardinality(0) == 65537
