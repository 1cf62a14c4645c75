"""Batched rank / select / contains / nextValue / previousValue on the MI355X (rbg_point_query,
rbg_ctx_point_query[_device]; RB/RoaringBitmap.java:1693, 2574-2624, 2820-2883, 2972-2979) against numpy
over the bitmap's sorted values v = O.to_values(buf):
  rank = searchsorted(v, x, 'right'), select = v[j] or -1, contains = isin,
  next = v[searchsorted(v, x, 'left')] or -1, prev = v[searchsorted(v, x, 'right') - 1] or -1.

The portable format types a non-run container by its cardinality (above 4096: bitmap), so a bitmap
container cannot hold bits in one word alone: the "bits only in word 0 / word 1023" shapes are the
nearest a bitmap container gets, 4,097 values packed into its first / last 65 words (the first / last
nine directory blocks, every other entry equal)."""
import os

import numpy as np
import pytest

import _gen
import _oracle as O
from _fmt import A, B, R, encode, runs_of

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
OPS = ("rank", "select", "contains", "next", "prev")


def _expect(v, op, q):
    v = np.asarray(v, dtype=np.int64)
    q = np.asarray(q, dtype=np.int64)
    if op == "rank":
        return np.searchsorted(v, q, "right").astype(np.int64)
    if op == "contains":
        return np.isin(q, v).astype(np.int64)
    ve = np.concatenate([v, [-1]])  # index len(v) and index -1 both read the -1
    if op == "select":
        return ve[np.minimum(q, v.size)]
    if op == "next":
        return ve[np.searchsorted(v, q, "left")]
    return ve[np.searchsorted(v, q, "right") - 1]


def _check_all(buf, xs, js, tag=""):
    import roaringbitmap_amd as rb
    v = O.to_values(buf)
    x = rb.RoaringBitmap(buf)
    xs = np.asarray(xs, dtype=np.int64)
    js = np.asarray(js, dtype=np.int64)
    got = {"rank": x.rank_many(xs), "select": x.select_many(js), "contains": x.contains_many(xs),
           "next": x.next_values(xs), "prev": x.previous_values(xs)}
    for op in OPS:
        q = js if op == "select" else xs
        want = _expect(v, op, q)
        g = got[op]
        assert g.dtype == np.int64 and g.shape == want.shape, (tag, op)
        bad = np.nonzero(g != want)[0]
        assert bad.size == 0, (tag, op, [(int(q[i]), int(g[i]), int(want[i])) for i in bad[:5]])
    return v


def _value_queries(rng, ctrs):
    xs = [0, (2 << 16) - 1, 3 << 16, 0xFFFFFFFF, (40000 << 16) + 65535]
    for key, _, vals in ctrs:
        base = key << 16
        vals = np.asarray(vals, dtype=np.int64)
        xs += [base + low for low in (0, 1, 63, 64, 511, 512, 513, 65535)]
        xs += [base + int(vals[0]), base + int(vals[-1])]
        samp = vals[rng.choice(vals.size, size=min(200, vals.size), replace=False)]
        for d in (-1, 0, 1):
            xs += list(base + samp + d)
        for s, ln in runs_of(vals)[:300]:
            xs += [base + s - 1, base + s, base + s + ln, base + s + ln + 1]
    xs = np.asarray(xs, dtype=np.int64)
    xs = xs[(xs >= 0) & (xs <= 0xFFFFFFFF)]
    xs = np.concatenate([xs, xs[:50]])  # duplicates
    return rng.permutation(xs)


def _select_queries(rng, cards):
    tot = int(sum(cards))
    js = [0, tot - 1, tot, tot + 5, 0xFFFFFFFF]
    for b in np.cumsum(cards):
        js += [int(b) - 1, int(b), int(b) + 1]
    js += list(rng.integers(0, tot, size=200))
    js = np.asarray(js, dtype=np.int64)
    js = js[(js >= 0) & (js <= 0xFFFFFFFF)]
    return rng.permutation(np.concatenate([js, js[:20]]))


@pytest.mark.parametrize("mode", _gen.MODES)
def test_container_kinds(gpu, mode):
    """every generator mode at keys (2, 9, 40000) between an array container and a full run container"""
    rng = np.random.default_rng(4100 + _gen.MODES.index(mode))
    ctrs = [(k, *_gen.container(rng, mode)) for k in (2, 9, 40000)]
    ctrs += [(5, A, np.sort(rng.choice(65536, 300, replace=False))), (20000, R, np.arange(65536))]
    ctrs.sort(key=lambda c: c[0])
    buf = encode(ctrs)
    _check_all(buf, _value_queries(rng, ctrs), _select_queries(rng, [len(c[2]) for c in ctrs]), mode)


SHAPES = {
    "runs_32768": [(0, R, np.arange(0, 65536, 2))],
    "full_bitmap": [(0, B, np.arange(65536))],
    "full_run": [(0, R, np.arange(65536))],
    "bitmap_last_words": [(0, B, np.arange(65536 - 4097, 65536))],
    "bitmap_first_words": [(0, B, np.arange(4097))],
    "run_single_last": [(0, R, np.array([65535]))],
    "array_one": [(0, A, np.array([12345]))],
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_directory_shapes(gpu, name):
    rng = np.random.default_rng(17)
    ctrs = SHAPES[name]
    # the same container again at key 3, so that the prefix in front of it is not zero
    both = ctrs + [(3, ctrs[0][1], ctrs[0][2])]
    for cs in (ctrs, both):
        xs = _value_queries(rng, cs)
        xs = np.concatenate([xs, rng.integers(0, 4 << 16, size=300)])
        _check_all(encode(cs), xs, _select_queries(rng, [len(c[2]) for c in cs]), name)


def test_empty_bitmap(gpu):
    import roaringbitmap_amd as rb
    for x in (rb.RoaringBitmap(), rb.ImmutableRoaringBitmap(), rb.MutableRoaringBitmap()):
        qs = [0, 1, 65536, 0xFFFFFFFF]
        assert (x.rank_many(qs) == 0).all() and (x.contains_many(qs) == 0).all()
        assert (x.next_values(qs) == -1).all() and (x.previous_values(qs) == -1).all()
        assert (x.select_many(qs) == -1).all()
        assert x.rankLong(5) == 0 and x.nextValue(0) == -1 and x.previousValue(0xFFFFFFFF) == -1
        assert x.rangeCardinality(0, 1 << 32) == 0
        with pytest.raises(rb.IllegalArgumentException):
            x.select(0)
        with pytest.raises(rb.NoSuchElementException):
            x.first()
        with pytest.raises(rb.NoSuchElementException):
            x.last()
        assert x.rank_many([]).shape == (0,) and x.select_many(np.zeros(0, dtype=np.uint32)).dtype == np.int64


def test_full_universe(gpu):
    """2^32 values: rankLong does not fit a Java int, and select's j is unsigned"""
    import roaringbitmap_amd as rb
    univ = rb.RoaringBitmap.add(rb.RoaringBitmap(), 0, 1 << 32)
    assert univ.rankLong(0xFFFFFFFF) == 1 << 32 and univ.rank(0xFFFFFFFF) == 0
    assert univ.rankLong(0) == 1 and univ.rank(0x7FFFFFFF) == -(1 << 31)
    assert list(univ.select_many([0, 65536, 0xFFFFFFFF])) == [0, 65536, 0xFFFFFFFF]
    assert univ.select(0xFFFFFFFF) == -1 and univ.select(-1) == -1  # the Java int of 0xFFFFFFFF, either way
    assert univ.rangeCardinality(0, 1 << 32) == 1 << 32
    assert univ.first() == 0 and univ.last() == -1
    assert univ.nextValue(0xFFFFFFFF) == 0xFFFFFFFF and univ.previousValue(0) == 0
    holed = rb.RoaringBitmap.remove(univ, 123456, 123457)
    assert holed.rankLong(0xFFFFFFFF) == (1 << 32) - 1 and holed.rank(0xFFFFFFFF) == -1
    assert holed.rankLong(123455) == 123456 and holed.rankLong(123456) == 123456 and holed.rankLong(123457) == 123457
    assert list(holed.select_many([123455, 123456, 0xFFFFFFFE, 0xFFFFFFFF])) == [123455, 123457, 0xFFFFFFFF, -1]
    assert list(holed.contains_many([123455, 123456, 123457])) == [1, 0, 1]
    assert holed.nextValue(123456) == 123457 and holed.previousValue(123456) == 123455
    assert holed.rangeCardinality(0, 1 << 32) == (1 << 32) - 1 and holed.rangeCardinality(123456, 123457) == 0
    with pytest.raises(rb.IllegalArgumentException):
        holed.select(0xFFFFFFFF)


@pytest.fixture(scope="module")
def mixed():
    rng = np.random.default_rng(4242)
    buf = _gen.bitmap(rng, np.arange(8))
    return buf, O.to_values(buf)


@pytest.mark.parametrize("n", [0, 1, 63, 65, 257, 1000])
def test_query_counts(gpu, mixed, n):
    import roaringbitmap_amd as rb
    buf, v = mixed
    rng = np.random.default_rng(n)
    xs = rng.integers(0, 9 << 16, size=n)
    js = rng.integers(0, v.size + 10, size=n)
    x = rb.RoaringBitmap(buf)
    for op, f in (("rank", x.rank_many), ("select", x.select_many), ("contains", x.contains_many),
                  ("next", x.next_values), ("prev", x.previous_values)):
        q = js if op == "select" else xs
        got = f(q)
        assert got.dtype == np.int64 and got.shape == (n,)
        assert (got == _expect(v, op, q)).all(), (op, n)


def test_session_path(gpu):
    """separate resident batches queried in turn (the second round from the cached directory), release and
    reload, the rejection of a packed batch, and the device-pointer path against the host path"""
    import torch
    import roaringbitmap_amd as rb
    rng = np.random.default_rng(99)
    bufs = [_gen.bitmap(rng, np.arange(6), p_present=0.9), _gen.bitmap(rng, np.arange(3, 12), p_present=0.9)]
    vs = [O.to_values(b) for b in bufs]
    eng = rb.Engine(0)
    ids = eng.load_pair(*bufs)
    ids.append(eng.load([bufs[0]]))
    vs.append(vs[0])
    xs = rng.integers(0, 13 << 16, size=1000)
    for rnd in range(2):
        for b, v in zip(ids, vs):
            js = rng.integers(0, v.size + 5, size=300)
            for op in OPS:
                q = js if op == "select" else xs
                got = eng.point_query(op, b, q)
                assert got.dtype == np.int64 and (got == _expect(v, op, q)).all(), (rnd, b, op)
    eng.release(ids[0])
    again = eng.load_pair(bufs[1])[0]
    assert (eng.point_query("rank", again, xs) == _expect(vs[1], "rank", xs)).all()
    assert (eng.point_query("rank", ids[1], xs) == _expect(vs[1], "rank", xs)).all()
    with pytest.raises(rb.IllegalArgumentException):
        eng.point_query(16, ids[1], xs)  # no op beyond the five
    # a packed batch (arrays alone, 2 B granularity) is not an operand: the engine's own error, raised by
    # operand() on the host before any launch (engine.cpp: "pairwise operands must be single-bitmap ...")
    arr = O.from_values(np.arange(0, 3 << 16, 97, dtype=np.uint32))
    packed = eng.load([arr], packed=True)
    with pytest.raises(rb.IllegalArgumentException, match="slot-aligned"):
        eng.point_query("rank", packed, xs)
    two = eng.load(bufs)  # two bitmaps in one batch: not an operand either
    with pytest.raises(rb.IllegalArgumentException):
        eng.point_query("rank", two, xs)
    with pytest.raises(rb.IllegalArgumentException):
        eng.point_query(99, ids[1], xs)
    # device pointers: torch tensors in and out, enqueued on the engine stream
    dev = torch.device("cuda", 0)
    for op in OPS:
        q = rng.integers(0, vs[1].size + 5, size=1000) if op == "select" else xs
        qt = torch.from_numpy(np.asarray(q, dtype=np.int64)).to(dev)
        out = eng.point_query(op, ids[1], qt)
        eng.sync()
        assert isinstance(out, torch.Tensor) and out.dtype == torch.int64 and out.device.type == "cuda"
        host = eng.point_query(op, ids[1], q)
        assert (out.cpu().numpy() == host).all() and (host == _expect(vs[1], op, q)).all(), op
    assert eng.point_query("rank", ids[1], torch.zeros(0, dtype=torch.int64, device=dev)).numel() == 0
    eng.close()


def test_realdata(gpu):
    z = np.load(os.path.join(GOLD, "realdata", "census1881.npz"))
    vals = z["values"][z["offsets"][0]:z["offsets"][1]]
    rng = np.random.default_rng(1881)
    for run_opt in (False, True):
        buf = O.from_values(vals, run_opt)
        v = O.to_values(buf)
        hi = int(v[-1]) + 70000
        xs = np.concatenate([rng.integers(0, hi, size=8000), v[rng.integers(0, v.size, size=2000)]])
        js = rng.integers(0, v.size + 3, size=10000)
        _check_all(buf, xs, js, f"census1881 run_opt={run_opt}")


def test_closed_form(gpu):
    """multiples of 7: the answers follow from arithmetic alone"""
    import roaringbitmap_amd as rb
    n = 100000
    x = rb.RoaringBitmap.bitmapOf(np.arange(n, dtype=np.int64) * 7)
    k = np.concatenate([[0, 1, n - 2], np.random.default_rng(7).integers(0, n - 1, size=5000)])
    assert (x.rank_many(7 * k) == k + 1).all()
    assert (x.rank_many(7 * k + 3) == k + 1).all()
    assert (x.select_many(k) == 7 * k).all()
    assert (x.next_values(7 * k + 1) == 7 * k + 7).all()
    assert (x.previous_values(7 * k + 6) == 7 * k).all()
    assert (x.contains_many(7 * k) == 1).all() and (x.contains_many(7 * k + 1) == 0).all()
    assert x.rankLong(7 * 1234) == 1235 and x.select(1234) == 7 * 1234
    assert x.nextValue(7 * 1234 + 1) == 7 * 1235 and x.previousValue(7 * 1234 + 6) == 7 * 1234
    assert x.nextValue(7 * (n - 1) + 1) == -1 and x.previousValue(0) == 0
    assert x.first() == 0 and x.last() == 7 * (n - 1)


def test_scalar_api(gpu):
    import roaringbitmap_amd as rb
    rng = np.random.default_rng(31)
    ctrs = [(0, *_gen.container(rng, "a_mid")), (1, *_gen.container(rng, "b_mid")), (2, *_gen.container(rng, "r_mid")),
            (40000, A, np.array([7, 65535]))]
    buf = encode(ctrs)
    v = O.to_values(buf).astype(np.int64)
    for cls in (rb.RoaringBitmap, rb.ImmutableRoaringBitmap, rb.MutableRoaringBitmap):
        x = cls(buf)
        for st, en in ((5, 60000), (70000, (2 << 16) + 123), (100, 100), (9, 3), (0, 1 << 32)):
            want = int(np.searchsorted(v, en, "left") - np.searchsorted(v, st, "left")) if st < en else 0
            assert x.rangeCardinality(st, en) == want, (st, en)
        for st, en in ((-1, 10), (0, (1 << 32) + 1)):
            with pytest.raises(ValueError):
                x.rangeCardinality(st, en)
        assert x.first() == int(v[0]) and x.last() == rb.roaring._int32(int(v[-1]))
        assert x.last() < 0  # key 40000: the Java int is negative
        assert x.select(0) == int(v[0]) and x.select(v.size - 1) == x.last()
        assert x.rank(int(v[10])) == 11 and x.rankLong(0xFFFFFFFF) == v.size
        assert x.nextValue(int(v[10]) + 1) == int(v[11]) and x.previousValue(int(v[10]) - 1) == int(v[9])
        assert x.nextValue((40000 << 16) + 65535) == (40000 << 16) + 65535 and x.nextValue(40001 << 16) == -1
        assert x.contains(int(v[5])) and x.contains_many([int(v[5])])[0] == 1  # contains(int) itself is unchanged
        with pytest.raises(rb.IllegalArgumentException):
            x.select(v.size)
