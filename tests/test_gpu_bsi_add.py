"""Two resident bit-sliced indexes added on the MI355X (rbg_ctx_bsi_add, rbg_bsi_add; RoaringBitmapSliceIndex.add,
BSI/:66-95, min / max :97-138).  The acceptance throughout: the result batch, fetched, is byte for byte the
reference's sequence composed on the CPU oracle (tests/_bsi_add.py add_reference), {nbits, min, max} are its,
and the batch behaves as the loaded batch of those bitmaps does in every op that takes an index."""
import numpy as np
import pytest

import _bsi
import _oracle as O
from _bsi import BSI
from _bsi_add import add_reference, sum_values

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng(gpu):
    import roaringbitmap_amd as rb
    e = rb.Engine(0)
    yield e
    e.close()


def _fetch(eng, b):
    return [x.serialize() for x in eng.batch_fetch_range(b)]


def _kinds(buf):
    s = O.stats(buf)
    return s["array"], s["bitmap"], s["run"]


def _add(eng, a, b):
    """the device sum of two oracle indexes -> (bitmaps, nbits, min, max); every batch released"""
    ia, ib = eng.load([a.ebm] + a.ba), eng.load([b.ebm] + b.ba)
    r, nbits, mn, mx = eng.bsi_add(ia, a.bit_count(), ib, b.bit_count(), a.min, a.max)
    got = _fetch(eng, r)
    for x in (ia, ib, r):
        eng.release(x)
    return got, nbits, mn, mx


def _check(eng, a, b, tag="", want=None):
    want = want or add_reference(a, b)
    got, nbits, mn, mx = _add(eng, a, b)
    assert (nbits, mn, mx) == (want.bit_count(), want.min, want.max), tag
    assert len(got) == 1 + nbits and got == [want.ebm] + want.ba, (tag, [len(x) for x in got])
    return want


def _pairs(cols, vals):
    return BSI.from_columns(np.asarray(cols, dtype=np.int64), np.asarray(vals, dtype=np.int64))


def test_known_answers(eng):
    """RBBsiTest.testAdd and testAddAndEvaluate"""
    x = np.arange(1, 120)
    a = _pairs(np.arange(1, 100), np.arange(1, 100))
    r = _check(eng, a, _pairs(x, x), "testAdd")
    assert (r.min, r.max) == (2, 198)
    r = _check(eng, a, _pairs(120 - x, x), "testAddAndEvaluate")
    assert O.to_values(r.compare("EQ", 120)).tolist() == list(range(1, 100))
    assert O.to_values(r.compare("RANGE", 1, 20)).tolist() == list(range(100, 120))


def test_carry_through_every_slice(eng):
    """0x7FFF + 1 on the even columns and 0x7FFF + 0 on the odd ones of the same words: the carry of the
    even columns runs through all 15 slices and opens a 16th"""
    cols = (3 << 16) + np.arange(640)
    a, b = _pairs(cols, np.full(640, 0x7FFF)), _pairs(cols, 1 - (cols & 1))
    r = _check(eng, a, b)
    assert (a.bit_count(), b.bit_count(), r.bit_count(), r.min, r.max) == (15, 1, 16, 0x7FFF, 0x8000)


@pytest.mark.parametrize("va,vb,nbits", [(1, 2, 2), (1, 0x300, 10), (0x300, 1, 10), (0, 0, 1), (0, 5, 3), (3, 1, 3)])
def test_slice_counts(eng, va, vb, nbits):
    """na < nb, na > nb, no growth (1 + 2), zero values, growth by one (3 + 1)"""
    cols = np.array([5, 6, 70000, 0xFFFFFFFF])
    r = _check(eng, _pairs(cols, np.full(4, va)), _pairs(cols[1:], np.full(3, vb)), (va, vb))
    assert r.bit_count() == nbits


@pytest.mark.parametrize("nx,ny,both,kind", [(2048, 2048, 0, (1, 0, 0)), (2048, 2049, 0, (0, 1, 0)),
                                             (5000, 5000, 2952, (1, 0, 0)), (5000, 5001, 2952, (0, 1, 0))])
def test_cardinality_threshold_in_a_result_slice(eng, nx, ny, both, kind):
    """slice 0 of the sum is the xor of two arrays / of two bitmaps with exactly 4096 and 4097 values"""
    p = np.random.default_rng(nx + ny).permutation(65536)
    x, y = p[:nx], p[nx - both:nx - both + ny]
    a, b = _pairs((9 << 16) + x, np.ones(nx)), _pairs((9 << 16) + y, np.ones(ny))
    r = _check(eng, a, b)
    assert _kinds(r.ba[0]) == kind and O.stats(r.ba[0])["card"] == nx + ny - 2 * both
    assert O.stats(r.ba[1])["card"] == both if both else r.bit_count() == 1


def test_slice_container_cancels_under_one_key(eng):
    """1 + 1 on every column of key 4, 1 + nothing under key 6: slice 0 keeps a container for key 6 alone,
    and key 4 is still there in slice 1"""
    c4, c6 = (4 << 16) + np.arange(0, 3000, 3), (6 << 16) + np.arange(50)
    a, b = _pairs(np.concatenate([c4, c6]), np.ones(1050)), _pairs(c4, np.ones(1000))
    r = _check(eng, a, b)
    assert O.to_values(r.ba[0]).tolist() == c6.tolist() and O.to_values(r.ba[1]).tolist() == c4.tolist()


def test_full_slices_and_full_existence_bitmaps(eng):
    """key 1: 65,536 columns of value 1 on both sides (slice 0 vanishes, slice 1 is a full bitmap, ebM' a
    run); key 2: bitmap with array, full (stays a bitmap); key 3: array with bitmap, full (a run); key 5: a
    full container of a alone (a clone: stays a bitmap)"""
    full = np.arange(65536)
    ca = np.concatenate([(1 << 16) + full, (2 << 16) + full[4000:], (3 << 16) + full[:4000], (5 << 16) + full])
    cb = np.concatenate([(1 << 16) + full, (2 << 16) + full[:4000], (3 << 16) + full[4000:]])
    r = _check(eng, _pairs(ca, np.ones(ca.size)), _pairs(cb, np.ones(cb.size)))
    assert _kinds(r.ebm) == (0, 2, 2) and O.stats(r.ebm)["card"] == 4 * 65536
    assert _kinds(r.ba[0]) == (0, 3, 0) and _kinds(r.ba[1]) == (0, 1, 0) and O.stats(r.ba[1])["card"] == 65536


def test_keys_of_one_side_and_columns_of_one_side(eng):
    """keys only in a (0), only in b (65535) and in both (9); within key 9 the two sides interleave inside
    shared 64-bit words, some columns on both sides"""
    rng = np.random.default_rng(5)
    ca = np.concatenate([np.arange(0, 200, 2), (9 << 16) + np.arange(0, 4000, 2), [(9 << 16) + 65535]])
    cb = np.concatenate([(9 << 16) + np.arange(1, 4000, 3), (65535 << 16) + np.array([0, 63, 64, 65535])])
    va, vb = rng.integers(0, 1 << 12, ca.size), rng.integers(0, 1 << 9, cb.size)
    r = _check(eng, _pairs(ca, va), _pairs(cb, vb))
    cols, vals = sum_values(ca, va, cb, vb)
    assert O.to_values(r.ebm).tolist() == cols.tolist() and (r.min, r.max) == (int(vals.min()), int(vals.max()))


def _nine_keys(seed):
    """two indexes of up to 200,000 columns over nine keys: arrays, bitmaps, the 4096 / 4097 boundary, a full
    container, keys of one side alone"""
    rng = np.random.default_rng(seed)
    keys = np.array([0, 1, 7, 40, 41, 300, 4000, 65534, 65535], dtype=np.int64)
    out = []
    for bits, sizes in ((20, [30000, 100, 60000, 0, 5, 4096, 4097, 20000, 35000]),
                        (17, [4097, 0, 65536, 50000, 700, 4096, 30, 0, 45000])):
        sizes = list(rng.permutation(sizes)) if seed else sizes
        cols = np.concatenate([(k << 16) + rng.choice(65536, s, replace=False) for k, s in zip(keys, sizes)])
        out.append((cols.astype(np.int64), rng.integers(0, 1 << bits, size=cols.size)))
    return out


_nine = {}


def _nine_case(seed):
    if seed not in _nine:
        (ca, va), (cb, vb) = _nine_keys(seed)
        a, b = _pairs(ca, va), _pairs(cb, vb)
        _nine[seed] = (a, b, add_reference(a, b), sum_values(ca, va, cb, vb))
    return _nine[seed]


@pytest.mark.parametrize("seed", [0, 1, 2, 3, 4])
def test_array_bitmap_mix_over_nine_keys(eng, seed):
    a, b, want, (cols, vals) = _nine_case(seed)
    _check(eng, a, b, seed, want=want)
    assert (want.min, want.max) == (int(vals.min()), int(vals.max()))


def test_many_keys_in_one_pass(eng):
    """600 present keys of two or three columns each: the min / max descent takes its wave-per-key form (512
    keys and more in a pass), and the extremes sit in single columns of keys in the middle"""
    rng = np.random.default_rng(600)
    k = np.arange(600, dtype=np.int64) * 100
    ca = np.concatenate([(k << 16) + (k % 7), (k << 16) + 65535 - (k % 5)])
    cb = np.concatenate([(k[::3] << 16) + (k[::3] % 7), (k[1::3] << 16) + 40000])
    va, vb = rng.integers(50, 1 << 10, ca.size), rng.integers(50, 1 << 12, cb.size)
    va[301], vb[77] = 3, 1 << 13  # a column of key 30100 that a alone holds; a column of key 23100 on both sides
    r = _check(eng, _pairs(ca, va), _pairs(cb, vb))
    cols, vals = sum_values(ca, va, cb, vb)
    assert (r.min, r.max) == (int(vals.min()), int(vals.max())) == (3, int(va[231]) + (1 << 13))


@pytest.mark.parametrize("budget", ["one_key", "1", "two_keys"])
def test_forced_passes(eng, monkeypatch, budget):
    """the workspace budget forced down through the environment switch: whole keys per pass, the same bytes
    and the same min / max (taken in the first sweep alone)"""
    a, b, want, _ = _nine_case(0)
    m = 2 + max(a.bit_count(), b.bit_count())
    nbytes = {"one_key": 8192 * m, "1": 1, "two_keys": 2 * 8192 * m + 100}[budget]
    assert -(-9 // max(1, nbytes // (8192 * m))) >= 3  # nine keys: at least three passes
    monkeypatch.setenv("RBG_BSI_BUILD_WS", str(nbytes))
    _check(eng, a, b, budget, want=want)
    monkeypatch.delenv("RBG_BSI_BUILD_WS")
    _check(eng, a, b, "default again", want=want)


def test_added_to_itself(eng):
    (ca, va), _ = _nine_keys(0)
    a = _pairs(ca, va)
    want = add_reference(a, a)
    ia = eng.load([a.ebm] + a.ba)
    r, nbits, mn, mx = eng.bsi_add(ia, a.bit_count(), ia, a.bit_count())
    assert _fetch(eng, r) == [want.ebm] + want.ba and (nbits, mn, mx) == (want.bit_count(), want.min, want.max)
    assert _fetch(eng, ia) == [a.ebm] + a.ba  # the operand is untouched
    pc, pv = eng.bsi_to_pairs(r, nbits)
    order = np.argsort(ca)
    assert (pc == ca[order]).all() and (pv == 2 * va[order]).all()
    eng.release(r)
    eng.release(ia)


def test_empty_operands_and_the_32nd_slice(eng):
    a = _pairs([5, 70000, 6], [9, 2, 4])
    e = _pairs([], [])
    got, nbits, mn, mx = _add(eng, a, e)  # b empty: a itself, with the extrema handed in
    assert got == [a.ebm] + a.ba and (nbits, mn, mx) == (4, 2, 9)
    ia, ie = eng.load([a.ebm] + a.ba), eng.load([e.ebm])
    r, nbits, mn, mx = eng.bsi_add(ia, 4, ie, 0, 123, 456)  # not recomputed (BSI/:67-69)
    assert _fetch(eng, r) == [a.ebm] + a.ba and (nbits, mn, mx) == (4, 123, 456)
    for x in (ia, ie, r):
        eng.release(x)
    _check(eng, e, a, "a empty")  # b's slices as clones, min / max recomputed
    got, nbits, mn, mx = _add(eng, e, e)
    assert got == [_bsi.EMPTY] and (nbits, mn, mx) == (0, 0, 0)
    wide = _pairs([5, 70000], [2**31 - 1, 3])
    r = _check(eng, wide, _pairs([5], [1]), "wrap")
    assert (r.bit_count(), r.min, r.max) == (32, 3, -2**31)


def test_refusals_leave_no_batch(eng):
    import roaringbitmap_amd as rb
    wide, one = _pairs([5, 70000], [2**31 - 1, 3]), _pairs([5], [1])
    iw, io = eng.load([wide.ebm] + wide.ba), eng.load([one.ebm] + one.ba)
    top, nbits, mn, mx = eng.bsi_add(iw, 31, io, 1)  # 2^31 at column 5: 32 slices
    assert nbits == 32
    ro = BSI.from_columns(np.arange(1000), np.arange(1000) // 100, True)
    assert _kinds(ro.ebm)[2] == 1
    ir = eng.load([ro.ebm] + ro.ba)
    probe, *_ = eng.bsi_add(io, 1, io, 1)
    eng.release(probe)
    with pytest.raises(rb.IllegalArgumentException, match="more than 32 slices"):
        eng.bsi_add(top, 32, top, 32)  # 2^31 + 2^31
    for x, nx, y, ny in ((ir, ro.bit_count(), io, 1), (io, 1, ir, ro.bit_count())):
        with pytest.raises(rb.IllegalArgumentException, match="composed route"):
            eng.bsi_add(x, nx, y, ny)
    with pytest.raises(rb.IllegalArgumentException):
        eng.bsi_add(io, 2, io, 1)  # n_bm != 1 + nbits
    with pytest.raises(rb.IllegalArgumentException):
        eng.bsi_add(io, 1, io, 33)
    again, nbits, mn, mx = eng.bsi_add(io, 1, io, 1)
    assert again == probe  # every refusal freed its slot: the next sum takes the released id
    assert _fetch(eng, again) == [one.ebm, _bsi.EMPTY, one.ba[0]] and (nbits, mn, mx) == (2, 2, 2)
    for x in (iw, io, top, ir, again):
        eng.release(x)


def test_result_as_an_index_operand(eng):
    """the sum against the loaded batch of the reference's bitmaps in everything that takes a built index"""
    a, b, want, (cols, vals) = _nine_case(0)
    ia, ib = eng.load([a.ebm] + a.ba), eng.load([b.ebm] + b.ba)
    built, nbits, mn, mx = eng.bsi_add(ia, a.bit_count(), ib, b.bit_count())
    loaded = eng.load([want.ebm] + want.ba)
    sb, sl = eng.batch_stats(built), eng.batch_stats(loaded)
    assert len(sb) == 8 and sb == sl, (sb, sl)
    assert (eng.batch_counts(built) == eng.batch_counts(loaded)).all()
    rng = np.random.default_rng(91)
    for op in ("EQ", "RANGE"):
        for lo, hi in ((int(vals[5]), int(vals[5]) + 1000), tuple(sorted(int(x) for x in rng.integers(0, mx + 2, 2)))):
            res = []
            for x in (built, loaded):
                eng.bsi(x, op, nbits, lo, hi, mn, mx, want_sum=True)
                res.append((eng.fetch().serialize(), eng.bsi_sums()))
            assert res[0] == res[1] and res[0][0] == want.compare(op, lo, hi), (op, lo, hi)
            assert res[0][1] == want.sum(res[0][0])
    eng.bsi_buffer(built, 0, nbits, int(vals[7]), 0, mn, mx)
    got = eng.fetch().serialize()
    eng.bsi_buffer(loaded, 0, nbits, int(vals[7]), 0, mn, mx)
    assert got == eng.fetch().serialize()
    q = np.concatenate([cols[::97], [1 << 20, 0xFFFFFFF0]]).astype(np.int64)
    exp = np.where(np.isin(q, cols), vals[np.minimum(np.searchsorted(cols, q), cols.size - 1)], -1)
    assert (eng.bsi_get_values(built, nbits, q) == exp).all()
    pc, pv = eng.bsi_to_pairs(built, nbits)
    assert (pc == cols).all() and (pv == vals).all()
    rb_, ab = eng.run_optimize(built)
    rl, al = eng.run_optimize(loaded)
    assert ab == al and _fetch(eng, rb_) == _fetch(eng, rl)
    st, en = (1 << 16) + 5, (41 << 16) + 2
    sb_, sl_ = eng.select_range(built, st, en), eng.select_range(loaded, st, en)
    assert _fetch(eng, sb_) == _fetch(eng, sl_)
    for x in (ia, ib, built, loaded, rb_, rl, sb_, sl_):
        eng.release(x)


def _rb_index(cls, o):
    import roaringbitmap_amd as rb
    x = cls(rb.RoaringBitmap(o.ebm), [rb.RoaringBitmap(s) for s in o.ba], o.min, o.max)
    x.runOptimized = o.run_optimized
    return x


def _rb_bytes(x):
    return [x.ebM.serialize()] + [s.serialize() for s in x.bA], x.bitCount(), x.minValue, x.maxValue


@pytest.mark.parametrize("cls_name", ["RoaringBitmapSliceIndex", "MutableBitSliceIndex"])
@pytest.mark.parametrize("composed", [False, True])
def test_python_classes(gpu, monkeypatch, cls_name, composed):
    import roaringbitmap_amd as rb
    cls = getattr(rb, cls_name)
    (ca, va), (cb, vb) = _nine_keys(0)
    keep_a, keep_b = (ca >> 16) < 41, (cb >> 16) >= 7  # keys of one side alone and of both
    a, b = _pairs(ca[keep_a], va[keep_a]), _pairs(cb[keep_b], vb[keep_b])
    want = add_reference(a, b)
    if composed:
        monkeypatch.setenv("RBG_BSI_ADD_COMPOSED", "1")
    x, y = _rb_index(cls, a), _rb_index(cls, b)
    x.add(y)
    assert _rb_bytes(x) == ([want.ebm] + want.ba, want.bit_count(), want.min, want.max)
    assert _rb_bytes(y)[0] == [b.ebm] + b.ba and x.runOptimized is False


def test_run_optimized_index_takes_the_composed_route(gpu):
    import roaringbitmap_amd as rb
    rng = np.random.default_rng(12)
    ca = np.concatenate([np.arange(20000), (3 << 16) + rng.choice(65536, 5000, replace=False)])
    cb = np.concatenate([np.arange(10000, 30000), (3 << 16) + rng.choice(65536, 300, replace=False)])
    a = BSI.from_columns(ca, ca // 700, True)
    b = BSI.from_columns(cb, rng.integers(0, 40, cb.size))
    assert _kinds(a.ebm)[2] >= 1 and sum(_kinds(s)[2] for s in a.ba) >= 1
    want = add_reference(a, b)
    x = _rb_index(rb.RoaringBitmapSliceIndex, a)
    x.add(_rb_index(rb.RoaringBitmapSliceIndex, b))
    assert _rb_bytes(x) == ([want.ebm] + want.ba, want.bit_count(), want.min, want.max) and x.runOptimized is True
    z = _rb_index(rb.MutableBitSliceIndex, a)
    with pytest.raises(rb.IllegalArgumentException, match="run container"):
        z.add(_rb_index(rb.MutableBitSliceIndex, b))
    assert _rb_bytes(z)[0] == [a.ebm] + a.ba
