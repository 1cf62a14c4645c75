"""(column, value) pairs written into a resident bit-sliced index on the MI355X (rbg_ctx_bsi_set_values[_device],
rbg_bsi_set_values; RoaringBitmapSliceIndex.setValues, BSI/:349-357, setValue :299-313).  The acceptance
throughout: the result batch, fetched, is byte for byte the oracle's replay of the pairs in order
(tests/_bsi_set.py set_reference), {nbits, min, max} are its, the operand's bytes are what they were, and the
batch behaves as the loaded batch of those bitmaps does in the ops that take an index."""
import ctypes

import numpy as np
import pytest

import _bsi
import _oracle as O
from _bsi import BSI
from _bsi_set import replay_values, set_reference

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


def _index(cols, vals):
    return BSI.from_columns(np.asarray(cols, dtype=np.int64), np.asarray(vals, dtype=np.int64))


def _all(o):
    return [o.ebm] + o.ba


def _set(eng, a, cols, vals, nbits=None):
    """the device setValues on an oracle index -> (bitmaps, nbits, min, max); the operand checked unchanged,
    every batch released"""
    ia = eng.load(_all(a))
    r, nb, mn, mx = eng.bsi_set_values(ia, a.bit_count() if nbits is None else nbits, cols, vals, a.min, a.max)
    got = _fetch(eng, r)
    assert _fetch(eng, ia) == _all(a), "the operand changed"
    eng.release(ia)
    eng.release(r)
    return got, nb, mn, mx


def _check(eng, a, cols, vals, tag="", want=None):
    want = want or set_reference(a, cols, vals)
    got, nb, mn, mx = _set(eng, a, cols, vals)
    assert (nb, mn, mx) == (want.bit_count(), want.min, want.max), tag
    assert len(got) == 1 + nb and got == _all(want), (tag, [len(x) for x in got], [len(x) for x in _all(want)])
    return want


def _values(x, cols):
    v = np.zeros(len(cols), dtype=np.int64)
    for i, s in enumerate(x.ba):
        v |= np.isin(cols, O.to_values(s)).astype(np.int64) << i
    return v


def test_starting_points(eng):
    """into the empty batch bsi_from_columns makes for n = 0, and with one pair"""
    e, nb, mn, mx = eng.bsi_from_columns(np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64))
    assert (nb, mn, mx) == (0, 0, 0)
    cols, vals = np.array([70000, 5, 70000, 0xFFFFFFFF]), np.array([9, 300, 2, 0])
    want = set_reference(_index([], []), cols, vals)
    r, nb, mn, mx = eng.bsi_set_values(e, 0, cols, vals)
    assert _fetch(eng, r) == _all(want) and (nb, mn, mx) == (9, 0, 300) == (want.bit_count(), want.min, want.max)
    assert _fetch(eng, e) == [_bsi.EMPTY]
    eng.release(e)
    eng.release(r)
    a = _index([5, 6, 70000], [3, 9, 4])
    _check(eng, a, [6], [5], "setValue: an update")
    _check(eng, a, [7], [5], "setValue: an insert")
    _check(eng, _index([], []), [0], [0], "setValue(0, 0) into nothing: one empty slice")


def test_updates_and_inserts(eng):
    """updates alone, inserts alone, both; new keys below, between and above the operand's, keys 0 and 65535"""
    rng = np.random.default_rng(3)
    cols = np.concatenate([(k << 16) + rng.choice(65536, s, replace=False) for k, s in ((2, 3000), (9, 20000), (700, 50))])
    a = _index(cols, rng.integers(0, 1 << 12, cols.size))
    upd = rng.choice(cols, 4000, replace=False)
    ins = np.concatenate([rng.integers(0, 65536, 300), (1 << 16) + rng.integers(0, 65536, 10),
                          (5 << 16) + rng.integers(0, 65536, 5000), (9 << 16) + rng.integers(0, 65536, 100),
                          (65535 << 16) + rng.integers(0, 65536, 70), [0, 0xFFFFFFFF, 0xFFFF0000]])
    ins = np.setdiff1d(ins, cols)
    for tag, c in (("updates", upd), ("inserts", ins), ("both", rng.permutation(np.concatenate([upd, ins])))):
        w = _check(eng, a, c, rng.integers(0, 1 << 12, c.size), tag)
        assert O.stats(w.ebm)["card"] == cols.size + (0 if tag == "updates" else ins.size)


def test_bits_cleared(eng):
    a = _index([5, 6, (4 << 16) + 1, (4 << 16) + 2], [7, 1, 4, 4])
    w = _check(eng, a, [5], [0], "7 overwritten by 0")
    assert _values(w, np.array([5, 6])).tolist() == [0, 1] and O.to_values(w.ebm).size == 4
    w = _check(eng, a, [(4 << 16) + 1, (4 << 16) + 2], [1, 2], "slice 2 loses its container of key 4")
    assert O.to_values(w.ba[2]).tolist() == [5] and O.stats(w.ba[2])["array"] == 1 and w.bit_count() == 3
    w = _check(eng, a, [5, 6], [2, 2], "slice 0 left empty, key 0 gone from slices 0 and 2")
    assert w.ba[0] == _bsi.EMPTY and O.to_values(w.ba[2]).tolist() == [(4 << 16) + 1, (4 << 16) + 2]


def test_type_boundaries(eng):
    base = (9 << 16) + np.random.default_rng(7).permutation(65536)
    a = _index(base[:4096], np.ones(4096))
    w = _check(eng, a, base[4096:4097], [1], "4096 -> 4097 by insert: slice 0 and ebM")
    assert _kinds(w.ba[0]) == (0, 1, 0) and _kinds(w.ebm) == (0, 1, 0)
    w2 = _check(eng, w, base[:1], [0], "4097 -> 4096 by an overwrite that clears")
    assert _kinds(w2.ba[0]) == (1, 0, 0) and _kinds(w2.ebm) == (0, 1, 0)
    w3 = _check(eng, a, base[5000:5001], [0], "ebM alone 4096 -> 4097")
    assert _kinds(w3.ebm) == (0, 1, 0) and _kinds(w3.ba[0]) == (1, 0, 0)
    full = _index((2 << 16) + np.arange(65535), np.full(65535, 3))
    w4 = _check(eng, full, [(2 << 16) + 65535], [3], "65,535 -> 65,536: a bitmap, not a run")
    assert [_kinds(x) for x in _all(w4)] == [(0, 1, 0)] * 3 and O.stats(w4.ebm)["card"] == 65536


def test_depth_rule(eng):
    a = _index([5, 6, 70000], [3, 9, 4])
    w = _check(eng, a, [6, 8, 6], [3, 0x1F5, 4], "grow by several slices")
    assert (w.bit_count(), w.min, w.max) == (9, 3, 0x1F5)
    w = _check(eng, a, [5, 7], [1, 2], "min only")
    assert (w.bit_count(), w.min, w.max) == (4, 1, 9)
    w = _check(eng, a, [6], [5], "neither: the overwritten maximum stays")
    assert (w.bit_count(), w.min, w.max) == (4, 3, 9)
    w = _check(eng, a, [5, 7], [1, 0x1F5], "both exceeded: high bits dropped, max unchanged")
    assert (w.bit_count(), w.min, w.max) == (4, 1, 9) and _values(w, np.array([5, 7])).tolist() == [1, 5]
    deep = BSI(a.ebm, a.ba + [_bsi.EMPTY] * 3, 3, 9)  # a caller's nbits above bitlen(max)
    w = _check(eng, deep, [6, 9], [100, 2], "seven slices: 100 fits, min alone moves")
    assert (w.bit_count(), w.min, w.max) == (7, 2, 9) and _values(w, np.array([6])).tolist() == [100]
    w = _check(eng, deep, [6], [300], "seven slices grow to nine")
    assert (w.bit_count(), w.min, w.max) == (9, 3, 300)


def test_thirty_two_slices_from_bsi_add(eng):
    """2^31 - 1 + 1 at column 5: the sum has 32 slices and slice 31 always loses a written column"""
    wide, one = _index([5, 70000], [2**31 - 1, 3]), _index([5], [1])
    iw, io = eng.load(_all(wide)), eng.load(_all(one))
    top, nb, mn, mx = eng.bsi_add(iw, 31, io, 1)
    assert (nb, mn, mx) == (32, 3, -2**31)
    a = BSI(_fetch(eng, top)[0], _fetch(eng, top)[1:], mn, mx)
    cols, vals = np.array([5, 6, 5]), np.array([5, 2**31 - 1, 7])
    want = set_reference(a, cols, vals)
    r, nb2, mn2, mx2 = eng.bsi_set_values(top, 32, cols, vals, mn, mx)
    assert _fetch(eng, r) == _all(want) and (nb2, mn2, mx2) == (32, 3, 2**31 - 1) == (want.bit_count(), want.min, want.max)
    assert want.ba[31] == _bsi.EMPTY and _values(want, np.array([5, 6])).tolist() == [7, 2**31 - 1]
    for x in (iw, io, top, r):
        eng.release(x)


def test_repeated_columns(eng):
    rng = np.random.default_rng(17)
    a = _index((3 << 16) + np.arange(0, 2000, 2), rng.integers(0, 256, 1000))
    w = _check(eng, a, [(3 << 16) + 10, (3 << 16) + 10], [0xAA, 0x55], "two copies in one wave")
    assert _values(w, np.array([(3 << 16) + 10])).tolist() == [0x55]
    c = (3 << 16) + rng.permutation(100000)[:100000] % 65536 + (rng.integers(0, 3, 100000) << 16)
    c[0] = c[-1] = 123456789
    c[1:-1][c[1:-1] == 123456789] += 1
    v = rng.integers(0, 256, 100000)
    v[0], v[-1] = 0xF0, 0x0F
    w = _check(eng, a, c, v, "copies at pair indices 0 and n - 1 of 100,000")
    assert _values(w, np.array([123456789])).tolist() == [0x0F]
    v = rng.integers(0, 256, 4096)
    w = _check(eng, a, np.full(4096, (3 << 16) + 11), v, "one column 4,096 times")
    assert _values(w, np.array([(3 << 16) + 11])).tolist() == [int(v[-1])] and O.stats(w.ebm)["card"] == 1001


_nine = {}


def _nine_case():
    """an index of 154,000 columns over nine keys (arrays, bitmaps, the 4096 / 4097 boundary, a missing key) and
    200,000 pairs over the same nine keys, a tenth of them repeats of earlier columns with other values"""
    if not _nine:
        rng = np.random.default_rng(9)
        keys = np.array([0, 1, 7, 40, 41, 300, 4000, 65534, 65535], dtype=np.int64)
        cols = np.concatenate([(k << 16) + rng.choice(65536, s, replace=False)
                               for k, s in zip(keys, [30000, 100, 60000, 0, 5, 4096, 4097, 20000, 35000])])
        a = _index(cols, rng.integers(0, 1 << 20, cols.size))
        d = np.concatenate([(k << 16) + rng.choice(65536, 20000, replace=False) for k in keys])
        bc = np.concatenate([d, rng.choice(d, 20000, replace=False)])
        bv = rng.integers(0, 1 << 20, bc.size)
        _nine.update(a=a, cols=cols, bc=bc, bv=bv, rng=rng)
    return _nine


@pytest.mark.parametrize("order", ["given", "reversed", "by_column", "shuffled_1", "shuffled_2"])
def test_nine_keys_in_five_orders(eng, order):
    n = _nine_case()
    bc, bv = n["bc"], n["bv"]
    p = {"given": np.arange(bc.size), "reversed": np.arange(bc.size)[::-1], "by_column": np.argsort(bc, kind="stable"),
         "shuffled_1": np.random.default_rng(1).permutation(bc.size),
         "shuffled_2": np.random.default_rng(2).permutation(bc.size)}[order]
    assert bc.size == 200000 and np.unique(bc).size == 180000
    w = _check(eng, n["a"], bc[p], bv[p], order)
    if order == "given":
        n["want"] = w


@pytest.mark.parametrize("budget", ["one_key", "1", "two_keys"])
def test_forced_passes(eng, monkeypatch, budget):
    """the workspace budget forced down through the environment switch: whole keys per pass, every pass resolves
    the repeats of its own keys"""
    n = _nine_case()
    want = n.get("want") or set_reference(n["a"], n["bc"], n["bv"])
    key_bytes = 8192 * (1 + want.bit_count()) + 4 * 65536
    nbytes = {"one_key": key_bytes, "1": 1, "two_keys": 2 * key_bytes + 100}[budget]
    assert -(-9 // max(1, nbytes // key_bytes)) >= 3  # nine keys: at least three passes
    monkeypatch.setenv("RBG_BSI_BUILD_WS", str(nbytes))
    _check(eng, n["a"], n["bc"], n["bv"], budget, want=want)
    monkeypatch.delenv("RBG_BSI_BUILD_WS")
    _check(eng, n["a"], n["bc"], n["bv"], "default again", want=want)


def _full_run_index():
    rng = np.random.default_rng(21)
    cols = np.concatenate([(1 << 16) + np.arange(65536), (3 << 16) + np.arange(65536),
                           (6 << 16) + rng.choice(65536, 5000, replace=False)])
    a = _index(cols, rng.integers(0, 1 << 10, cols.size))
    a.ebm = O.run_optimize(a.ebm)
    assert _kinds(a.ebm) == (0, 1, 2) or _kinds(a.ebm) == (1, 0, 2)
    assert not any(_kinds(s)[2] for s in a.ba)
    return a, rng


def test_full_run_existence_bitmap(eng):
    """ebM with two full run containers and bitmap slices: updates inside them, inserts in other keys"""
    a, rng = _full_run_index()
    upd = (1 << 16) + rng.choice(65536, 3000, replace=False)
    w = _check(eng, a, upd, rng.integers(0, 1 << 10, 3000), "updates inside a full run container")
    assert w.ebm == a.ebm
    ins = np.concatenate([rng.integers(0, 65536, 200), (2 << 16) + rng.integers(0, 65536, 6000),
                          (6 << 16) + rng.integers(0, 65536, 50), (9 << 16) + rng.integers(0, 65536, 5)])
    c = rng.permutation(np.concatenate([upd, ins, (3 << 16) + np.arange(100)]))
    w = _check(eng, a, c, rng.integers(0, 1 << 10, c.size), "updates inside and inserts in other keys")
    assert _kinds(w.ebm)[2] == 2
    w = _check(eng, w, [(3 << 16) + 5, (7 << 16) + 5], [1000, 3000], "on its own result, growing")
    assert _kinds(w.ebm)[2] == 2 and w.bit_count() == 12


def _first_free(eng):
    """the lowest free batch slot: a leaked batch would take it"""
    probe = eng.from_values([1])
    eng.release(probe)
    return probe


def test_refusals_leave_no_batch(eng):
    import roaringbitmap_amd as rb
    from roaringbitmap_amd import _lib as L
    a = _index([5, 6, 70000], [3, 9, 4])
    ro = BSI.from_columns(np.arange(1000), np.arange(1000) // 100, True)
    assert _kinds(ro.ebm)[2] == 1 and any(_kinds(s)[2] for s in ro.ba)
    part = BSI(ro.ebm, [O.remove_run_compression(s) for s in ro.ba], ro.min, ro.max)  # a run of 1,000 in ebM alone
    slice_run = BSI(O.remove_run_compression(ro.ebm), ro.ba, ro.min, ro.max)
    ia, ip, isl = eng.load(_all(a)), eng.load(_all(part)), eng.load(_all(slice_run))
    free = _first_free(eng)
    one, v = np.array([5]), np.array([1])
    with pytest.raises(rb.IllegalArgumentException, match="run container"):
        eng.bsi_set_values(isl, ro.bit_count(), one, v, ro.min, ro.max)
    assert _first_free(eng) == free
    with pytest.raises(rb.IllegalArgumentException, match="run container"):
        eng.bsi_set_values(ip, ro.bit_count(), one, v, ro.min, ro.max)
    assert _first_free(eng) == free
    with pytest.raises(rb.IllegalArgumentException, match="non-negative"):
        eng.bsi_set_values(ia, 4, [5, 6], [1, -1], 3, 9)
    c2, v2 = (ctypes.c_uint32 * 2)(5, 6), (ctypes.c_int32 * 2)(1, -1)  # past the Python check: the device's
    out, out3 = ctypes.c_int32(-7), (ctypes.c_int32 * 3)()
    assert L.lib().rbg_ctx_bsi_set_values(eng._ctx, ia, 4, 3, 9, c2, v2, 2, ctypes.byref(out), out3) == \
        L.RBG_ERR_ILLEGAL_ARGUMENT and out.value == -7
    assert b"non-negative" in L.lib().rbg_last_error()
    assert _first_free(eng) == free
    with pytest.raises(rb.IllegalArgumentException, match="no pair"):
        eng.bsi_set_values(ia, 4, [], [], 3, 9)
    assert _first_free(eng) == free
    for nbits in (3, 5, 33, -1):  # n_bm != 1 + nbits, more slices than an int has bits
        with pytest.raises(rb.IllegalArgumentException):
            eng.bsi_set_values(ia, nbits, one, v, 3, 9)
    packed = eng.load(_all(a), packed=True)
    with pytest.raises(rb.IllegalArgumentException, match="key-major, unpacked"):
        eng.bsi_set_values(packed, 4, one, v, 3, 9)
    eng.release(packed)
    assert _first_free(eng) == free
    r, nb, mn, mx = eng.bsi_set_values(ia, 4, one, v, 3, 9)
    assert r == free and _fetch(eng, r) == _all(set_reference(a, one, v)) and (nb, mn, mx) == (4, 1, 9)
    for x in (ia, ip, isl, r):
        eng.release(x)


def test_result_as_an_index_operand(eng):
    """the result against the loaded batch of the oracle's bitmaps in compare + sum, its pairs against the
    replay, then written to again and added to itself"""
    n = _nine_case()
    a, bc, bv = n["a"], n["bc"], n["bv"]
    want = n.get("want") or set_reference(a, bc, bv)
    ia = eng.load(_all(a))
    built, nb, mn, mx = eng.bsi_set_values(ia, a.bit_count(), bc, bv, a.min, a.max)
    loaded = eng.load(_all(want))
    assert eng.batch_stats(built) == eng.batch_stats(loaded)
    assert (eng.batch_counts(built) == eng.batch_counts(loaded)).all()
    cols, vals = replay_values(n["cols"], _values(a, n["cols"]), bc, bv, nb)
    for op, lo, hi in (("EQ", int(vals[5]), 0), ("RANGE", 1000, 300000), ("GE", 1 << 19, 0)):
        res = []
        for x in (built, loaded):
            eng.bsi(x, op, nb, lo, hi, mn, mx, want_sum=True)
            res.append((eng.fetch().serialize(), eng.bsi_sums()))
        assert res[0] == res[1] and res[0][0] == want.compare(op, lo, hi), (op, lo, hi)
        assert res[0][1] == want.sum(res[0][0])
    pc, pv = eng.bsi_to_pairs(built, nb)
    assert (pc == cols).all() and (pv == vals).all()
    c2, v2 = np.concatenate([cols[::50], [12 << 16]]), np.concatenate([vals[::50] ^ 1, [1 << 22]])
    want2 = set_reference(want, c2, v2)
    again, nb2, mn2, mx2 = eng.bsi_set_values(built, nb, c2, v2, mn, mx)
    assert _fetch(eng, again) == _all(want2) and (nb2, mn2, mx2) == (want2.bit_count(), want2.min, want2.max)
    dbl, nb3, mn3, mx3 = eng.bsi_add(built, nb, built, nb)
    d = BSI(_fetch(eng, dbl)[0], _fetch(eng, dbl)[1:], mn3, mx3)
    assert not _kinds(d.ebm)[2]
    want3 = set_reference(d, c2, v2)
    r3, nb4, mn4, mx4 = eng.bsi_set_values(dbl, nb3, c2, v2, mn3, mx3)
    assert _fetch(eng, r3) == _all(want3) and (nb4, mn4, mx4) == (want3.bit_count(), want3.min, want3.max)
    for x in (ia, built, loaded, again, dbl, r3):
        eng.release(x)


def test_torch_device_inputs(eng):
    import torch
    n = _nine_case()
    a, bc, bv = n["a"], n["bc"][:50000], n["bv"][:50000]
    want = set_reference(a, bc, bv)
    ia = eng.load(_all(a))
    dev = torch.device("cuda", 0)
    for ct, vt in ((torch.int64, torch.int64), (torch.int64, torch.int32)):
        c = torch.tensor(bc, dtype=torch.int64, device=dev).to(ct)
        v = torch.tensor(bv, dtype=torch.int64, device=dev).to(vt)
        r, nb, mn, mx = eng.bsi_set_values(ia, a.bit_count(), c, v, a.min, a.max)
        assert _fetch(eng, r) == _all(want) and (nb, mn, mx) == (want.bit_count(), want.min, want.max)
        eng.release(r)
    free = _first_free(eng)
    import roaringbitmap_amd as rb
    with pytest.raises(rb.IllegalArgumentException, match="non-negative"):
        eng.bsi_set_values(ia, a.bit_count(), torch.tensor([5, 6], dtype=torch.int64, device=dev),
                           torch.tensor([1, -1], dtype=torch.int32, device=dev), a.min, a.max)
    assert _first_free(eng) == free
    eng.release(ia)


def _rb_index(cls, o):
    import roaringbitmap_amd as rb
    x = cls(rb.RoaringBitmap(o.ebm), [rb.RoaringBitmap(s) for s in o.ba], o.min, o.max)
    x.runOptimized = o.run_optimized
    return x


def _rb_bytes(x):
    return [x.ebM.serialize()] + [s.serialize() for s in x.bA], x.bitCount(), x.minValue, x.maxValue


@pytest.mark.parametrize("cls_name", ["RoaringBitmapSliceIndex", "MutableBitSliceIndex"])
def test_python_classes_and_the_one_shot(gpu, cls_name):
    import roaringbitmap_amd as rb
    cls = getattr(rb, cls_name)
    n = _nine_case()
    a, bc, bv = n["a"], n["bc"][-60000:], n["bv"][-60000:]
    want = set_reference(a, bc, bv)
    x = _rb_index(cls, a)
    x.setValues(bc, bv, gpu=True)
    assert _rb_bytes(x) == (_all(want), want.bit_count(), want.min, want.max) and x.runOptimized is False
    y = _rb_index(cls, a)
    y.setValues(bc, bv)  # the host form: the same object
    assert _rb_bytes(y) == _rb_bytes(x)
    f, _ = _full_run_index()
    z = _rb_index(cls, f)
    c, v = np.array([(1 << 16) + 9, (8 << 16) + 1, (1 << 16) + 9]), np.array([5, 6, 7])
    z.setValues(c, v, gpu=True)  # an ebM with full run containers and a new column: the device form alone
    wz = set_reference(f, c, v)
    assert _rb_bytes(z) == (_all(wz), wz.bit_count(), wz.min, wz.max)
    ro = BSI.from_columns(np.arange(1000), np.arange(1000) // 100, True)
    q = _rb_index(cls, ro)
    with pytest.raises(rb.IllegalArgumentException, match="run container"):
        q.setValues([5], [1], gpu=True)
    assert _rb_bytes(q)[0] == _all(ro)
