"""Values out of a resident bit-sliced index on the MI355X (rbg_ctx_bsi_get_values[_device],
rbg_ctx_bsi_to_pairs[_device], rbg_bsi_get_values): RoaringBitmapSliceIndex.getValue (BSI/:181-196) for many
columns at once, the loop body of batchIn / transposeWithCount (BBSI/:551-639), and toPairList()
(BBSI/:534-549), against the oracle's getValue (tests/_bsi.py) over loaded and built batches."""
import numpy as np
import pytest

import _gen
import _oracle as O
from _bsi import BSI

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng(gpu):
    import roaringbitmap_amd as rb
    e = rb.Engine(0)
    yield e
    e.close()


def _mix():
    """nine keys, 65535 among them, whose ebM containers are arrays, bitmaps and (run-optimized) runs; the
    values of key 40 are clustered so its slices hold runs too"""
    rng = np.random.default_rng(61)
    keys = np.sort(np.concatenate([rng.choice(65000, 8, replace=False), [65535]]))
    cols = O.to_values(_gen.bitmap(rng, keys, p_present=1.0)).astype(np.int64)
    vals = rng.integers(0, 1 << 18, size=cols.size)
    k3 = (cols >> 16) == keys[3]
    vals[k3] = (cols[k3] & 0xFFFF) // 700
    return keys, cols, vals


KEYS, COLS, VALS = _mix()
_cache = {}


def _index():
    """the run-optimized oracle index, its column -> value map and the queries (shared, left unchanged)"""
    if not _cache:
        o = BSI.from_columns(COLS, VALS, True)
        kinds = [O.stats(b) for b in [o.ebm] + o.ba]
        assert all(sum(k[t] for k in kinds) > 0 for t in ("array", "bitmap", "run")), kinds
        rng = np.random.default_rng(62)
        present = rng.choice(COLS, 3000)
        lows = rng.integers(0, 65536, size=2000)
        under_present_keys = (rng.choice(KEYS, 2000).astype(np.int64) << 16) | lows
        absent_keys = (rng.choice(np.setdiff1d(np.arange(65536), KEYS), 500).astype(np.int64) << 16) | lows[:500]
        # just outside every run of ebM: the value before each run's start and after its end
        sc = np.sort(COLS)
        brk = np.nonzero(np.diff(sc) != 1)[0]
        edges = np.concatenate([sc[brk] + 1, sc[brk + 1] - 1, [sc[0] - 1, sc[-1] + 1]])
        edges = edges[(edges >= 0) & (edges < 1 << 32)]
        q = np.concatenate([present, under_present_keys, absent_keys, edges, [0, 0xFFFFFFFF], present[:100]])
        q = rng.permutation(q)
        lut = dict(zip(COLS.tolist(), VALS.tolist()))
        exp = np.array([lut.get(int(c), -1) for c in q], dtype=np.int64)
        for c in q[:12]:  # the map is the oracle's getValue
            v, ok = o.get_value(int(c))
            assert (v if ok else -1) == lut.get(int(c), -1)
        assert (exp == -1).sum() > 1000 and (exp >= 0).sum() > 3000
        _cache.update(o=o, q=q, exp=exp)
    return _cache["o"], _cache["q"], _cache["exp"]


@pytest.fixture(scope="module")
def batches(eng):
    o, _, _ = _index()
    loaded = eng.load([o.ebm] + o.ba)
    built, nbits, mn, mx = eng.bsi_from_columns(COLS, VALS, True)
    assert nbits == o.bit_count()
    found = O.from_values(COLS[::5])
    with_found = eng.load([o.ebm] + o.ba + [found])
    yield {"loaded": loaded, "built": built, "with_found": with_found}
    for b in (loaded, built, with_found):
        eng.release(b)


@pytest.mark.parametrize("which", ["loaded", "built", "with_found"])
def test_get_values(eng, batches, which):
    o, q, exp = _index()
    got = eng.bsi_get_values(batches[which], o.bit_count(), q, has_found=which == "with_found")
    assert got.dtype == np.int64 and got.shape == q.shape
    assert (got == exp).all(), np.nonzero(got != exp)[0][:10]


def test_get_values_torch_and_one_shot(eng, batches):
    import torch
    import roaringbitmap_amd as rb
    o, q, exp = _index()
    t = torch.from_numpy(q).to("cuda:0")
    got = eng.bsi_get_values(batches["built"], o.bit_count(), t)
    assert got.dtype == torch.int64 and got.device == t.device and (got.cpu().numpy() == exp).all()
    t32 = torch.from_numpy(q.astype(np.uint32).view(np.int32)).to("cuda:0").view(torch.uint32)
    assert (eng.bsi_get_values(batches["loaded"], o.bit_count(), t32).cpu().numpy() == exp).all()
    assert eng.bsi_get_values(batches["built"], o.bit_count(), torch.zeros(0, dtype=torch.int64, device="cuda:0")).numel() == 0
    assert eng.bsi_get_values(batches["built"], o.bit_count(), []).size == 0
    x = rb.RoaringBitmapSliceIndex(rb.RoaringBitmap(o.ebm), [rb.RoaringBitmap(b) for b in o.ba], o.min, o.max)
    assert (x.getValues(q, gpu=True) == exp).all() and (x.getValues(q) == exp).all()
    with pytest.raises(rb.IllegalArgumentException):  # the batch holds no foundSet / more slices than nbits says
        eng.bsi_get_values(batches["built"], o.bit_count(), q, has_found=True)
    with pytest.raises(rb.IllegalArgumentException):
        eng.bsi_get_values(batches["built"], o.bit_count() - 1, q)


@pytest.mark.parametrize("which", ["loaded", "built", "with_found"])
def test_to_pairs(eng, batches, which):
    o, _, _ = _index()
    order = np.argsort(COLS)
    c, v = eng.bsi_to_pairs(batches[which], o.bit_count(), has_found=which == "with_found")
    assert c.dtype == np.uint32 and v.dtype == np.int32
    assert (c == COLS[order]).all() and (v == VALS[order]).all()


def test_to_pairs_torch_without_sync_and_size_query(eng, batches):
    import torch
    o, _, _ = _index()
    order = np.argsort(COLS)
    assert eng.bsi_pairs_count(batches["built"], o.bit_count()) == COLS.size  # null outputs: the size alone
    for dt, vt in ((torch.uint32, torch.int32), (torch.int64, torch.int64)):
        c, v = eng.bsi_to_pairs(batches["built"], o.bit_count(), dtype=dt)
        assert c.dtype == dt and v.dtype == vt and c.numel() == v.numel() == COLS.size
        # used on torch's current stream with no engine or device sync in between
        s = (c.view(torch.int32) if dt == torch.uint32 else c).to(torch.int64)
        s = torch.where(s < 0, s + (1 << 32), s)
        total = (s * 3 + v.to(torch.int64)).sum()
        assert int(total) == int((COLS * 3 + VALS).sum())
        assert (s.cpu().numpy() == COLS[order]).all() and (v.cpu().numpy() == VALS[order]).all()
    with pytest.raises(ValueError):
        eng.bsi_to_pairs(batches["built"], o.bit_count(), dtype=torch.float32)


@pytest.mark.parametrize("ro", [False, True])
def test_round_trip(eng, ro):
    """build -> to_pairs -> build again: the same bytes"""
    rng = np.random.default_rng(70 + ro)
    p = rng.permutation(COLS.size)
    b1, nbits, mn, mx = eng.bsi_from_columns(COLS[p], VALS[p], ro)
    c, v = eng.bsi_to_pairs(b1, nbits)
    b2, nbits2, mn2, mx2 = eng.bsi_from_columns(c, v, ro)
    assert (nbits, mn, mx) == (nbits2, mn2, mx2)
    f1 = [x.serialize() for x in eng.batch_fetch_range(b1)]
    assert f1 == [x.serialize() for x in eng.batch_fetch_range(b2)]
    o = BSI.from_columns(COLS, VALS, ro)
    assert f1 == [o.ebm] + o.ba
    eng.release(b1)
    eng.release(b2)


def test_empty_and_all_zero(eng):
    e, nbits, _, _ = eng.bsi_from_columns([], [])
    assert eng.bsi_get_values(e, nbits, [0, 5, 0xFFFFFFFF]).tolist() == [-1, -1, -1]
    c, v = eng.bsi_to_pairs(e, nbits)
    assert c.size == 0 and v.size == 0 and eng.bsi_pairs_count(e, nbits) == 0
    eng.release(e)
    z, nbits, _, _ = eng.bsi_from_columns([9, 70000], [0, 0])
    assert nbits == 1 and eng.bsi_get_values(z, nbits, [9, 10, 70000]).tolist() == [0, -1, 0]
    c, v = eng.bsi_to_pairs(z, nbits)
    assert c.tolist() == [9, 70000] and v.tolist() == [0, 0]
    eng.release(z)


def test_one_million_pairs(eng):
    """1 M pairs with 31-bit values over 64 keys: the pairs come back in column order"""
    rng = np.random.default_rng(80)
    cols = rng.choice(64 << 16, 1_000_000, replace=False).astype(np.int64)
    vals = rng.integers(0, 1 << 31, size=cols.size)
    vals[0] = 2**31 - 1
    b, nbits, mn, mx = eng.bsi_from_columns(cols, vals)
    assert (nbits, mn, mx) == (31, int(vals.min()), 2**31 - 1)
    c, v = eng.bsi_to_pairs(b, nbits)
    order = np.argsort(cols)
    assert (c == cols[order]).all() and (v == vals[order]).all()
    q = rng.permutation(np.concatenate([cols[:50000], (64 << 16) + np.arange(1000)]))
    lut = np.full(65 << 16, -1, dtype=np.int64)
    lut[cols] = vals
    assert (eng.bsi_get_values(b, nbits, q) == lut[q]).all()
    eng.release(b)


def test_to_pair_list_with_a_found_set(gpu):
    import roaringbitmap_amd as rb
    o, _, _ = _index()
    x = rb.RoaringBitmapSliceIndex(rb.RoaringBitmap(o.ebm), [rb.RoaringBitmap(b) for b in o.ba], o.min, o.max)
    rng = np.random.default_rng(81)
    found = rb.RoaringBitmap.from_values(np.concatenate([COLS[::7], rng.integers(0, 1 << 32, size=3000)]))
    for f in (None, found):
        hc, hv = x.toPairList(f)
        gc, gv = x.toPairList(f, gpu=True)
        assert hc.dtype == gc.dtype == np.uint32 and (hc == gc).all() and (hv == gv).all()
    hc, hv = x.toPairList(found)
    keep = np.isin(COLS, found.toArray())
    order = np.argsort(COLS[keep])
    assert (hc == COLS[keep][order]).all() and (hv == VALS[keep][order]).all()
