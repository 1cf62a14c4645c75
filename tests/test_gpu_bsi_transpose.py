"""GROUP BY value / COUNT(*) over a resident bit-sliced index on the MI355X (rbg_ctx_bsi_transpose,
rbg_bsi_transpose; BitSliceIndexBase.parallelTransposeWithCount, BBSI/:551-597).  The acceptance throughout: every
bitmap of the result batch, fetched, is byte for byte the reference's sequence composed on the CPU oracle
(tests/_bsi_transpose.py transpose_reference), with its {nbits, min, max}, through Engine.bsi_transpose and
through the Python class's one-shot, and the batch behaves as a built or loaded index does."""
import numpy as np
import pytest

import _bsi
import _gen
import _oracle as O
from _bsi import BSI
from _bsi_transpose import (FULL_KEY, full_case, index_of, random_index, transpose_counts, transpose_reference)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng(gpu):
    import roaringbitmap_amd as rb
    e = rb.Engine(0)
    yield e
    e.close()


@pytest.fixture(autouse=True, params=["count", "sort"])
def route(request, monkeypatch):
    """every test under both routes: the count tables (csrc/bsitr.hip), and the sort + run-length encode + build
    route that sparse shapes take by themselves (forced, it still yields to the count tables in a call that could
    produce a run container).  test_route_chosen_by_density runs without the switch."""
    monkeypatch.setenv("RBG_BSI_TR_ROUTE", request.param)
    return request.param


def _kinds(buf):
    s = O.stats(buf)
    return s["array"], s["bitmap"], s["run"]


def _fetch(eng, r, nbits):
    return [x.serialize() for x in eng.batch_fetch_range(r, 0, 1 + nbits)]


def _same(got, nbits, mn, mx, want, tag=""):
    assert (nbits, mn, mx) == (want.bit_count(), want.min, want.max), tag
    assert len(got) == 1 + nbits
    assert got[0] == want.ebm, (tag, O.stats(got[0]), O.stats(want.ebm))
    for i, (g, w) in enumerate(zip(got[1:], want.ba)):
        assert g == w, (tag, i, O.stats(g), O.stats(w))


def _device(eng, o, parallelism=1, found=None):
    b = eng.load([o.ebm] + o.ba + ([found] if found is not None else []))
    r, nbits, mn, mx = eng.bsi_transpose(b, o.bit_count(), parallelism, has_found=found is not None)
    got = _fetch(eng, r, nbits)
    assert eng.batch_stats(r)["bitmaps"] == 1 + nbits
    eng.release(r)
    eng.release(b)
    return got, nbits, mn, mx


def _one_shot(o, parallelism=1, found=None):
    import roaringbitmap_amd as rb
    x = rb.MutableBitSliceIndex(rb.RoaringBitmap(o.ebm), [rb.RoaringBitmap(s) for s in o.ba], o.min, o.max)
    t = x.parallelTransposeWithCount(None if found is None else rb.RoaringBitmap(found), parallelism, pool=None)
    assert type(t) is type(x)
    return [t.ebM.serialize()] + [s.serialize() for s in t.bA], len(t.bA), t.minValue, t.maxValue


def _check(eng, o, parallelism=1, found=None, tag="", want=None, one_shot=False):
    want = transpose_reference(o, found, parallelism) if want is None else want
    _same(*_device(eng, o, parallelism, found), want, tag)
    if one_shot:
        _same(*_one_shot(o, parallelism, found), want, tag)
    return want


def test_known_answer(eng):
    """BufferBSITest.testTransposeWithCount"""
    x = np.arange(1, 100)
    r = _check(eng, BSI.from_columns(x, np.where(x <= 30, 1, np.where(x <= 60, 2, 3))), 2, one_shot=True)
    assert O.to_values(r.ebm).tolist() == [1, 2, 3] and (r.bit_count(), r.min, r.max) == (6, 30, 39)


# ---- the nine-key array / bitmap / run mix ---------------------------------------------------------------------------

_cache = {}


def _nine():
    """nine keys, 65535 among them, whose ebM containers are arrays, bitmaps and (run-optimized) runs; key 3's
    values are clustered so its slices hold runs too; a foundSet whose keys and columns only partly overlap ebM;
    both references (shared, left unchanged)"""
    if not _cache:
        rng = np.random.default_rng(61)
        keys = np.sort(np.concatenate([rng.choice(65000, 8, replace=False), [65535]]))
        cols = O.to_values(_gen.bitmap(rng, keys, p_present=1.0)).astype(np.int64)
        low = cols & 0xFFFF  # the two full keys cut down to one run each: under 200,000 columns in all
        k4, k7 = (cols >> 16) == keys[4], (cols >> 16) == keys[7]
        cols = cols[~(k4 & (low >= 20000)) & ~(k7 & ((low < 1000) | (low >= 31000)))]
        vals = rng.integers(0, 1 << 18, size=cols.size) >> rng.integers(0, 14, size=cols.size)
        k3 = (cols >> 16) == keys[3]
        vals[k3] = (cols[k3] & 0xFFFF) // 700
        o = BSI.from_columns(cols, vals, True)
        kinds = [O.stats(b) for b in [o.ebm] + o.ba]
        assert all(sum(k[t] for k in kinds) > 0 for t in ("array", "bitmap", "run")), kinds
        extra = np.concatenate([rng.integers(0, 1 << 32, size=3000), (int(keys[2]) << 16) + rng.integers(0, 65536, 500)])
        found_cols = np.unique(np.concatenate([cols[::5], cols[(cols >> 16) == keys[7]], extra]))
        found = O.run_optimize(O.from_values(found_cols))
        _cache.update(o=o, cols=cols, vals=vals, found=found, found_cols=found_cols,
                      want=transpose_reference(o, None, 3), want_found=transpose_reference(o, found, 3))
        assert cols.size <= 200000 and _cache["want"].bit_count() >= 8
    return _cache


def test_nine_keys_loaded(eng):
    c = _nine()
    _check(eng, c["o"], 3, want=c["want"], one_shot=True)


def test_nine_keys_built_on_the_device(eng):
    c = _nine()
    b, nbits, _, _ = eng.bsi_from_columns(c["cols"], c["vals"], True)
    r, n2, mn, mx = eng.bsi_transpose(b, nbits, 3)
    _same(_fetch(eng, r, n2), n2, mn, mx, c["want"])
    eng.release(r)
    eng.release(b)


def test_nine_keys_with_a_trailing_found_set(eng):
    c = _nine()
    _check(eng, c["o"], 3, c["found"], want=c["want_found"], one_shot=True)


@pytest.mark.parametrize("budget", ["one_key", "two_keys", "1"])
def test_forced_passes(eng, monkeypatch, budget):
    """the workspace budget forced down through the environment switch: whole result keys per pass (a count table
    of 256 KiB and one cell of 8 KiB for ebM and per bit of the column count), the same bytes"""
    c = _nine()
    per_key = 4 * 65536 + 8192 * (1 + int(c["cols"].size).bit_length())
    nbytes = {"one_key": per_key, "two_keys": 2 * per_key + 100, "1": 1}[budget]
    monkeypatch.setenv("RBG_BSI_BUILD_WS", str(nbytes))
    _check(eng, c["o"], 3, want=c["want"])
    _check(eng, c["o"], 3, c["found"], want=c["want_found"])
    monkeypatch.delenv("RBG_BSI_BUILD_WS")
    _check(eng, c["o"], 3, want=c["want"])


@pytest.mark.parametrize("parallelism", [1, 2, 7, 30])
def test_parallelism(eng, parallelism):
    c = _nine()
    _check(eng, c["o"], parallelism, tag=parallelism)


# ---- slices, widths, counts ----------------------------------------------------------------------------------------

def test_slice_without_a_container_and_zero_values(eng):
    """key 4 holds even values alone (slice 0 has no container there), key 6 the value 0 alone (no slice has one),
    key 8 odd values; the value 0 becomes column 0"""
    c4, c6, c8 = (4 << 16) + np.arange(3000), (6 << 16) + np.arange(0, 500, 7), (8 << 16) + np.arange(100)
    o = BSI.from_columns(np.concatenate([c4, c6, c8]), np.concatenate([2 * (c4 % 13), 0 * c6, 2 * (c8 % 4) + 1]))
    assert O.to_values(o.ba[0]).tolist() == c8.tolist()
    r = _check(eng, o, 2, one_shot=True)
    assert O.to_values(r.ebm)[0] == 0 and O.to_values(r.ebm).size == 13 + 4
    z = BSI.from_columns([9, 70000], [0, 0])  # one (empty) slice
    r = _check(eng, z, 1)
    assert O.to_values(r.ebm).tolist() == [0] and (r.bit_count(), r.min, r.max) == (2, 2, 2)


def test_thirty_two_slices(eng):
    """hand-made slices: bit 31 gives result columns >= 2^31, 0xFFFFFFFF lands under result key 65535"""
    cols, vals, found_cols = random_index(21, wide=True)
    o = index_of(cols, vals, 32)
    r = _check(eng, o, 2, one_shot=True)
    got = O.to_values(r.ebm)
    assert int(got[-1]) == 0xFFFFFFFF and int(got[0]) == 0 and (got >= 1 << 31).sum() > 50
    _check(eng, o, 7, O.from_values(found_cols))
    short = BSI(o.ebm, o.ba[:31], 0, 0)  # 31 slices: no value reaches 2^31
    assert int(O.to_values(_check(eng, short, 2).ebm)[-1]) < 1 << 31


def test_one_value_over_four_keys(eng):
    """200,000 columns spread over four input keys hold one value: the count is summed across workgroups"""
    cols = np.concatenate([(k << 16) + np.arange(50000) for k in (1, 2, 40, 65535)])
    o = index_of(cols, np.full(cols.size, 77777))
    r = _check(eng, o, 5, one_shot=True)
    assert (r.bit_count(), r.min, r.max) == (18, 200000, 200000) and O.to_values(r.ebm).tolist() == [77777]


def test_three_distinct_values(eng):
    cols = np.concatenate([(k << 16) + np.arange(0, 60000, 2) for k in (0, 9)])
    vals = np.array([5, 1 << 20, (1 << 20) + 1])[np.arange(cols.size) % 3]
    r = _check(eng, index_of(cols, vals), 4)
    assert O.to_values(r.ebm).tolist() == [5, 1 << 20, (1 << 20) + 1] and r.min == r.max == 20000


@pytest.mark.parametrize("k", [1, 6, 12])
def test_counts_at_powers_of_two(eng, k):
    """values 1, 2, 3 held by 2^k - 1, 2^k and 2^k + 1 columns"""
    n = [(1 << k) - 1, 1 << k, (1 << k) + 1]
    cols = np.arange(sum(n)) * 5
    r = _check(eng, index_of(cols, np.repeat([1, 2, 3], n)), 2)
    assert (r.bit_count(), r.min, r.max) == (k + 1, n[0], n[2])
    only = np.arange(n[0]) * 3  # the largest count is 2^k - 1: k slices
    assert _check(eng, index_of(only, np.full(only.size, 9)), 1).bit_count() == k


@pytest.mark.parametrize("n,kind", [(4096, (1, 0, 0)), (4097, (0, 1, 0))])
def test_result_key_and_count_slice_thresholds(eng, n, kind):
    """result key 2 holds exactly n distinct values, each held twice (so count slice 1 holds exactly n columns
    there and slice 0 none); result key 5 one value held three times"""
    low = np.random.default_rng(n).permutation(65536)[:n]
    vals = np.concatenate([(2 << 16) + low, (2 << 16) + low, [5 << 16] * 3])
    cols = np.random.default_rng(n + 1).permutation(1 << 18)[:vals.size]
    r = _check(eng, index_of(cols, vals), 3)
    assert _kinds(r.ebm) == (kind[0] + 1, kind[1], 0) and _kinds(r.ba[1]) == (kind[0] + 1, kind[1], 0)
    assert O.stats(r.ba[0])["card"] == 1 and O.stats(r.ba[1])["card"] == n + 1


# ---- full result keys -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("number", [1, 2, 3, 4, 5, 6])
def test_full_key_cases(eng, number):
    cols, vals, parallelism, size, run = full_case(number)
    r = _check(eng, index_of(cols, vals), parallelism, tag=number, one_shot=number in (1, 2))
    assert _kinds(r.ebm) == ((0, 0, 1) if run else (0, 1, 0)), number
    assert O.stats(r.ebm)["card"] == 65536 and int(O.to_values(r.ebm)[0]) == FULL_KEY << 16


@pytest.mark.parametrize("number", [1, 2, 6])
def test_full_key_cases_with_the_flag_from_the_host(eng, monkeypatch, number):
    """a byte budget below one bitmap per (full key, batch): the (rank, value) pairs go to the host, which applies
    the rule; one result key per pass as well"""
    monkeypatch.setenv("RBG_BSI_BUILD_WS", "1")
    cols, vals, parallelism, size, run = full_case(number)
    r = _check(eng, index_of(cols, vals), parallelism, tag=number)
    assert _kinds(r.ebm) == ((0, 0, 1) if run else (0, 1, 0)), number


_two_full = {}


def _two_full_keys():
    """batchSize 20,000 over 180,000 columns: result key 3 is case 1 (a run container), key 2 holds seven values,
    key 5 becomes full in a batch of exactly 4,096 distinct values (a bitmap) -- the full keys' positions among the
    full keys differ from their result key indexes, and their flags from each other; the index and its reference
    at parallelism 9 (shared, left unchanged)"""
    if not _two_full:
        _, v1, _, _, _ = full_case(1)  # 80,000 columns
        a = np.arange
        low5 = np.concatenate([a(61440), a(61440, 65536), np.full(20000 - 4096, 61440)])
        vals = np.concatenate([v1, (2 << 16) + a(18560) % 7, (5 << 16) + low5])
        assert vals.size == 180000
        o = index_of(a(vals.size), vals)
        _two_full.update(o=o, want=transpose_reference(o, None, 9))
    return _two_full


def test_two_full_keys_next_to_other_keys(eng):
    c = _two_full_keys()
    r = _check(eng, c["o"], 9, want=c["want"])
    assert _kinds(r.ebm) == (1, 1, 1) and O.stats(r.ebm)["card"] == 2 * 65536 + 7


def test_two_full_keys_in_three_passes(eng, monkeypatch):
    """the same with a budget of exactly one result key's bytes: one key per pass, and still above the 2 x 9 x
    8192 bytes of the per-(full key, batch) bitmaps, so the flags are computed on the device and the sweep that
    follows them has to fill every pass again"""
    c = _two_full_keys()
    per_key = 4 * 65536 + 8192 * (1 + (180000).bit_length())
    assert per_key == 417792 and per_key >= 2 * 9 * 8192
    monkeypatch.setenv("RBG_BSI_BUILD_WS", str(per_key))
    r = _check(eng, c["o"], 9, want=c["want"])
    assert _kinds(r.ebm) == (1, 1, 1) and O.stats(r.ebm)["card"] == 2 * 65536 + 7


@pytest.mark.parametrize("parallelism,kinds", [(1, (0, 1, 0)), (2, (0, 0, 1)), (16, (0, 1, 0))])
def test_value_equals_column(eng, parallelism, kinds):
    c = np.arange(65536)
    r = _check(eng, index_of(c, c), parallelism)
    assert _kinds(r.ebm) == kinds and (r.bit_count(), r.min, r.max) == (1, 1, 1)


def test_full_key_with_a_found_set_that_shifts_the_ranks(eng):
    """the batches are cut by the rank in the foundSet, not in ebM & foundSet: 30,000 columns that ebM lacks in
    front move the second batch's start into the index's columns"""
    c = np.arange(65536) + (1 << 16)
    o = index_of(c, c & 0xFFFF)
    found = O.from_values(np.concatenate([np.arange(30000), c]))
    r = _check(eng, o, 1, found)  # batchSize 65,536: batches of 35,536 and 30,000 values
    assert _kinds(r.ebm) == (0, 0, 1)
    r = _check(eng, o, 1, O.from_values(np.concatenate([np.arange(65536), c])))  # the second batch holds them all
    assert _kinds(r.ebm) == (0, 1, 0)


# ---- many keys -----------------------------------------------------------------------------------------------------

def test_600_result_keys_in_one_pass(eng):
    k = np.arange(600, dtype=np.int64) * 100
    vals = np.concatenate([(k << 16) + (k % 7), (k << 16) + 65535 - (k % 5), (k[::3] << 16) + 40000] * 2)
    cols = np.random.default_rng(600).permutation(1 << 20)[:vals.size]
    o = index_of(cols, vals)
    r = _check(eng, o, 4)
    assert len(set((O.to_values(r.ebm) >> 16).tolist())) == 600
    _check(eng, o, 4, O.from_values(np.concatenate([cols[::2], [1 << 30]])))


@pytest.mark.parametrize("n", [1023, 1024, 3000])
def test_route_chosen_by_density(eng, monkeypatch, n):
    """without the switch: four result keys and n columns, one short of 256 columns per result key (the sort
    route), exactly 256 and well above (the count tables); the same bytes on either side"""
    monkeypatch.delenv("RBG_BSI_TR_ROUTE")
    cols = np.arange(n) * 7
    vals = ((cols % 4) << 16) + (cols % 50)
    r = _check(eng, index_of(cols, vals), 2)
    assert len(set((O.to_values(r.ebm) >> 16).tolist())) == 4 and O.stats(r.ebm)["card"] == 4 * 25


# ---- the result as a resident index ---------------------------------------------------------------------------------

def test_result_as_a_resident_index(eng):
    c = _nine()
    o, want = c["o"], c["want"]
    idx = eng.load([o.ebm] + o.ba)
    res, nbits, mn, mx = eng.bsi_transpose(idx, o.bit_count(), 3)
    loaded = eng.load([want.ebm] + want.ba)
    sb, sl = eng.batch_stats(res), eng.batch_stats(loaded)
    assert sb == sl, (sb, sl)
    u, n = transpose_counts(c["cols"], c["vals"], None)
    pc, pv = eng.bsi_to_pairs(res, nbits)
    assert np.asarray(pc).tolist() == u.tolist() and np.asarray(pv).tolist() == n.tolist()
    assert (eng.bsi_get_values(res, nbits, u[:100]) == n[:100]).all()
    for x in (res, loaded):  # one compare of the buffer circuit
        eng.bsi_buffer(x, "GE", nbits, int(np.median(n)), 0, mn, mx)
        got = eng.fetch().serialize()
        assert O.to_values(got).tolist() == u[n >= int(np.median(n))].tolist()
    dbl, n2, mn2, mx2 = eng.bsi_add(res, nbits, res, nbits, mn, mx)  # added to itself: every count doubles
    dc, dv = eng.bsi_to_pairs(dbl, n2)
    assert np.asarray(dc).tolist() == u.tolist() and np.asarray(dv).tolist() == (2 * n).tolist()
    assert (mn2, mx2) == (2 * mn, 2 * mx)
    hit = eng.bsi_in(res, nbits, [int(n.max()), int(n.min())], 2)
    assert O.to_values(eng.batch_fetch(hit).serialize()).tolist() == u[(n == n.max()) | (n == n.min())].tolist()
    assert eng.batch_fetch_range(idx)[0].serialize() == o.ebm  # the operand is untouched
    for x in (idx, res, loaded, dbl, hit):
        eng.release(x)


def test_empty_results(eng):
    o = index_of([5, 70000], [3, 4])
    for found, p in ((_bsi.EMPTY, 1), (O.from_values([6, 1 << 20]), 3), (O.from_values([6, 70001]), 2)):
        r = _check(eng, o, p, found, one_shot=True)  # an empty foundSet, no shared key, shared keys but no column
        assert r.ebm == _bsi.EMPTY and r.bit_count() == 0
    _check(eng, index_of([], []), 2, one_shot=True)
    b = eng.load([o.ebm] + o.ba + [_bsi.EMPTY])
    r, nbits, mn, mx = eng.bsi_transpose(b, o.bit_count(), 1, has_found=True)  # a live batch of one empty bitmap
    assert (nbits, mn, mx) == (0, 0, 0) and eng.batch_stats(r)["bitmaps"] == 1
    assert eng.batch_stats(r)["cardinality"] == 0 and eng.to_values(r).size == 0
    eng.release(r)
    eng.release(b)


def test_refusals_leave_no_batch(eng):
    import roaringbitmap_amd as rb
    o = BSI.from_columns([5, 70000, 6], [9, 2, 9])
    idx = eng.load([o.ebm] + o.ba)
    with_found = eng.load([o.ebm] + o.ba + [o.ebm])
    packed = eng.load([o.ebm] + o.ba, packed=True)
    bitmap_major = eng.synth(3, 0xC4, 1)  # two bitmaps, sorted by (input, key)
    assert eng.batch_stats(bitmap_major)["bitmaps"] == 2
    big = eng.load([o.ebm] + o.ba + [O.bitmap_of_range(0, 1 << 31)])  # one column more than an int cardinality
    probe, nbits, mn, mx = eng.bsi_transpose(idx, 4)
    assert O.to_values(eng.batch_fetch_range(probe, 0, 1)[0].serialize()).tolist() == [2, 9] and (nbits, mn, mx) == (2, 1, 2)
    eng.release(probe)
    for args, kw in (((idx, 4, 0), {}), ((idx, 4, -3), {}),  # parallelism
                     ((idx, 33), {}), ((idx, -1), {}),  # slices
                     ((idx, 3), {}), ((idx, 5), {}), ((idx, 4, 1), {"has_found": True}),  # n_bm
                     ((with_found, 4), {}), ((with_found, 5), {"has_found": True}),
                     ((packed, 4), {}), ((bitmap_major, 1), {})):
        with pytest.raises(rb.IllegalArgumentException):
            eng.bsi_transpose(*args, **kw)
    with pytest.raises(rb.IllegalArgumentException, match="2\\^31 - 1"):
        eng.bsi_transpose(big, 4, 1, has_found=True)
    again = eng.bsi_transpose(with_found, 4, 1, has_found=True)
    assert again[0] == probe  # every refusal freed its slot: the next call takes the released id
    assert again[1:] == (2, 1, 2)
    for x in (idx, with_found, packed, bitmap_major, big, again[0]):
        eng.release(x)
