"""WHERE value IN (...) over a resident bit-sliced index on the MI355X (rbg_ctx_bsi_in, rbg_bsi_in;
BitSliceIndexBase.parallelIn, BBSI/:611-639).  The acceptance throughout: the result batch, fetched, is byte for
byte the reference's sequence composed on the CPU oracle (tests/_bsi_in.py in_reference), through Engine.bsi_in
and through parallelIn's one-shot, and the batch behaves as the loaded batch of those bytes does."""
import os
import re

import numpy as np
import pytest

import _bsi
import _gen
import _oracle as O
from _bsi import BSI
from _bsi_in import in_reference, in_set

pytestmark = pytest.mark.gpu

FULL = np.arange(65536, dtype=np.int64)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the longest value list k_bsi_in searches in LDS
with open(os.path.join(ROOT, "roaringbitmap_amd", "csrc", "kernels.hpp")) as _f:
    CAP = int(re.search(r"kBsiInLdsList = (\d+);", _f.read()).group(1))


@pytest.fixture(scope="module")
def eng(gpu):
    import roaringbitmap_amd as rb
    e = rb.Engine(0)
    yield e
    e.close()


def _kinds(buf):
    s = O.stats(buf)
    return s["array"], s["bitmap"], s["run"]


def _pairs(cols, vals, run_optimize=False):
    return BSI.from_columns(np.asarray(cols, dtype=np.int64), np.asarray(vals, dtype=np.int64), run_optimize)


def _ones(cols, run_optimize=False):
    return _pairs(cols, np.ones(len(cols)), run_optimize)


def _device(eng, o, values, parallelism=1, found=None):
    """the device IN over an oracle index (loaded, the foundSet trailing) -> the result's bytes"""
    b = eng.load([o.ebm] + o.ba + ([found] if found is not None else []))
    r = eng.bsi_in(b, o.bit_count(), values, parallelism, has_found=found is not None)
    got = eng.batch_fetch(r).serialize()
    eng.release(r)
    eng.release(b)
    return got


def _one_shot(o, values, parallelism=1, found=None):
    import roaringbitmap_amd as rb
    x = rb.MutableBitSliceIndex(rb.RoaringBitmap(o.ebm), [rb.RoaringBitmap(s) for s in o.ba], o.min, o.max)
    return x.parallelIn(parallelism, None if found is None else rb.RoaringBitmap(found), values).serialize()


def _check(eng, o, values, parallelism=1, found=None, tag="", want=None, one_shot=False):
    want = in_reference(o, found, values, parallelism) if want is None else want
    got = _device(eng, o, values, parallelism, found)
    assert got == want, (tag, O.stats(got), O.stats(want))
    if one_shot:
        assert _one_shot(o, values, parallelism, found) == want, tag
    return want


def test_known_answer(eng):
    """BufferBSITest.testIN"""
    x = np.arange(1, 100)
    r = _check(eng, _pairs(x, x), range(1, 21), 2, one_shot=True)
    assert O.to_values(r).tolist() == list(range(1, 21))


# ---- the nine-key array / bitmap / run mix of test_gpu_bsi_values.py ---------------------------------------------

def _mix():
    """nine keys, 65535 among them, whose ebM containers are arrays, bitmaps and (run-optimized) runs; the
    values of key 3 are clustered so its slices hold runs too"""
    rng = np.random.default_rng(61)
    keys = np.sort(np.concatenate([rng.choice(65000, 8, replace=False), [65535]]))
    cols = O.to_values(_gen.bitmap(rng, keys, p_present=1.0)).astype(np.int64)
    vals = rng.integers(0, 1 << 18, size=cols.size)
    k3 = (cols >> 16) == keys[3]
    vals[k3] = (cols[k3] & 0xFFFF) // 700
    return keys, cols, vals


_cache = {}


def _nine():
    """the run-optimized oracle index, a foundSet with columns and keys ebM lacks, a value list that a third
    of the columns match, and both references (shared, left unchanged)"""
    if not _cache:
        keys, cols, vals = _mix()
        rng = np.random.default_rng(63)
        o = _pairs(cols, vals, True)
        kinds = [O.stats(b) for b in [o.ebm] + o.ba]
        assert all(sum(k[t] for k in kinds) > 0 for t in ("array", "bitmap", "run")), kinds
        extra = np.concatenate([rng.integers(0, 1 << 32, size=3000),
                                (int(keys[2]) << 16) + rng.integers(0, 65536, 500)])
        found_cols = np.unique(np.concatenate([cols[::5], cols[(cols >> 16) == keys[7]], extra]))
        found = O.run_optimize(O.from_values(found_cols))
        values = np.concatenate([rng.choice(vals, vals.size // 3), np.arange(0, 94, 2), [-5, 1 << 18, 1 << 30]])
        values = rng.permutation(values)
        _cache.update(o=o, cols=cols, vals=vals, found=found, found_cols=found_cols, values=values,
                      want=in_reference(o, None, values, 3), want_found=in_reference(o, found, values, 3))
        s = in_set(cols, vals, None, values)
        assert O.to_values(_cache["want"]).tolist() == s.tolist() and cols.size // 20 < s.size < cols.size
        assert O.to_values(_cache["want_found"]).tolist() == in_set(cols, vals, found_cols, values).tolist()
    return _cache


def test_nine_keys_loaded(eng):
    c = _nine()
    _check(eng, c["o"], c["values"], 3, want=c["want"], one_shot=True)


def test_nine_keys_built_on_the_device(eng):
    c = _nine()
    b, nbits, _, _ = eng.bsi_from_columns(c["cols"], c["vals"], True)
    r = eng.bsi_in(b, nbits, c["values"], 3)
    assert eng.batch_fetch(r).serialize() == c["want"]
    eng.release(r)
    eng.release(b)


def test_nine_keys_with_a_trailing_found_set(eng):
    c = _nine()
    _check(eng, c["o"], c["values"], 3, c["found"], want=c["want_found"], one_shot=True)


@pytest.mark.parametrize("budget", ["one_key", "two_keys", "1"])
def test_forced_passes(eng, monkeypatch, budget):
    """the workspace budget forced down through the environment switch: whole keys per pass, the same bytes"""
    c = _nine()
    nbytes = {"one_key": 8192, "two_keys": 2 * 8192 + 100, "1": 1}[budget]
    monkeypatch.setenv("RBG_BSI_BUILD_WS", str(nbytes))
    _check(eng, c["o"], c["values"], 3, want=c["want"])
    _check(eng, c["o"], c["values"], 3, c["found"], want=c["want_found"])
    monkeypatch.delenv("RBG_BSI_BUILD_WS")
    _check(eng, c["o"], c["values"], 3, want=c["want"])


# ---- keys, slices, thresholds ---------------------------------------------------------------------------------

def test_keys_of_one_side_alone(eng):
    """keys 0 and 9 in ebM alone, 4 and 65535 in the foundSet alone, 7 in both (the foundSet's part of it
    reaching outside ebM's)"""
    cols = np.concatenate([np.arange(0, 200, 2), (7 << 16) + np.arange(0, 9000, 3), (9 << 16) + np.arange(50)])
    o = _pairs(cols, cols % 5)
    found = O.from_values(np.concatenate([(4 << 16) + np.arange(30), (7 << 16) + np.arange(100, 6000),
                                          (65535 << 16) + np.array([0, 65535])]))
    r = _check(eng, o, [0, 3], 2, found, one_shot=True)
    v = O.to_values(r)
    assert v.size and (v >> 16 == 7).all()
    r = _check(eng, o, [0, 3], 2)
    assert sorted(set((O.to_values(r) >> 16).tolist())) == [0, 7, 9]


def test_slice_without_a_container_and_zero_values(eng):
    """key 4 holds even values alone (slice 0 has no container there), key 6 the value 0 alone (no slice has
    one), key 8 odd values"""
    c4, c6, c8 = (4 << 16) + np.arange(3000), (6 << 16) + np.arange(0, 500, 7), (8 << 16) + np.arange(100)
    o = _pairs(np.concatenate([c4, c6, c8]), np.concatenate([2 * (c4 % 13), 0 * c6, 2 * (c8 % 4) + 1]))
    assert O.to_values(o.ba[0]).tolist() == c8.tolist()
    r = _check(eng, o, [0], one_shot=True)
    assert O.to_values(r).tolist() == np.concatenate([c4[c4 % 13 == 0], c6]).tolist()
    _check(eng, o, [0, 4, 7, 24, 25])
    z = _pairs([9, 70000], [0, 0])  # one (empty) slice
    assert O.to_values(_check(eng, z, [0])).tolist() == [9, 70000] and _check(eng, z, [1]) == _bsi.EMPTY


def test_array_slices_small_words_and_skipped_words(eng):
    """key 5 in array slices: words of exactly 4 and 5 columns side by side (a word of up to four columns takes
    the four-register form), a foundSet that keeps every third word alone (a thread's position in a slice's
    array has to pass the values under the words it skipped), and slices that hold columns ebM lacks"""
    rng = np.random.default_rng(55)
    lows = np.unique(np.concatenate([np.arange(0, 65536, 23), 3200 + np.arange(4), 3232 + np.arange(5),
                                     3264 + np.arange(0, 32, 2), 65504 + np.arange(32)]))
    cols = np.concatenate([(5 << 16) + lows, (6 << 16) + np.arange(0, 65536, 3)])
    vals = rng.integers(0, 64, cols.size)
    o = _pairs(cols, vals)
    assert all(_kinds(b)[0] >= 1 for b in o.ba)
    values = [0, 3, 17, 40, 41, 63, 64]
    r = _check(eng, o, values, 2, one_shot=True)
    assert O.to_values(r).tolist() == in_set(cols, vals, None, values).tolist()
    found = O.from_values(cols[((cols & 0xFFFF) >> 5) % 3 == 0])
    _check(eng, o, values, 2, found)
    stray = O.from_values((5 << 16) + np.setdiff1d(np.arange(1, 65536, 46), lows))
    loose = BSI(o.ebm, [O.pairwise("or", b, stray) for b in o.ba], o.min, o.max)
    assert _kinds(loose.ba[0])[0] >= 1 and _check(eng, loose, values, 2) == r
    _check(eng, loose, values, 2, found)


@pytest.mark.parametrize("n,kind", [(4096, (1, 0, 0)), (4097, (0, 1, 0))])
def test_cardinality_threshold_and_an_empty_key(eng, n, kind):
    """key 9: exactly n of 20,000 columns match, drawn from three batches; key 11: no column matches while its
    neighbours fill; key 12: two match"""
    p = np.random.default_rng(n).permutation(65536)[:20000]
    c9, c11, c12 = (9 << 16) + p, (11 << 16) + np.arange(300), (12 << 16) + np.arange(40)
    v9 = np.where(np.arange(20000) < n, 77, 5)
    o = _pairs(np.concatenate([c9, c11, c12]),
               np.concatenate([v9, np.full(300, 6), np.where(np.arange(40) < 2, 77, 9)]))
    r = _check(eng, o, [77], 3)
    assert _kinds(r) == (kind[0] + 1, kind[1], 0) and O.stats(r)["card"] == n + 2


# ---- full containers: a bitmap inside one batch, a run container across two ----------------------------------------

@pytest.mark.parametrize("run_optimize", [False, True])
@pytest.mark.parametrize("name,cols,found,parallelism,kinds", [
    ("aligned", np.concatenate([(1 << 16) + FULL, (2 << 16) + FULL]), None, 1, (0, 2, 0)),
    ("one_earlier_column", np.concatenate([[5], (1 << 16) + FULL, (2 << 16) + FULL]), None, 1, (1, 0, 2)),
    ("parallelism_2", (1 << 16) + FULL, None, 2, (0, 0, 1)),
    ("found_shifts_the_ranks", (1 << 16) + FULL, np.concatenate([[3, 9], (1 << 16) + FULL]), 1, (0, 0, 1)),
    ("found_pads_to_alignment", (1 << 16) + FULL, np.concatenate([FULL, (1 << 16) + FULL]), 1, (0, 1, 0)),
    ("parallelism_above_cardinality", (1 << 16) + FULL, None, 100000, (0, 1, 0)),  # batchSize = min(100000, 65536)
    ("parallelism_above_a_small_cardinality", np.arange(50), None, 1000, (1, 0, 0)),
])
def test_full_keys(eng, run_optimize, name, cols, found, parallelism, kinds):
    o = _ones(cols, run_optimize)
    assert (_kinds(o.ebm)[2] > 0) == run_optimize  # run-optimized: the inputs are run containers
    f = None if found is None else O.from_values(found, run_optimize)
    r = _check(eng, o, [1], parallelism, f, name, one_shot=not run_optimize)
    assert _kinds(r) == kinds, name


def test_found_set_of_two_to_the_31_columns(eng):
    """the largest foundSet the reference's int cardinality takes, [0, 2^31 - 1): batchSize 65,536 with key 1
    aligned; one column more is refused"""
    import roaringbitmap_amd as rb
    o = _ones(np.concatenate([(1 << 16) + FULL, [(40000 << 16) + 7]]))
    found = O.bitmap_of_range(0, (1 << 31) - 1)
    b = eng.load([o.ebm] + o.ba + [found])
    r = eng.bsi_in(b, 1, [1], 1, has_found=True)
    got = eng.batch_fetch(r).serialize()
    assert got == O.from_values((1 << 16) + FULL) and _kinds(got) == (0, 1, 0)
    eng.release(r)
    eng.release(b)
    b = eng.load([o.ebm] + o.ba + [O.bitmap_of_range(0, 1 << 31)])
    with pytest.raises(rb.IllegalArgumentException, match="2\\^31 - 1"):
        eng.bsi_in(b, 1, [1], 1, has_found=True)
    eng.release(b)


# ---- value lists -------------------------------------------------------------------------------------------------

def _spread():
    """40,000 columns over three keys with 18-bit values (shared)"""
    if "spread" not in _cache:
        rng = np.random.default_rng(71)
        cols = np.concatenate([(k << 16) + rng.choice(65536, n, replace=False)
                               for k, n in ((2, 30000), (3, 9000), (700, 1000))])
        vals = rng.integers(0, 1 << 18, size=cols.size)
        _cache["spread"] = (_pairs(cols, vals), cols, vals)
    return _cache["spread"]


@pytest.mark.parametrize("name", ["unsorted_with_repeats", "no_match", "single", "empty", "100000", "cap", "cap_plus_1",
                                  "cap_plus_1_none_listed_last"])
def test_value_lists(eng, name):
    o, cols, vals = _spread()
    rng = np.random.default_rng(72)
    distinct = np.unique(vals)
    values = {
        "unsorted_with_repeats": lambda: np.concatenate([vals[:50][::-1], vals[:50], vals[20:30]]),
        "no_match": lambda: [-1, -(1 << 31), 1 << 18, (1 << 31) - 1, -77],  # negative, >= 2^nbits
        "single": lambda: [int(vals[7])],
        "empty": lambda: [],
        "100000": lambda: rng.choice(1 << 18, 100000, replace=False),
        "cap": lambda: rng.permutation(distinct)[:CAP],
        "cap_plus_1": lambda: rng.permutation(distinct)[:CAP + 1],
        # the largest entry is the only one past the LDS list's reach were the cap off by one
        "cap_plus_1_none_listed_last": lambda: np.concatenate([np.sort(distinct)[:CAP], [int(distinct.max())]]),
    }[name]()
    r = _check(eng, o, values, 2, tag=name, one_shot=name in ("empty", "100000", "cap"))
    assert O.to_values(r).tolist() == in_set(cols, vals, None, values).tolist()
    if name in ("no_match", "empty"):
        assert r == _bsi.EMPTY
    if name.startswith("cap"):
        assert np.unique(np.asarray(values)).size == (CAP if name == "cap" else CAP + 1)
        assert O.stats(r)["card"] > CAP // 2


def test_thirty_two_slices_match_a_negative_value(eng):
    """hand-made slices: bit 31 makes getValue's int negative, and a negative list entry matches it"""
    cols = np.array([5, 70000, 70001, 70002], dtype=np.int64)
    vals = np.array([0x80000001, 3, 0xFFFFFFFF, 0x7FFFFFFF], dtype=np.int64)
    o = BSI(O.from_values(cols), [O.from_values(cols[(vals >> i) & 1 == 1]) for i in range(32)], 0, 0)
    r = _check(eng, o, [-(1 << 31) + 1, -1, 4], one_shot=True)
    assert O.to_values(r).tolist() == [5, 70001]
    assert O.to_values(_check(eng, o, [0x7FFFFFFF, 3, 1])).tolist() == [70000, 70002]
    short = BSI(o.ebm, o.ba[:31], 0, 0)  # 31 slices: no value is negative
    assert O.to_values(_check(eng, short, [-1, -(1 << 31) + 1, 1, 0x7FFFFFFF])).tolist() == [5, 70001, 70002]


def test_600_keys_in_one_pass(eng):
    k = np.arange(600, dtype=np.int64) * 100
    cols = np.concatenate([(k << 16) + (k % 7), (k << 16) + 65535 - (k % 5), (k[::3] << 16) + 40000])
    vals = np.random.default_rng(600).integers(0, 8, cols.size)
    found = O.from_values(np.concatenate([cols[::2], (k[5::7] << 16) + 123]))
    o = _pairs(cols, vals)
    r = _check(eng, o, [1, 6, 7], 4)
    assert len(set((O.to_values(r) >> 16).tolist())) > 400
    _check(eng, o, [1, 6, 7], 4, found)


# ---- the result as a resident bitmap ---------------------------------------------------------------------------------

def test_result_as_a_loaded_bitmap(eng):
    c = _nine()
    o, want = c["o"], c["want"]
    idx = eng.load([o.ebm] + o.ba)
    built = eng.bsi_in(idx, o.bit_count(), c["values"], 3)
    loaded = eng.load([want])
    sb, sl = eng.batch_stats(built), eng.batch_stats(loaded)
    assert len(sb) == 8 and sb == sl, (sb, sl)
    assert (eng.batch_counts(built) == eng.batch_counts(loaded)).all()
    other = eng.load([c["found"]])
    for op in ("and", "or", "xor", "andnot"):
        res = []
        for x in (built, loaded):
            eng.pairwise(op, x, other)
            res.append(eng.fetch().serialize())
            eng.pairwise(op, other, x)
            res.append(eng.fetch().serialize())
        assert res[0] == res[2] == O.pairwise(op, want, c["found"]) and res[1] == res[3], op
    assert (eng.to_values(built) == O.to_values(want)).all()
    assert (eng.to_values(built, first=1000, count=5000) == O.to_values(want)[1000:6000]).all()
    # as the trailing foundSet of a second query
    again = eng.load([o.ebm] + o.ba + [eng.batch_fetch(built).serialize()])
    second = eng.bsi_in(again, o.bit_count(), c["values"][::2], 1, has_found=True)
    assert eng.batch_fetch(second).serialize() == in_reference(o, want, c["values"][::2], 1)
    assert eng.batch_fetch_range(idx)[0].serialize() == o.ebm  # the operand is untouched
    for x in (idx, built, loaded, other, again, second):
        eng.release(x)


def test_empty_found_set_empty_index_and_disjoint_keys(eng):
    o, _, vals = _spread()
    v = [int(vals[0])]
    assert _check(eng, o, v, 1, _bsi.EMPTY, one_shot=True) == _bsi.EMPTY
    assert _check(eng, o, v, 5, O.from_values([1, (5 << 16) + 2])) == _bsi.EMPTY  # no shared key
    assert _check(eng, _pairs([], []), [0], 2, one_shot=True) == _bsi.EMPTY
    b = eng.load([o.ebm] + o.ba)
    r = eng.bsi_in(b, o.bit_count(), [])  # a live batch of one empty bitmap
    assert eng.batch_stats(r)["bitmaps"] == 1 and eng.batch_stats(r)["cardinality"] == 0
    assert eng.to_values(r).size == 0
    eng.release(r)
    eng.release(b)


def test_refusals_leave_no_batch(eng):
    import roaringbitmap_amd as rb
    o = _pairs([5, 70000, 6], [9, 2, 4])
    idx = eng.load([o.ebm] + o.ba)
    with_found = eng.load([o.ebm] + o.ba + [o.ebm])
    packed = eng.load([o.ebm] + o.ba, packed=True)
    bitmap_major = eng.synth(3, 0xC4, 1)  # two bitmaps, sorted by (input, key)
    assert eng.batch_stats(bitmap_major)["bitmaps"] == 2
    probe = eng.bsi_in(idx, 4, [9])
    assert eng.batch_fetch(probe).serialize() == O.from_values([5])
    eng.release(probe)
    for args, kw in (((idx, 4, [9], 0), {}), ((idx, 4, [9], -3), {}),  # parallelism
                     ((idx, 33, [9]), {}), ((idx, -1, [9]), {}),  # slices
                     ((idx, 3, [9]), {}), ((idx, 5, [9]), {}), ((idx, 4, [9], 1), {"has_found": True}),  # n_bm
                     ((with_found, 4, [9]), {}), ((with_found, 5, [9]), {"has_found": True}),
                     ((packed, 4, [9]), {}), ((bitmap_major, 1, [9]), {})):
        with pytest.raises(rb.IllegalArgumentException):
            eng.bsi_in(*args, **kw)
    with pytest.raises(rb.IllegalArgumentException, match="32 bits"):
        eng.bsi_in(idx, 4, [1 << 32])
    again = eng.bsi_in(with_found, 4, [9, 2], 1, has_found=True)
    assert again == probe  # every refusal freed its slot: the next query takes the released id
    assert eng.batch_fetch(again).serialize() == O.from_values([5, 70000])
    for x in (idx, with_found, packed, bitmap_major, again):
        eng.release(x)
