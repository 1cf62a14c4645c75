"""The two forms of the setValues oracle (tests/_bsi_set.py) against each other: the dict replay typed by
cardinality and the pairwise composition or(andnot(slice, B), S_i) must give the same bytes and the same
{nbits, min, max}.  CPU only."""
import numpy as np
import pytest

import _oracle as O
from _bsi import BSI
from _bsi_set import capacity, replay_values, set_composed, set_reference


def _index(cols, vals):
    return BSI.from_columns(np.asarray(cols, dtype=np.int64), np.asarray(vals, dtype=np.int64))


def _kinds(buf):
    s = O.stats(buf)
    return s["array"], s["bitmap"], s["run"]


def _agree(a, cols, vals, tag=""):
    r, c = set_reference(a, cols, vals), set_composed(a, cols, vals)
    assert (r.bit_count(), r.min, r.max) == (c.bit_count(), c.min, c.max), tag
    assert [r.ebm] + r.ba == [c.ebm] + c.ba, tag
    return r


def test_depth_rule_branches():
    assert capacity(True, 0, 0, 0, 5, 9) == (4, 5, 9)  # empty ebM: both fields, grow
    assert capacity(True, 6, 7, 7, 0, 0) == (6, 0, 0)  # empty ebM below the caller's depth; bitlen(0) = 1
    assert capacity(False, 4, 3, 9, 1, 5) == (4, 1, 9)  # min alone
    assert capacity(False, 4, 3, 9, 1, 100) == (4, 1, 9)  # both exceeded: the else-if leaves max and the depth
    assert capacity(False, 4, 3, 9, 3, 100) == (7, 3, 100)  # max: grow
    assert capacity(False, 4, 3, 9, 3, 9) == (4, 3, 9)  # neither
    assert capacity(False, 9, 3, 9, 3, 100) == (9, 3, 100)  # a caller's depth above bitlen(max) stays


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_forms_agree_on_random_batches(seed):
    rng = np.random.default_rng(seed)
    keys = np.array([0, 3, 4, 900, 65535])
    cols = np.concatenate([(k << 16) + rng.choice(65536, s, replace=False)
                           for k, s in zip(keys, rng.permutation([5000, 4097, 4096, 30, 60000]))])
    a = _index(cols, rng.integers(0, 1 << 11, cols.size))
    upd = rng.choice(cols, 3000, replace=False)
    ins = np.concatenate([(rng.choice([1, 4, 70, 65534], 800) << 16) + rng.integers(0, 65536, 800), upd[:300]])
    bc = rng.permutation(np.concatenate([upd, ins, upd[:500]]))  # columns given twice and three times
    for hi, tag in ((1 << 11, "neither or min"), (1 << 14, "grow")):
        bv = rng.integers(0, hi, bc.size)
        r = _agree(a, bc, bv, (seed, tag))
        c0, v0 = replay_values(cols, _values(a, cols), bc, bv, r.bit_count())
        assert O.to_values(r.ebm).tolist() == c0.tolist()
        assert _values(r, c0).tolist() == v0.tolist()


def _values(x, cols):
    v = np.zeros(len(cols), dtype=np.int64)
    for i, s in enumerate(x.ba):
        v |= np.isin(cols, O.to_values(s)).astype(np.int64) << i
    return v


def test_type_boundaries_in_both_directions():
    low = np.random.default_rng(7).permutation(65536)
    base = (9 << 16) + low
    a = _index(base[:4096], np.ones(4096))
    r = _agree(a, base[4096:4097], [1])  # 4096 -> 4097 by insert: slice 0 and ebM turn into bitmaps
    assert _kinds(r.ba[0]) == (0, 1, 0) and _kinds(r.ebm) == (0, 1, 0)
    r2 = _agree(r, base[:1], [0])  # 4097 -> 4096 by an overwrite that clears: an array again; ebM stays
    assert _kinds(r2.ba[0]) == (1, 0, 0) and _kinds(r2.ebm) == (0, 1, 0) and O.stats(r2.ba[0])["card"] == 4096
    r3 = _agree(a, base[:4096], np.zeros(4096))  # the slice's only container emptied: gone, the slice stays
    assert r3.ba == [O.from_values([])] and r3.bit_count() == 1


def test_full_key_is_a_bitmap_container():
    a = _index((2 << 16) + np.arange(65535), np.full(65535, 3))
    r = _agree(a, [(2 << 16) + 65535], [3])
    assert [_kinds(x) for x in [r.ebm] + r.ba] == [(0, 1, 0)] * 3 and O.stats(r.ebm)["card"] == 65536


def test_the_four_depth_branches_and_repeats():
    a = _index([5, 6, 70000], [3, 9, 4])
    e = _index([], [])
    r = _agree(e, [1, 1, 2, 1], [9, 3, 200, 7])  # empty: min / max of the batch (an overwritten 9 counts)
    assert (r.bit_count(), r.min, r.max) == (8, 3, 200) and _values(r, np.array([1, 2])).tolist() == [7, 200]
    r = _agree(a, [5, 7], [1, 2])  # min alone
    assert (r.bit_count(), r.min, r.max) == (4, 1, 9)
    r = _agree(a, [5, 7], [1, 0x1F5])  # both exceeded: the high bits of 0x1F5 are dropped, max stays
    assert (r.bit_count(), r.min, r.max) == (4, 1, 9) and _values(r, np.array([5, 7])).tolist() == [1, 5]
    r = _agree(a, [6, 8, 6], [3, 0x1F5, 4])  # grow by several slices; column 6 ends at 4, max stays stale
    assert (r.bit_count(), r.min, r.max) == (9, 3, 0x1F5) and _values(r, np.array([6, 8])).tolist() == [4, 0x1F5]
    r = _agree(a, [6], [5])  # neither: the overwritten maximum stays in the field
    assert (r.bit_count(), r.min, r.max) == (4, 3, 9)
    r = _agree(a, [5], [0])  # 3 overwritten by 0: bits cleared, the column stays in ebM
    assert _values(r, np.array([5])).tolist() == [0] and O.to_values(r.ebm).tolist() == [5, 6, 70000]


def test_full_run_ebm_keeps_its_run_containers():
    cols = np.concatenate([np.arange(65536), (5 << 16) + np.arange(100)])
    a = BSI.from_columns(cols, cols & 1023)
    a.ebm = O.run_optimize(a.ebm)
    assert _kinds(a.ebm)[2] >= 1 and not any(_kinds(s)[2] for s in a.ba)
    r = set_reference(a, [7, 9], [1, 2])
    assert r.ebm == a.ebm
    r = set_reference(a, [7, (9 << 16) + 1], [1, 2])
    assert O.to_values(r.ebm).tolist() == sorted(cols.tolist() + [(9 << 16) + 1])
    assert O.stats(r.ebm)["run"] == O.stats(a.ebm)["run"]
