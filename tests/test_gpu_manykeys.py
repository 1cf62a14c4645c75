"""Many-key sparse parity of the per-key kernels outside the pairwise family, byte for byte against the oracle.

The small-shape files of these families (test_gpu_addoffset / rangemut / range / inplace / buffer_pairwise /
contains / ornot) cover every container type on 3 to 60 containers.  At that size three things never happen:
a result record lands past the first 64-record tile, plan_emit (wave.hpp) adds up the task counts of other
256-key plan workgroups (an empty one among them), and a wave takes a second task (k_rmut's stride loop with
its prefetched record, k_aoff's chunk with the Q container carried in registers as the next task's P), which
needs more tasks than the 8,192 waves an MI355X holds.  The inputs here are _gen.sparse_keys /
sparse_bitmap: 9,300 to 9,700 keys with gaps, tiny containers, a heavy container on every 97th key.
tests/test_manykeys_host.py pins those inputs and checks the oracle's results against plain numpy set
arithmetic; one assertion per family here checks the GPU's result against the same numpy restatement.
"""
import hashlib

import numpy as np
import pytest

import _oracle as O
from _fmt import container_table
from test_manykeys_host import (OFFSETS, SEEDS, inputs, np_add_offset, np_pair, np_range_mut, np_range_op,
                                np_select, ornot_agrees, ornot_mask, vals)

pytestmark = pytest.mark.gpu

RANGES = ("absent", "mid_to_end", "all", "hole")


def _rb():
    import roaringbitmap_amd as rb
    return rb


def _same(got: bytes, exp: bytes, what):
    """bytes equality with a short message (a pytest diff of two 1 MB strings takes minutes)"""
    if got == exp:
        return
    n = min(len(got), len(exp))
    first = next((i for i in range(n) if got[i] != exp[i]), n)
    raise AssertionError(f"{what}: {len(got)} B (sha {hashlib.sha1(got).hexdigest()[:12]}) vs oracle {len(exp)} B "
                         f"(sha {hashlib.sha1(exp).hexdigest()[:12]}), first difference at byte {first}")


def _same_set(got: bytes, want, what):
    assert np.array_equal(vals(got), want), f"{what}: not the numpy set"


@pytest.fixture(scope="module", params=SEEDS, ids=[f"seed{x:x}" for x in SEEDS])
def s(request, gpu):
    return inputs(request.param)


# ---- addOffset --------------------------------------------------------------------------------------
def test_add_offset(s):
    """P-only, Q-only and two-part tasks, chunks of three tasks per wave across key gaps (the carried Q
    taken only when the previous task's key is this one's minus one and it had a Q container)"""
    rb = _rb()
    x, m = rb.RoaringBitmap(s.x), rb.ImmutableRoaringBitmap(s.x)
    for off in OFFSETS:
        want = O.add_offset(s.x, off)
        got = rb.RoaringBitmap.addOffset(x, off)
        assert type(got) is rb.RoaringBitmap
        _same(got.serialize(), want, f"addOffset {off}")
        gm = rb.MutableRoaringBitmap.addOffset(m, off)
        assert isinstance(gm, rb.MutableRoaringBitmap)
        _same(gm.serialize(), want, f"buffer addOffset {off}")
        if off in (300, -300, (1 << 32) - 1):
            _same_set(got.serialize(), np_add_offset(s.vx, off), f"addOffset {off}")
    assert x.serialize() == s.x


def test_add_offset_resident(s):
    """Engine.add_offset on a device-resident batch, one op after the other on the same context"""
    rb = _rb()
    eng = rb.Engine()
    (ia,) = eng.load_pair(s.x)
    for off in OFFSETS:
        eng.add_offset(ia, off)
        _same(eng.fetch().serialize(), O.add_offset(s.x, off), f"resident addOffset {off}")
    eng.close()


# ---- range mutations ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", RANGES)
def test_range_mutations(s, name):
    """static add / remove / flip (heap and buffer: RMUT_REMOVE with BUF) and the in-place forms
    (RMUT_ADD_INPLACE over thousands of keys between the first and the last) with their cardinalities"""
    rb = _rb()
    st, en = s.ranges[name]
    x, m = rb.RoaringBitmap(s.x), rb.MutableRoaringBitmap(s.x)
    for op in ("add", "remove", "flip"):
        got = getattr(rb.RoaringBitmap, op)(x, st, en).serialize()
        _same(got, O.range_mut(op, s.x, st, en), f"{op} {name}")
        gotb = getattr(rb.MutableRoaringBitmap, op)(m, st, en)
        assert isinstance(gotb, rb.MutableRoaringBitmap)
        _same(gotb.serialize(), O.range_mut(op, s.x, st, en, buffer=True), f"buffer {op} {name}")
        if name == "absent" or op == "remove":
            _same_set(got, np_range_mut(op, s.vx, st, en), f"{op} {name}")
    assert x.serialize() == s.x and m.serialize() == s.x
    for cls, buffer in ((rb.RoaringBitmap, False), (rb.MutableRoaringBitmap, True)):
        for op in ("add", "remove", "flip"):
            y = cls(s.x)
            assert getattr(y, op)(st, en) is None
            want = O.range_mut("add_inplace" if op == "add" else op, s.x, st, en, buffer=buffer)
            _same(y.serialize(), want, f"in-place {cls.__name__}.{op} {name}")
            assert y.getLongCardinality() == int(container_table(want)[2].sum()), (cls.__name__, op, name)


# ---- removeRunCompression, limit, selectRange --------------------------------------------------------
def test_remove_run_compression(s):
    """RMUT_DERUN converting more than 3,000 one- and two-run containers between cloned ones"""
    rb = _rb()
    want = O.remove_run_compression(s.xr)
    for cls in (rb.RoaringBitmap, rb.MutableRoaringBitmap):
        x = cls(s.xr)
        assert x.removeRunCompression() is True
        _same(x.serialize(), want, f"{cls.__name__}.removeRunCompression")
        assert x.container_stats()[2] == 0
    _same_set(x.serialize(), vals(s.xr), "removeRunCompression")


def test_limit(s):
    """RMUT_LIMIT: the plan's limit rule past key 255, the cut in the first container, in a heavy one
    past task 8,192 and in the last one, and no cut at all"""
    rb = _rb()
    x, m = rb.RoaringBitmap(s.x), rb.ImmutableRoaringBitmap(s.x)
    for name, n in s.limits.items():
        want = O.limit(s.x, n)
        got = x.limit(n)
        assert type(got) is rb.RoaringBitmap
        _same(got.serialize(), want, f"limit {name} {n}")
        gm = m.limit(n)
        assert isinstance(gm, rb.MutableRoaringBitmap)
        _same(gm.serialize(), want, f"buffer limit {name} {n}")
        _same_set(got.serialize(), s.vx[:n], f"limit {name} {n}")


def test_select_range(s):
    rb = _rb()
    x, m = rb.RoaringBitmap(s.x), rb.ImmutableRoaringBitmap(s.x)
    for name in RANGES:
        st, en = s.ranges[name]
        got = x.selectRange(st, en)
        assert type(got) is rb.RoaringBitmap
        _same(got.serialize(), O.range_op("select", [s.x], st, en), f"selectRange {name}")
        gm = m.selectRange(st, en)
        assert isinstance(gm, rb.MutableRoaringBitmap)
        _same(gm.serialize(), O.range_op("select_buf", [s.x], st, en), f"buffer selectRange {name}")
        _same_set(got.serialize(), np_select(s.vx, st, en), f"selectRange {name}")


# ---- range-restricted aggregations -------------------------------------------------------------------
@pytest.mark.parametrize("name", RANGES)
def test_range_aggregations(s, name):
    """and / or / xor(Iterator, start, end) and andNot(x1, x2, start, end), heap and buffer, over three
    sparse bitmaps that share most keys and a third of their containers"""
    rb = _rb()
    st, en = s.ranges[name]
    bufs = [s.x, s.y, s.z]
    vs = [s.vx, vals(s.y), vals(s.z)]
    for cls, suffix in ((rb.RoaringBitmap, ""), (rb.ImmutableRoaringBitmap, "_buf")):
        bms = [cls(b) for b in bufs]
        for op in ("and", "or", "xor", "andnot"):
            if op == "andnot":
                got = cls.andNot(bms[0], bms[1], st, en)
                want = O.range_op("andnot" + suffix, bufs[:2], st, en)
            else:
                got = getattr(cls, op)(iter(bms), st, en)
                want = O.range_op(op + suffix, bufs, st, en)
            assert isinstance(got, rb.MutableRoaringBitmap if suffix else rb.RoaringBitmap)
            _same(got.serialize(), want, f"{cls.__name__}.{op} {name}")
            if not suffix:
                _same_set(got.serialize(), np_range_op(op, vs, st, en), f"{op} {name}")


# ---- in-place and buffer pairwise --------------------------------------------------------------------
def test_in_place_pairwise(s):
    """x1.and / or / xor / andNot(x2) in place: thousands of records through the in-place fix-up"""
    rb = _rb()
    vy = vals(s.y)
    for op, oop in (("and", "and"), ("or", "ior"), ("xor", "xor"), ("andNot", "andnot")):
        for a, b, va, vb, tag in ((s.x, s.y, s.vx, vy, "x.y"), (s.y, s.x, vy, s.vx, "y.x")):
            x1 = rb.RoaringBitmap(a)
            getattr(x1, op)(rb.RoaringBitmap(b))
            _same(x1.serialize(), O.pairwise(oop, a, b), f"in-place {op} {tag}")
            want = np_pair(oop.replace("ior", "or"), va, vb)
            _same_set(x1.serialize(), want, f"in-place {op} {tag}")
            assert x1.getLongCardinality() == want.size


def test_buffer_pairwise(s):
    """the buffer package's static and / andNot and MutableRoaringBitmap's in-place forms"""
    rb = _rb()
    I, M = rb.ImmutableRoaringBitmap, rb.MutableRoaringBitmap
    vy = vals(s.y)
    for a, b, va, vb, tag in ((s.x, s.y, s.vx, vy, "x.y"), (s.y, s.x, vy, s.vx, "y.x")):
        for op, oop, f in (("and", "and_buf", getattr(I, "and")), ("andnot", "andnot_buf", I.andNot)):
            want, want_set = O.pairwise(oop, a, b), np_pair(op, va, vb)
            got = f(I(a), I(b))
            assert isinstance(got, M)
            _same(got.serialize(), want, f"buffer static {op} {tag}")
            _same_set(got.serialize(), want_set, f"buffer static {op} {tag}")
            y = M(a)
            getattr(y, "and" if op == "and" else "andNot")(I(b))
            _same(y.serialize(), want, f"buffer in-place {op} {tag}")
            assert y.getLongCardinality() == want_set.size


# ---- contains(subset), isHammingSimilar --------------------------------------------------------------
def test_contains_and_hamming(s):
    """a subset that lacks values under late keys only, and a bitmap with exactly one value more under key
    65535 (the last record of the last tile decides)"""
    rb = _rb()
    for cls in (rb.RoaringBitmap, rb.ImmutableRoaringBitmap):
        x, sub, non = cls(s.x), cls(s.sub), cls(s.non)
        assert x.contains(sub) and x.contains(x) and non.contains(x) and non.contains(sub)
        assert not sub.contains(x) and not x.contains(non) and not sub.contains(non)
    x, sub, non = rb.RoaringBitmap(s.x), rb.RoaringBitmap(s.sub), rb.RoaringBitmap(s.non)
    d = s.sub_dist
    assert np.setxor1d(s.vx, vals(s.sub)).size == d
    assert x.isHammingSimilar(sub, d) and sub.isHammingSimilar(x, d)
    assert not x.isHammingSimilar(sub, d - 1) and not sub.isHammingSimilar(x, d - 1)
    assert x.isHammingSimilar(non, 1) and not x.isHammingSimilar(non, 0)
    assert non.isHammingSimilar(sub, d + 1) and not non.isHammingSimilar(sub, d)


# ---- orNot --------------------------------------------------------------------------------------------
def test_ornot_end_in_empty_workgroup(s):
    """rangeEnd under a key of the plan workgroup that holds no key of either operand, all four forms"""
    rb = _rb()
    end = s.ornot_end
    x1, x2 = rb.RoaringBitmap(s.x), rb.RoaringBitmap(s.y)
    got = rb.RoaringBitmap.orNot(x1, x2, end).serialize()
    _same(got, O.ornot(s.x, s.y, end), "static orNot")
    assert ornot_agrees(O.to_values(got), s.vx, ornot_mask(s.vx, vals(s.y), end), end), "static orNot: not the set"
    assert x1.serialize() == s.x
    y = rb.RoaringBitmap(s.x)
    y.orNot(x2, end)
    _same(y.serialize(), O.ornot(s.x, s.y, end, inplace=True), "in-place orNot")
    gotb = rb.ImmutableRoaringBitmap.orNot(rb.ImmutableRoaringBitmap(s.x), rb.ImmutableRoaringBitmap(s.y), end)
    assert isinstance(gotb, rb.MutableRoaringBitmap)
    _same(gotb.serialize(), O.ornot(s.x, s.y, end, buffer=True), "buffer static orNot")
    m = rb.MutableRoaringBitmap(s.x)
    m.orNot(rb.ImmutableRoaringBitmap(s.y), end)
    _same(m.serialize(), O.ornot(s.x, s.y, end, inplace=True, buffer=True), "buffer in-place orNot")
