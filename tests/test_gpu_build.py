"""Bitmaps built from their values on the MI355X (rbg_ctx_from_values[_device], rbg_build_values;
RoaringBitmap.add(int...) / bitmapOf, RB/RoaringBitmap.java:483-570, optionally followed by runOptimize(),
:2764-2774).  The acceptance throughout: the built batch, fetched, is byte for byte what the host builder
O.from_values gives, with and without run_optimize, and it behaves as the loaded batch of those bytes does
in every op that takes one."""
import numpy as np
import pytest

import _gen
import _oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng(gpu):
    import roaringbitmap_amd as rb
    e = rb.Engine(0)
    yield e
    e.close()


def _u32(v):
    return np.ascontiguousarray(np.asarray(v, dtype=np.int64).astype(np.uint32))


def _check(eng, values, tag=""):
    """both run_optimize settings against the host builder; -> the run_optimize=False bytes"""
    v = _u32(values)
    out = None
    for ro in (False, True):
        want = O.from_values(v, ro)
        b = eng.from_values(v, ro)
        got = eng.batch_fetch(b).serialize()
        eng.release(b)
        assert got == want, (tag, ro, len(got), len(want))
        out = out or want
    return out


def _thrice_shuffled(rng, v):
    return rng.permutation(np.repeat(np.asarray(v, dtype=np.int64), 3))


@pytest.mark.parametrize("values", [[], [0], [0xFFFFFFFF], [0, 0xFFFFFFFF]], ids=["empty", "zero", "max", "ends"])
def test_edges(eng, values):
    _check(eng, values)


def test_one_value_per_key(eng):
    rng = np.random.default_rng(300)
    keys = rng.choice(65536, 300, replace=False).astype(np.int64)
    _check(eng, (keys << 16) | rng.integers(0, 65536, 300))


@pytest.mark.parametrize("distinct,kind", [(4096, "array"), (4097, "bitmap")])
def test_cardinality_threshold_with_duplicates(eng, distinct, kind):
    """the type comes from the distinct count: every value three times, shuffled"""
    rng = np.random.default_rng(distinct)
    lows = rng.choice(65536, distinct, replace=False).astype(np.int64)
    v = _thrice_shuffled(rng, (7 << 16) | lows)
    _check(eng, v)
    b = eng.from_values(v)
    st = eng.batch_stats(b)
    eng.release(b)
    assert st["containers"] == 1 and st[kind] == 1 and st["cardinality"] == distinct


def _runs(n_runs, length, stride):
    return (np.arange(n_runs, dtype=np.int64)[:, None] * stride + np.arange(length)[None, :]).reshape(-1)


RUN_CASES = {
    # A: R iff 2 card > 2 + 4 nruns
    "card3_one_run_stays_array": (np.arange(100, 103), "array"),
    "card4_one_run_becomes_run": (np.arange(100, 104), "run"),
    # B: R iff 2 + 4 nruns < 8192; runs of 3 values at stride 32 (card > 4096 either way)
    "runs_2047_becomes_run": (_runs(2047, 3, 32), "run"),
    "runs_2048_stays_bitmap": (_runs(2048, 3, 32), "bitmap"),
    "full_becomes_one_run": (np.arange(65536), "run"),
}


@pytest.mark.parametrize("name", list(RUN_CASES))
def test_run_thresholds(eng, name):
    lows, kind = RUN_CASES[name]
    rng = np.random.default_rng(len(name))
    v = rng.permutation((11 << 16) | np.asarray(lows, dtype=np.int64))
    _check(eng, v, name)
    b = eng.from_values(v, True)
    st = eng.batch_stats(b)
    eng.release(b)
    assert st["containers"] == 1 and st[kind] == 1, (name, st)


@pytest.mark.parametrize("mode", _gen.MODES)
def test_generator_modes(eng, mode):
    """a 12-key bitmap of the mode's containers, its values with 10 % duplicates, permuted"""
    rng = np.random.default_rng(5200 + _gen.MODES.index(mode))
    keys = np.sort(rng.choice(65536, 12, replace=False))
    v = O.to_values(_gen.bitmap(rng, keys, modes=[mode], p_present=1.0)).astype(np.int64)
    v = rng.permutation(np.concatenate([v, v[rng.integers(0, v.size, size=v.size // 10 + 1)]]))
    _check(eng, v, mode)


def _orders():
    rng = np.random.default_rng(22)
    base = rng.integers(0, 1 << 22, size=200000)
    return {
        "ascending": np.sort(base),
        "descending": np.sort(base)[::-1],
        "random": base,
        "one_value": np.full(100000, (3 << 16) + 77),  # every lane of every wave hits one word
        "sorted_dense": np.arange(3 * 65536 + 1000),  # 64 lanes span two words
    }


ORDERS = _orders()


@pytest.mark.parametrize("name", list(ORDERS))
def test_input_orders(eng, name):
    _check(eng, ORDERS[name], name)


PAD_CARDS = _gen.PAD_CARDS


def _pad_values(rng, shift=0):
    """one array container of every card in PAD_CARDS (keys 0..7), values away from 0 and 65535"""
    out = []
    for k, c in enumerate(PAD_CARDS):
        lows = np.sort(rng.choice(60000, c, replace=False)) + 100 + shift
        out.append((k << 16) | lows.astype(np.int64))
    return np.concatenate(out)


def test_array_slot_padding(eng):
    """an array slot is padded to 16 B with copies of its last value: ops that read whole 16 B vectors of
    two built batches, and point queries at the last value"""
    rng = np.random.default_rng(16)
    va, vb = _pad_values(rng), np.concatenate([_pad_values(rng, 1), _pad_values(rng)[::2]])
    a, b = eng.from_values(rng.permutation(va)), eng.from_values(rng.permutation(vb))
    ba, bb = O.from_values(_u32(va)), O.from_values(_u32(vb))
    assert eng.batch_fetch(a).serialize() == ba and eng.batch_fetch(b).serialize() == bb
    for op in ("or", "xor", "and", "andnot"):
        eng.pairwise(op, a, b)
        assert eng.fetch().serialize() == O.pairwise(op, ba, bb), op
        eng.pairwise(op, b, a)
        assert eng.fetch().serialize() == O.pairwise(op, bb, ba), op
    eng.wide("or", a)
    got = eng.fetch().serialize()
    assert got == O.wide("or", [ba]) and (O.to_values(got) == np.unique(_u32(va))).all()
    sv = np.unique(va)
    ends = np.cumsum(PAD_CARDS)
    last = sv[ends - 1]  # the last value of every container
    assert (eng.point_query("select", a, ends - 1) == last).all()
    assert (eng.point_query("rank", a, last) == ends).all()
    assert (eng.point_query("next", a, last) == last).all()
    assert (eng.point_query("prev", a, last) == last).all()
    assert (eng.point_query("next", a, last[:-1] + 1) == sv[ends[:-1]]).all()  # past the padding: the next key's first
    eng.release(a)
    eng.release(b)


@pytest.mark.parametrize("ro", [False, True])
def test_as_operand(eng, ro):
    """a built batch against the loaded batch of the same bytes"""
    rng = np.random.default_rng(77 + ro)
    keys = np.arange(3, 15)
    v = O.to_values(_gen.bitmap(rng, keys, p_present=1.0)).astype(np.int64)
    v = rng.permutation(np.concatenate([v, v[::7]]))
    buf = O.from_values(_u32(v), ro)
    built, loaded = eng.from_values(v, ro), eng.load([buf])
    assert eng.batch_fetch(built).serialize() == buf
    sb, sl = eng.batch_stats(built), eng.batch_stats(loaded)
    assert len(sb) == 8 and sb == sl, (sb, sl)
    rb_, ab = eng.run_optimize(built)
    rl, al = eng.run_optimize(loaded)
    assert ab == al
    assert eng.batch_fetch(rb_).serialize() == eng.batch_fetch(rl).serialize() == O.run_optimize(buf)
    st, en = (4 << 16) + 12345, (9 << 16) + 5
    eng.range_mut("flip", built, st, en)
    got = eng.fetch().serialize()
    eng.range_mut("flip", loaded, st, en)
    assert got == eng.fetch().serialize() == O.range_mut("flip", buf, st, en)
    for off in (70001, -(2 << 16) - 9):
        eng.add_offset(built, off)
        got = eng.fetch().serialize()
        eng.add_offset(loaded, off)
        assert got == eng.fetch().serialize() == O.add_offset(buf, off), off
    for b in (built, loaded, rb_, rl):
        eng.release(b)


def test_torch_tensors(eng):
    import torch
    rng = np.random.default_rng(9)
    v = np.concatenate([rng.integers(0, 1 << 32, size=50000), [0xFFFFFFFF, 0, 0xFFFF0000]])
    dev = torch.device("cuda", 0)
    for ro in (False, True):
        want = O.from_values(_u32(v), ro)
        host = eng.from_values(v, ro)
        assert eng.batch_fetch(host).serialize() == want
        signed = np.where(v >= 1 << 31, v - (1 << 32), v).astype(np.int64)  # 0xFFFFFFFF as -1: the low 32 bits count
        assert signed.min() < 0 and -1 in signed
        for t in (torch.from_numpy(v.astype(np.int64)).to(dev), torch.from_numpy(signed).to(dev),
                  torch.from_numpy(_u32(v).view(np.int32)).to(dev).view(torch.uint32)):
            b = eng.from_values(t, ro)
            assert eng.batch_fetch(b).serialize() == want, (ro, t.dtype)
            eng.release(b)
        eng.release(host)
    e = eng.from_values(torch.zeros(0, dtype=torch.int64, device=dev))
    assert eng.batch_stats(e)["containers"] == 0
    eng.release(e)
    with pytest.raises(ValueError):
        eng.from_values(torch.zeros(4, dtype=torch.int32, device=dev))


def test_lifecycle(eng):
    rng = np.random.default_rng(4)
    v1, v2 = rng.integers(0, 1 << 24, size=5000), rng.integers(1 << 23, 1 << 25, size=7000)
    b1, b2 = eng.from_values(v1), eng.from_values(v2, True)
    assert b1 != b2
    assert eng.batch_fetch(b1).serialize() == O.from_values(_u32(v1))  # b2's build left b1 alone
    assert eng.batch_fetch(b2).serialize() == O.from_values(_u32(v2), True)
    eng.release(b1)
    b3 = eng.from_values(v1, True)
    assert eng.batch_fetch(b3).serialize() == O.from_values(_u32(v1), True)
    assert eng.batch_fetch(b2).serialize() == O.from_values(_u32(v2), True)
    eng.release(b2)
    eng.release(b3)
    big = rng.integers(0, 1 << 32, size=4_000_000, dtype=np.int64)  # every key, then three values
    bb = eng.from_values(big)
    small = eng.from_values([5, 1 << 20, 5])
    assert eng.batch_fetch(small).serialize() == O.from_values(_u32([5, 1 << 20]))
    assert eng.batch_fetch(bb).serialize() == O.from_values(_u32(big))
    eng.release(bb)
    eng.release(small)


def test_one_shot(gpu):
    import roaringbitmap_amd as rb
    rng = np.random.default_rng(12)
    v = np.concatenate([rng.integers(0, 1 << 21, size=100000), np.arange(5 << 16, (5 << 16) + 30000)])
    for ro in (False, True):
        got = rb.RoaringBitmap.from_values(v, ro, gpu=True).serialize()
        assert got == rb.RoaringBitmap.from_values(v, ro).serialize() == O.from_values(_u32(v), ro), ro
    assert rb.RoaringBitmap.from_values([], gpu=True).serialize() == rb.RoaringBitmap.from_values([]).serialize()
    assert rb.RoaringBitmap.bitmapOf(3, 1, 2).serialize() == rb.RoaringBitmap.from_values([1, 2, 3], gpu=True).serialize()
