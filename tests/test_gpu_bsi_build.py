"""A bit-sliced index built from (column, value) pairs on the MI355X (rbg_ctx_bsi_from_columns[_device],
rbg_bsi_from_columns; RoaringBitmapSliceIndex.setValue, BSI/:299-347, optionally followed by runOptimize(),
:141-150).  The acceptance throughout: the built batch, fetched, is byte for byte the oracle's ebM and slices
(tests/_bsi.py BSI.from_columns), with and without run_optimize, {nbits, min, max} are the oracle's, and the
batch behaves as the loaded batch of those bitmaps does in every op that takes one."""
import numpy as np
import pytest

import _bsi
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


def _fetch(eng, b):
    return [x.serialize() for x in eng.batch_fetch_range(b)]


def _check(eng, cols, vals, tag="", want=None):
    """both run_optimize settings against the oracle; -> {run_optimize: oracle index}"""
    cols, vals = np.asarray(cols, dtype=np.int64), np.asarray(vals, dtype=np.int64)
    out = {}
    for ro in (False, True):
        o = want[ro] if want else BSI.from_columns(cols, vals, ro)
        b, nbits, mn, mx = eng.bsi_from_columns(cols, vals, ro)
        got = _fetch(eng, b)
        eng.release(b)
        assert (nbits, mn, mx) == (o.bit_count(), o.min, o.max), (tag, ro)
        assert len(got) == 1 + nbits and got == [o.ebm] + o.ba, (tag, ro, [len(x) for x in got])
        out[ro] = o
    return out


def _kinds(buf):
    s = O.stats(buf)
    return s["array"], s["bitmap"], s["run"]


EDGES = {
    "empty": ([], []),
    "one_pair": ([12345], [5]),
    "all_zero_one_empty_slice": (np.arange(10) * 7001, np.zeros(10)),
    "int_max_31_slices": ([1, 70000, 3], [2**31 - 1, 0, 5]),
    "columns_0_and_max": ([0, 0xFFFFFFFF], [6, 9]),
}


@pytest.mark.parametrize("name", list(EDGES))
def test_edges(eng, name):
    cols, vals = EDGES[name]
    o = _check(eng, cols, vals, name)[False]
    if name == "empty":
        assert (o.bit_count(), o.min, o.max) == (0, 0, 0) and o.ebm == _bsi.EMPTY
    if name == "all_zero_one_empty_slice":
        assert o.ba == [_bsi.EMPTY]
    if name == "int_max_31_slices":
        assert o.bit_count() == 31
    if name == "columns_0_and_max":
        assert O.to_values(o.ebm).tolist() == [0, 0xFFFFFFFF]


def test_slice_without_a_container_under_a_key(eng):
    """three keys; key 5 holds even values only, so slice 0 has no container there and the key's segment
    holds fewer than nbits + 1 containers"""
    rng = np.random.default_rng(31)
    cols = np.concatenate([rng.choice(65536, 300, replace=False), (5 << 16) + rng.choice(65536, 5000, replace=False),
                           (65535 << 16) + np.array([0, 1, 65535])]).astype(np.int64)
    vals = rng.integers(0, 1 << 20, size=cols.size)
    vals[(cols >> 16) == 5] &= ~1
    p = rng.permutation(cols.size)
    o = _check(eng, cols[p], vals[p])[False]
    assert sum(_kinds(o.ebm)) == 3 and sum(_kinds(o.ba[0])) == 2


def test_full_slice_container(eng):
    """65,536 columns of one key whose values all have bit 2: a full bitmap, one run with run_optimize"""
    rng = np.random.default_rng(32)
    cols = np.concatenate([(3 << 16) + np.arange(65536), rng.choice(65536, 2000, replace=False)]).astype(np.int64)
    vals = rng.integers(0, 64, size=cols.size)
    vals[:65536] |= 4
    p = rng.permutation(cols.size)
    o = _check(eng, cols[p], vals[p])
    full = (3 << 16) + np.arange(65536)
    assert np.isin(full, O.to_values(o[False].ba[2])).all()
    assert _kinds(o[True].ba[2])[2] >= 1


@pytest.mark.parametrize("card,kind", [(4096, (1, 0, 0)), (4097, (0, 1, 0))])
def test_cardinality_threshold_in_a_slice(eng, card, kind):
    """the 4096 / 4097 boundary met by slice 0 alone: ebM's container holds 6,000 columns either way"""
    rng = np.random.default_rng(card)
    cols = (9 << 16) + rng.choice(65536, 6000, replace=False).astype(np.int64)
    vals = np.full(6000, 2)
    vals[:card] |= 1
    p = rng.permutation(6000)
    o = _check(eng, cols[p], vals[p])[False]
    assert _kinds(o.ebm) == (0, 1, 0) and _kinds(o.ba[0]) == kind and O.stats(o.ba[0])["card"] == card


def _runs(n_runs, length, stride):
    return (np.arange(n_runs, dtype=np.int64)[:, None] * stride + np.arange(length)[None, :]).reshape(-1)


RUN_CASES = {
    # A: R iff 2 card > 2 + 4 nruns
    "card3_one_run_stays_array": (np.arange(100, 103), (1, 0, 0)),
    "card4_one_run_becomes_run": (np.arange(100, 104), (0, 0, 1)),
    # B: R iff 2 + 4 nruns < 8192; runs of 3 values at stride 32 (card > 4096 either way)
    "runs_2047_becomes_run": (_runs(2047, 3, 32), (0, 0, 1)),
    "runs_2048_stays_bitmap": (_runs(2048, 3, 32), (0, 1, 0)),
}


@pytest.mark.parametrize("name", list(RUN_CASES))
def test_run_thresholds_in_a_slice(eng, name):
    """slice 0 sits on a runOptimize boundary; ebM is the whole key (one run) and slice 1 is random"""
    lows, kind = RUN_CASES[name]
    rng = np.random.default_rng(len(name))
    cols = (11 << 16) + np.arange(65536, dtype=np.int64)
    vals = rng.integers(0, 2, size=65536) << 1
    vals[np.asarray(lows)] |= 1
    p = rng.permutation(65536)
    o = _check(eng, cols[p], vals[p], name)[True]
    assert _kinds(o.ba[0]) == kind and _kinds(o.ebm) == (0, 0, 1), (name, _kinds(o.ba[0]))


def _nine_keys():
    """about 200,000 pairs over nine keys (65535 among them): arrays, bitmaps and, in the sorted stretch of
    key 40, runs"""
    rng = np.random.default_rng(22)
    keys = np.array([0, 1, 7, 40, 41, 300, 4000, 65534, 65535], dtype=np.int64)
    sizes = [30000, 100, 60000, 50000, 5, 4096, 4097, 20000, 35000]
    cols = np.concatenate([(k << 16) + (np.arange(s) if k == 40 else rng.choice(65536, s, replace=False))
                           for k, s in zip(keys, sizes)]).astype(np.int64)
    vals = rng.integers(0, 1 << 20, size=cols.size)
    vals[(cols >> 16) == 40] = (cols[(cols >> 16) == 40] & 0xFFFF) // 3000  # clustered: long runs in the slices
    return cols, vals


NINE = _nine_keys()
_nine_want = {}


def _nine_oracle():
    if not _nine_want:
        for ro in (False, True):
            _nine_want[ro] = BSI.from_columns(NINE[0], NINE[1], ro)
    return _nine_want


def _orders():
    cols, vals = NINE
    rng = np.random.default_rng(23)
    n = cols.size
    return {
        "ascending": np.argsort(cols),
        "descending": np.argsort(cols)[::-1],
        "random": rng.permutation(n),
        "by_value": np.argsort(vals, kind="stable"),
        "keys_interleaved": np.argsort(cols & 0xFFFF, kind="stable"),  # neighbouring lanes hit different keys
    }


ORDERS = _orders()


@pytest.mark.parametrize("name", list(ORDERS))
def test_input_orders(eng, name):
    p = ORDERS[name]
    _check(eng, NINE[0][p], NINE[1][p], name, want=_nine_oracle())


@pytest.mark.parametrize("budget", ["one_key", "1", "two_keys"])
def test_forced_passes(eng, monkeypatch, budget):
    """the workspace budget forced down through the environment switch: whole keys per pass, the same bytes"""
    want = _nine_oracle()
    m = want[False].bit_count() + 1
    nbytes = {"one_key": 8192 * m, "1": 1, "two_keys": 2 * 8192 * m + 100}[budget]
    keys_per_pass = max(1, nbytes // (8192 * m))
    assert -(-9 // keys_per_pass) >= 3  # nine keys: at least three passes
    monkeypatch.setenv("RBG_BSI_BUILD_WS", str(nbytes))
    p = ORDERS["random"]
    _check(eng, NINE[0][p], NINE[1][p], budget, want=want)
    monkeypatch.delenv("RBG_BSI_BUILD_WS")
    _check(eng, NINE[0][p], NINE[1][p], "default again", want=want)


@pytest.mark.parametrize("ro", [False, True])
def test_as_bsi_operand(eng, ro):
    """Engine.bsi / bsi_buffer over the built batch against the loaded batch of the oracle's bitmaps"""
    cols, vals = NINE
    o = _nine_oracle()[ro]
    built, nbits, mn, mx = eng.bsi_from_columns(cols, vals, ro)
    loaded = eng.load([o.ebm] + o.ba)
    sb, sl = eng.batch_stats(built), eng.batch_stats(loaded)
    assert len(sb) == 8 and sb == sl, (sb, sl)
    assert (eng.batch_counts(built) == eng.batch_counts(loaded)).all()
    rng = np.random.default_rng(90 + ro)
    for op in _bsi.OPS:
        for a, e in ((int(vals[5]), int(vals[5]) + 1000), tuple(sorted(int(x) for x in rng.integers(0, mx + 2, 2)))):
            res = []
            for b in (built, loaded):
                eng.bsi(b, op, nbits, a, e, mn, mx, want_sum=True)
                res.append((eng.fetch().serialize(), eng.bsi_sums()))
            assert res[0] == res[1] and res[0][0] == o.compare(op, a, e), (op, a, e)
            assert res[0][1] == o.sum(res[0][0])
    for op in list(range(7)) + [7]:  # 7: rangeNEQ called directly
        a, e = sorted(int(x) for x in rng.integers(0, mx + 2, 2))
        res = []
        for b in (built, loaded):
            eng.bsi_buffer(b, op, nbits, a, e, mn, mx)
            res.append(eng.fetch().serialize())
        assert res[0] == res[1], (op, a, e)
    if not ro:
        rb_, ab = eng.run_optimize(built)
        rl, al = eng.run_optimize(loaded)
        want = _nine_oracle()[True]
        assert ab == al and _fetch(eng, rb_) == _fetch(eng, rl) == [want.ebm] + want.ba
        eng.release(rb_)
        eng.release(rl)
    st, en = (1 << 16) + 5, (41 << 16) + 2
    sb_, sl_ = eng.select_range(built, st, en), eng.select_range(loaded, st, en)
    assert _fetch(eng, sb_) == _fetch(eng, sl_)
    for b in (built, loaded, sb_, sl_):
        eng.release(b)


def _pad_pairs(values):
    """PAD_CARDS[k] columns under key k (never adjacent); every value 3, or values drawn from {1, 2, 3}"""
    rng = np.random.default_rng(62)
    cols = np.concatenate([(k << 16) | lows for k, lows in enumerate(_gen.pad_lows(rng))])
    vals = np.full(cols.size, 3) if values == "all_3" else rng.integers(1, 4, size=cols.size)
    p = rng.permutation(cols.size)
    return cols[p], vals[p]


@pytest.mark.parametrize("ro", [False, True])
@pytest.mark.parametrize("values", ["all_3", "of_1_2_3"])
def test_array_slot_padding(eng, values, ro):
    """k_bsib_write's array slots are padded to 16 B with copies of their last value: small array containers of
    ebM and both slices, read by the BSI ops in whole 16 B vectors, against the loaded batch of the oracle's
    bitmaps and the oracle's own answers"""
    cols, vals = _pad_pairs(values)
    o = BSI.from_columns(cols, vals, ro)
    assert o.bit_count() == 2
    for x in [o.ebm] + o.ba:  # arrays only: the non-adjacent columns keep them under run_optimize
        ka, kb, kr = _kinds(x)
        assert ka >= 1 and (kb, kr) == (0, 0)
        if values == "all_3":  # ebM and both slices hold PAD_CARDS[k] values under key k
            assert ka == len(_gen.PAD_CARDS) and O.stats(x)["card"] == sum(_gen.PAD_CARDS)
    built, nbits, mn, mx = eng.bsi_from_columns(cols, vals, ro)
    loaded = eng.load([o.ebm] + o.ba)
    assert (nbits, mn, mx) == (2, o.min, o.max) and _fetch(eng, built) == [o.ebm] + o.ba
    for op in _bsi.OPS:
        for a, e in ((3, 3), (1, 2), (2, 5), (0, 1)):
            res = []
            for b in (built, loaded):
                eng.bsi(b, op, nbits, a, e, mn, mx, want_sum=True)
                res.append((eng.fetch().serialize(), eng.bsi_sums()))
            assert res[0] == res[1] and res[0][0] == o.compare(op, a, e), (op, a, e)
            assert res[0][1] == o.sum(res[0][0])
    for op in list(range(7)) + [7]:  # 7: rangeNEQ called directly
        for a, e in ((3, 3), (1, 2), (2, 5)):
            res = []
            for b in (built, loaded):
                eng.bsi_buffer(b, op, nbits, a, e, mn, mx)
                res.append(eng.fetch().serialize())
            assert res[0] == res[1], (op, a, e)
    eng.release(built)
    eng.release(loaded)


def test_refusals_leave_no_batch(eng):
    import roaringbitmap_amd as rb
    cols, vals = np.array([5, 70000, 6, 7]), np.array([1, 2, 3, 4])
    ok, *_ = eng.bsi_from_columns(cols, vals)
    eng.release(ok)
    neg = vals.copy()
    neg[2] = -1
    with pytest.raises(rb.IllegalArgumentException):
        eng.bsi_from_columns(cols, neg)
    # the device entry point's own check (the Python layer looks at int64 values before it)
    import torch
    t = torch.from_numpy(neg.astype(np.int32)).to("cuda:0")
    with pytest.raises(rb.IllegalArgumentException):
        eng.bsi_from_columns(torch.from_numpy(cols).to("cuda:0"), t)
    for v in (np.array([1, 2, 3, 1]), np.array([1, 2, 3, 9])):  # the repeated column with an equal / another value
        with pytest.raises(rb.IllegalArgumentException):
            eng.bsi_from_columns(np.array([5, 70000, 6, 5]), v)
    with pytest.raises(rb.IllegalArgumentException):
        eng.bsi_from_columns(cols, vals[:3])
    again, nbits, mn, mx = eng.bsi_from_columns(cols, vals)
    assert again == ok  # every refusal freed its slot: the next build takes the released id
    o = BSI.from_columns(cols, vals)
    assert _fetch(eng, again) == [o.ebm] + o.ba and (nbits, mn, mx) == (3, 1, 4)
    eng.release(again)


def test_torch_tensors(eng):
    import torch
    rng = np.random.default_rng(9)
    cols = np.unique(np.concatenate([rng.integers(0, 1 << 32, size=50000), [0xFFFFFFFF, 0, 0xFFFF0000]]))
    cols = rng.permutation(cols)
    vals = rng.integers(0, 1 << 31, size=cols.size)
    dev = torch.device("cuda", 0)
    signed = np.where(cols >= 1 << 31, cols - (1 << 32), cols).astype(np.int64)  # 0xFFFFFFFF as -1: the low 32 bits count
    for ro in (False, True):
        o = BSI.from_columns(cols, vals, ro)
        for tc, tv in ((torch.from_numpy(cols.astype(np.int64)).to(dev), torch.from_numpy(vals).to(dev)),
                       (torch.from_numpy(signed).to(dev), torch.from_numpy(vals.astype(np.int32)).to(dev)),
                       (torch.from_numpy(cols.astype(np.uint32).view(np.int32)).to(dev).view(torch.uint32),
                        torch.from_numpy(vals.astype(np.int32)).to(dev))):
            b, nbits, mn, mx = eng.bsi_from_columns(tc, tv, ro)
            assert (nbits, mn, mx) == (o.bit_count(), o.min, o.max)
            assert _fetch(eng, b) == [o.ebm] + o.ba, (ro, tc.dtype)
            eng.release(b)
    e, nbits, mn, mx = eng.bsi_from_columns(torch.zeros(0, dtype=torch.int64, device=dev),
                                            torch.zeros(0, dtype=torch.int64, device=dev))
    assert (nbits, mn, mx) == (0, 0, 0) and eng.batch_stats(e)["bitmaps"] == 1 and eng.batch_stats(e)["containers"] == 0
    eng.release(e)
    with pytest.raises(ValueError):
        eng.bsi_from_columns(torch.zeros(4, dtype=torch.float32, device=dev), torch.zeros(4, dtype=torch.int64, device=dev))


def test_one_shot(gpu):
    import roaringbitmap_amd as rb
    cols, vals = NINE
    p = ORDERS["random"][::3]
    for ro in (False, True):
        g = rb.RoaringBitmapSliceIndex.from_columns(cols[p], vals[p], ro, gpu=True)
        h = rb.RoaringBitmapSliceIndex.from_columns(cols[p], vals[p], ro)
        o = BSI.from_columns(cols[p], vals[p], ro)
        assert g.ebM.serialize() == h.ebM.serialize() == o.ebm
        assert [b.serialize() for b in g.bA] == [b.serialize() for b in h.bA] == o.ba
        assert (g.minValue, g.maxValue, g.runOptimized) == (h.minValue, h.maxValue, h.runOptimized) == (o.min, o.max, ro)
    e = rb.RoaringBitmapSliceIndex.from_columns([], [], gpu=True)
    assert e.ebM.serialize() == _bsi.EMPTY and e.bA == [] and (e.minValue, e.maxValue) == (0, 0)
    with pytest.raises(rb.IllegalArgumentException):
        rb.RoaringBitmapSliceIndex.from_columns([1, 1], [2, 3], gpu=True)
