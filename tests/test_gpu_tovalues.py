"""Resident bitmaps expanded to their values on the MI355X (rbg_ctx_to_values[_device], rbg_expand_values;
RoaringBitmap.toArray, RB/RoaringBitmap.java:3224, and the window BatchIterator.nextBatch / limit walk):
every result equals O.to_values(buf)[first:first + count], ascending and unsigned."""
import numpy as np
import pytest

import _gen
import _oracle as O
from _fmt import R, encode

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng(gpu):
    import roaringbitmap_amd as rb
    e = rb.Engine(0)
    yield e
    e.close()


def _same(got, want, tag=""):
    assert isinstance(got, np.ndarray) and got.dtype == np.uint32 and got.shape == want.shape, (tag, got.shape, want.shape)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (tag, [(int(i), int(got[i]), int(want[i])) for i in bad[:5]])


@pytest.mark.parametrize("mode", _gen.MODES)
def test_generator_modes(eng, mode):
    rng = np.random.default_rng(6100 + _gen.MODES.index(mode))
    keys = np.concatenate([np.sort(rng.choice(65535, 11, replace=False)), [65535]])  # the top key: nothing sign-extended
    buf = _gen.bitmap(rng, keys, modes=[mode], p_present=1.0)
    want = O.to_values(buf)
    assert want.dtype == np.uint32 and want[-1] >= 0xFFFF0000
    b = eng.load([buf])
    _same(eng.to_values(b), want, mode)
    eng.release(b)


@pytest.fixture(scope="module")
def mix(eng):
    """nine keys, A / B / R in turn: (batch, values, per-container cardinalities, containers)"""
    rng = np.random.default_rng(909)
    modes = ["a_mid", "b_mid", "r_mid", "a_small", "b_sparse_runs", "r_few", "a_edge", "b_dense", "r_many"]
    ctrs = [(3 * k + 1, *_gen.container(rng, m)) for k, m in enumerate(modes)]
    buf = encode(ctrs)
    b = eng.load([buf])
    yield b, O.to_values(buf), [len(c[2]) for c in ctrs], ctrs
    eng.release(b)


def test_windows(eng, mix):
    b, v, cards, ctrs = mix
    card = v.size
    rng = np.random.default_rng(31)
    wins = [(0, 0), (card, 5), (card - 1, 5), (0, card + 7), (card + 100, 0)]
    bounds = np.concatenate([[0], np.cumsum(cards)])
    for e in bounds[1:-1]:
        e = int(e)
        wins += [(e - 1, 1), (e - 1, 2), (e, 1), (e + 1, 3), (e - 1, 70), (0, e), (0, e + 1), (0, e - 1), (e, card)]
    # a start in the middle of a bitmap word: the rank of a value of container 1 (B) whose bit is not bit 0
    lows = np.asarray(ctrs[1][2], dtype=np.int64)
    inner = int(np.nonzero((lows & 63) > 20)[0][5])
    wins += [(int(bounds[1]) + inner, 200), (int(bounds[1]) + inner, 1), (int(bounds[1]) + inner, 5000)]
    # a start in the middle of a run: container 5 (R, r_few: runs of 100 values and more)
    wins += [(int(bounds[5]) + 37, 300), (int(bounds[5]) + 37, 1), (int(bounds[5]) + 37, cards[5])]
    # inside the run container of more than 2,047 runs
    wins += [(int(bounds[8]) + 1234, 4000)]
    for _ in range(200):
        f = int(rng.integers(0, card))
        wins.append((f, int(rng.integers(0, 3000)) if rng.random() < 0.7 else int(rng.integers(0, card))))
    for f, c in wins:
        _same(eng.to_values(b, first=f, count=c), v[f:f + c], (f, c))
    _same(eng.to_values(b, first=int(bounds[4]) + 9), v[int(bounds[4]) + 9:], "count=None")


def test_long_runs(eng):
    import roaringbitmap_amd as rb
    n = 3 * 65536 + 1000
    rng_bm = rb.RoaringBitmap.bitmapOfRange(0, n)
    assert O.stats(rng_bm.serialize())["run"] == 4  # three one-run full containers and a partial one
    b = eng.load([rng_bm])
    want = np.arange(n, dtype=np.uint32)
    _same(eng.to_values(b), want, "range")
    _same(eng.to_values(b, first=65536 + 77, count=70000), want[65536 + 77:65536 + 77 + 70000], "range window")
    eng.release(b)
    starts = np.arange(2500) * 26 + 3
    two = np.sort(np.concatenate([starts, starts + 1]))  # 2,500 runs of two values
    runs65 = (np.arange(65)[:, None] * 1000 + np.arange(9)[None, :]).reshape(-1)  # crosses one wave's width
    buf = encode([(1, R, two), (2, R, runs65), (65535, R, np.arange(65536))])
    b = eng.load([buf])
    want = O.to_values(buf)
    _same(eng.to_values(b), want, "runs")
    _same(eng.to_values(b, first=4999, count=600), want[4999:5599], "runs window")
    eng.release(b)


def test_device_made_batches(eng):
    rng = np.random.default_rng(55)
    buf = _gen.bitmap(rng, np.arange(10, 22), p_present=1.0)
    want = O.to_values(buf)
    a = eng.load([buf])
    ro, _ = eng.run_optimize(a)  # holes after the containers that shrank
    _same(eng.to_values(ro), want, "runOptimize result")
    _same(eng.to_values(ro, first=want.size // 3, count=50000), want[want.size // 3:want.size // 3 + 50000], "ro window")
    for flag in (False, True):
        built = eng.from_values(rng.permutation(want.astype(np.int64)), flag)
        _same(eng.to_values(built), want, f"from_values {flag}")
        eng.release(built)
    eng.release(ro)
    eng.release(a)
    e = eng.from_values([])
    _same(eng.to_values(e), np.zeros(0, dtype=np.uint32), "empty")
    _same(eng.to_values(e, first=3, count=4), np.zeros(0, dtype=np.uint32), "empty window")
    eng.release(e)


def test_round_trip(eng):
    rng = np.random.default_rng(1 << 20)
    v = rng.integers(0, 1 << 32, size=1 << 20, dtype=np.int64)
    b = eng.from_values(v)
    _same(eng.to_values(b), np.unique(v).astype(np.uint32), "round trip")
    eng.release(b)
    v = rng.integers(0, 1 << 23, size=1 << 20, dtype=np.int64)  # dense keys: bitmap containers
    b = eng.from_values(v, True)
    _same(eng.to_values(b), np.unique(v).astype(np.uint32), "round trip dense")
    eng.release(b)


def test_torch_outputs(eng, mix):
    import torch
    b, v, cards, _ = mix
    u = eng.to_values(b, dtype=torch.uint32)
    # used on torch's current stream right away, with no explicit synchronisation in between
    as64 = u.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    w = eng.to_values(b, dtype=torch.int64)
    same = bool((as64 == w).all())
    total = int(w.sum())
    assert isinstance(u, torch.Tensor) and u.dtype == torch.uint32 and u.device.type == "cuda" and u.numel() == v.size
    assert w.dtype == torch.int64 and same and total == int(v.astype(np.int64).sum())
    assert (w.cpu().numpy() == v.astype(np.int64)).all()
    assert (u.cpu().view(torch.int32).numpy().view(np.uint32) == v).all()
    f, c = cards[0] + 17, 9000
    win = eng.to_values(b, first=f, count=c, dtype=torch.int64)
    picked = torch.zeros(1 << 20, dtype=torch.int64, device=win.device)
    picked[win - (1 << 16)] = 1  # the values as indices, as torch indexing takes them
    assert int(picked.sum()) == c and (win.cpu().numpy() == v[f:f + c].astype(np.int64)).all()
    assert eng.to_values(b, first=v.size, count=5, dtype=torch.int64).numel() == 0
    with pytest.raises(ValueError):
        eng.to_values(b, dtype=torch.int32)


def test_refusals(eng):
    import roaringbitmap_amd as rb
    rng = np.random.default_rng(8)
    bufs = [_gen.bitmap(rng, np.arange(4), p_present=1.0), _gen.bitmap(rng, np.arange(2, 6), p_present=1.0)]
    packed = eng.load([O.from_values(np.arange(0, 3 << 16, 97, dtype=np.uint32))], packed=True)
    with pytest.raises(rb.IllegalArgumentException, match="slot-aligned"):
        eng.to_values(packed)
    two = eng.load(bufs)
    with pytest.raises(rb.IllegalArgumentException):
        eng.to_values(two)
    one = eng.load([bufs[0]])
    with pytest.raises(rb.IllegalArgumentException):
        eng.to_values(one, ia=1)
    with pytest.raises(rb.IllegalArgumentException):
        eng.to_values(12345)  # no such batch
    _same(eng.to_values(one), O.to_values(bufs[0]), "after the refusals")
    for b in (packed, two, one):
        eng.release(b)


def test_one_shot(gpu):
    import roaringbitmap_amd as rb
    rng = np.random.default_rng(3)
    buf = _gen.bitmap(rng, np.concatenate([np.arange(5), [40000, 65535]]), p_present=1.0)
    x = rb.RoaringBitmap(buf)
    got = x.toArray(gpu=True)
    _same(got, x.toArray(), "one-shot")
    _same(got, O.to_values(buf), "one-shot oracle")
    assert rb.RoaringBitmap().toArray(gpu=True).shape == (0,)
