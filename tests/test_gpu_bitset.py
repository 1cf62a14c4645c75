"""Dense bitsets and masks to resident bitmaps and back on the MI355X (rbg_ctx_from_bitset[_device],
rbg_ctx_to_bitset[_device], rbg_bitset_build / rbg_bitset_expand; BitSetUtil, RB/BitSetUtil.java).  A build's
acceptance: the built batch, fetched, is byte for byte what the host builder O.from_values gives for the set bit
positions, with and without run_optimize.  An expansion's: every word / byte of the window equals the bits of
toArray(), and nothing outside the window is written."""
import ctypes

import numpy as np
import pytest

import _gen
import _oracle as O
from _fmt import encode

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng(gpu):
    import roaringbitmap_amd as rb
    e = rb.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def dev(gpu):
    import torch
    return torch.device("cuda", 0)


def _words(bits):
    """bits (0 / 1 per position) as little-endian uint64 words, zero padded"""
    bits = np.asarray(bits, dtype=np.uint8)
    bits = np.concatenate([bits, np.zeros(-bits.size % 64, dtype=np.uint8)])
    return np.packbits(bits, bitorder="little").view("<u8").astype(np.uint64)


def _fetch(eng, b):
    got = eng.batch_fetch(b).serialize()
    eng.release(b)
    return got


def _t64(words, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(words).view(np.int64)).to(dev)


def _check_words(eng, dev, words, tag=""):
    """both run_optimize settings, the uploaded and the in-place form, against the host builder"""
    words = np.ascontiguousarray(words, dtype=np.uint64)
    pos = np.flatnonzero(np.unpackbits(words.view(np.uint8), bitorder="little")).astype(np.uint32)
    t = _t64(words, dev)
    for ro in (False, True):
        want = O.from_values(pos, ro)
        assert _fetch(eng, eng.from_words(words, ro)) == want, (tag, ro, "numpy")
        assert _fetch(eng, eng.from_words(t, ro)) == want, (tag, ro, "torch")
    return pos


# ---- build, packed -------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, 7, 8, 9])
def test_byte_lengths(eng, dev, n):
    import torch
    b = np.random.default_rng(100 + n).integers(1, 256, size=n, dtype=np.uint8)
    pos = np.flatnonzero(np.unpackbits(b, bitorder="little")).astype(np.uint32)
    for ro in (False, True):
        want = O.from_values(pos, ro)
        assert _fetch(eng, eng.from_words(b.tobytes(), ro)) == want
        assert _fetch(eng, eng.from_words(b, ro)) == want
        assert _fetch(eng, eng.from_words(torch.from_numpy(b.copy()).to(dev), ro)) == want
    if n == 0:
        e = eng.from_words(b"")
        assert eng.batch_stats(e)["containers"] == 0 and eng.to_values(e).size == 0  # a live empty batch
        eng.release(e)


@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 2049])
def test_word_lengths(eng, dev, n):
    rng = np.random.default_rng(n)
    words = _words(rng.random(64 * n) < 0.3)
    words[-1] |= np.uint64(1 << 63)  # the last bit of the input counts
    pos = _check_words(eng, dev, words, n)
    assert pos[-1] == 64 * n - 1


def test_key_gaps_and_cardinality_threshold(eng, dev):
    """keys {0, 3, 7} with all-zero blocks between; blocks of exactly 4,096 (array) and 4,097 bits (bitmap)"""
    rng = np.random.default_rng(37)
    bits = np.zeros(8 << 16, dtype=np.uint8)
    for k, c in ((0, 4096), (3, 4097), (7, 11)):
        bits[(k << 16) + rng.choice(1 << 16, c, replace=False)] = 1
    words = _words(bits)
    _check_words(eng, dev, words)
    b = eng.from_words(words)
    st = eng.batch_stats(b)
    eng.release(b)
    assert (st["containers"], st["array"], st["bitmap"], st["run"], st["cardinality"]) == (3, 2, 1, 0, 4096 + 4097 + 11)


def test_full_block(eng, dev):
    words = np.full(1024, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    _check_words(eng, dev, words)
    for ro, kind in ((False, "bitmap"), (True, "run")):
        b = eng.from_words(words, ro)
        st = eng.batch_stats(b)
        eng.release(b)
        assert st["containers"] == 1 and st[kind] == 1, (ro, st)


def _runs(n_runs, length, stride):
    return (np.arange(n_runs, dtype=np.int64)[:, None] * stride + np.arange(length)[None, :]).reshape(-1)


RUN_CASES = {  # A: R iff 2 card > 2 + 4 nruns; B: R iff 2 + 4 nruns < 8192
    "card3_one_run_stays_array": (np.arange(100, 103), "array"),
    "card4_one_run_becomes_run": (np.arange(100, 104), "run"),
    "runs_2047_becomes_run": (_runs(2047, 3, 32), "run"),
    "runs_2048_stays_bitmap": (_runs(2048, 3, 32), "bitmap"),
    "full_becomes_one_run": (np.arange(65536), "run"),
}


@pytest.mark.parametrize("name", list(RUN_CASES))
def test_run_thresholds(eng, dev, name):
    lows, kind = RUN_CASES[name]
    bits = np.zeros(12 << 16, dtype=np.uint8)
    bits[(11 << 16) + np.asarray(lows)] = 1
    words = _words(bits)
    _check_words(eng, dev, words, name)
    b = eng.from_words(words, True)
    st = eng.batch_stats(b)
    eng.release(b)
    assert st["containers"] == 1 and st[kind] == 1, (name, st)


def test_nothing_behind_the_end_is_read(eng, dev):
    """a short last block in a larger tensor of ones: words, and bytes that end inside a word"""
    import torch
    rng = np.random.default_rng(5)
    n = 1024 + 500
    words = _words(rng.random(64 * n) < 0.4)
    big = torch.full((3 * 1024,), -1, dtype=torch.int64, device=dev)
    big[:n] = _t64(words, dev)
    pos = np.flatnonzero(np.unpackbits(words.view(np.uint8), bitorder="little")).astype(np.uint32)
    raw = big.view(torch.uint8)
    for ro in (False, True):
        assert _fetch(eng, eng.from_words(big[:n], ro)) == O.from_values(pos, ro)
        for tail in (1, 3, 7):
            nb = 8 * (n - 1) + tail
            cut = pos[pos < 8 * nb]
            assert _fetch(eng, eng.from_words(raw[:nb], ro)) == O.from_values(cut, ro), (ro, tail)


def test_eight_byte_aligned_view(eng, dev):
    import torch
    rng = np.random.default_rng(6)
    words = _words(rng.random(64 * 2050) < 0.2)
    t = _t64(words, dev)
    v = t[1:]
    assert v.data_ptr() % 16 == 8
    pos = np.flatnonzero(np.unpackbits(words[1:].view(np.uint8), bitorder="little")).astype(np.uint32)
    for ro in (False, True):
        assert _fetch(eng, eng.from_words(v, ro)) == O.from_values(pos, ro)
    odd = t.view(torch.uint8)[3:8 * 1100 + 3]  # a byte view at an odd address: copied to an aligned one
    ob = words.view(np.uint8)[3:8 * 1100 + 3]
    assert _fetch(eng, eng.from_words(odd)) == O.from_values(
        np.flatnonzero(np.unpackbits(ob, bitorder="little")).astype(np.uint32))
    assert _fetch(eng, eng.from_words(t[::2])) == O.from_values(  # not contiguous
        np.flatnonzero(np.unpackbits(words[::2].copy().view(np.uint8), bitorder="little")).astype(np.uint32))


def test_whole_universe(eng, dev):
    """2^26 words: bit positions at and above 2^31, key 65535; one word more is refused before any device work"""
    import torch
    import roaringbitmap_amd as rb
    t = torch.zeros((1 << 26) + 1, dtype=torch.int64, device=dev)
    put = {0: 0b1011, 5: -(1 << 63), 32768 * 1024: 1, 32768 * 1024 + 1023: -1, 65535 * 1024 + 7: 0x5555, (1 << 26) - 1: -(1 << 63)}
    for w, x in put.items():
        t[w] = x
    pos = []
    for w, x in put.items():
        pos += [64 * w + i for i in range(64) if ((x & 0xFFFFFFFFFFFFFFFF) >> i) & 1]
    pos = np.asarray(sorted(pos), dtype=np.int64).astype(np.uint32)
    assert pos[-1] == 0xFFFFFFFF
    for ro in (False, True):
        assert _fetch(eng, eng.from_words(t[:1 << 26], ro)) == O.from_values(pos, ro)
    probe = eng.from_values([1])
    eng.release(probe)
    with pytest.raises(rb.IllegalArgumentException, match="2\\^32 bits"):
        eng.from_words(t)
    again = eng.from_values([1])
    eng.release(again)
    assert again == probe  # the refusal left no batch behind


# ---- build, mask ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 65535, 65536, 65537])
def test_mask_lengths(eng, dev, n):
    import torch
    rng = np.random.default_rng(7000 + n)
    m = rng.random(n) < 0.3
    if n:
        m[-1] = True
    pos = np.flatnonzero(m).astype(np.uint32)
    vals = np.where(m, rng.choice(np.array([1, 2, 255], dtype=np.uint8), size=n), 0).astype(np.uint8)  # 2 and 255 count
    big = torch.full((n + 300,), 255, dtype=torch.uint8, device=dev)  # nonzero memory behind the end
    big[:n] = torch.from_numpy(vals).to(dev)
    for ro in (False, True):
        want = O.from_values(pos, ro)
        assert _fetch(eng, eng.from_mask(m, ro)) == want, "numpy bool"
        assert _fetch(eng, eng.from_mask(vals, ro)) == want, "numpy uint8"
        assert _fetch(eng, eng.from_mask(torch.from_numpy(m).to(dev), ro)) == want, "torch bool"
        assert _fetch(eng, eng.from_mask(big[:n], ro)) == want, "torch uint8 view"
        if n > 3:
            assert _fetch(eng, eng.from_mask(big[3:n], ro)) == O.from_values(pos[pos >= 3] - 3, ro), "unaligned view"


def test_mask_not_contiguous(eng, dev):
    import torch
    rng = np.random.default_rng(71)
    m = rng.random(300001) < 0.5
    t = torch.from_numpy(m).to(dev)
    assert not t[::2].is_contiguous()
    assert _fetch(eng, eng.from_mask(t[::2])) == O.from_values(np.flatnonzero(m[::2]).astype(np.uint32))
    x = torch.from_numpy(rng.standard_normal(100000).astype(np.float32)).to(dev)
    assert _fetch(eng, eng.from_mask(x > 0, True)) == O.from_values(
        np.flatnonzero(x.cpu().numpy() > 0).astype(np.uint32), True)
    with pytest.raises(ValueError):
        eng.from_mask(x)


# ---- a built batch as an operand --------------------------------------------------------------------------

@pytest.mark.parametrize("ro", [False, True])
def test_as_operand(eng, dev, ro):
    """a batch built from words against the loaded batch of the same bytes"""
    rng = np.random.default_rng(770 + ro)
    v = O.to_values(_gen.bitmap(rng, np.arange(3, 15), p_present=1.0)).astype(np.int64)
    bits = np.zeros(15 << 16, dtype=np.uint8)
    bits[v] = 1
    buf = O.from_values(v.astype(np.uint32), ro)
    built, loaded = eng.from_words(_t64(_words(bits), dev), ro), eng.load([buf])
    assert eng.batch_fetch(built).serialize() == buf
    sb, sl = eng.batch_stats(built), eng.batch_stats(loaded)
    assert len(sb) == 8 and sb == sl, (sb, sl)
    other_buf = _gen.bitmap(rng, np.arange(0, 18), p_present=0.9)
    other = eng.load([other_buf])
    for op in ("xor", "and"):
        eng.pairwise(op, built, other)
        got = eng.fetch().serialize()
        eng.pairwise(op, loaded, other)
        assert got == eng.fetch().serialize() == O.pairwise(op, buf, other_buf), op
    rb_, ab = eng.run_optimize(built)
    rl, al = eng.run_optimize(loaded)
    assert ab == al
    assert eng.batch_fetch(rb_).serialize() == eng.batch_fetch(rl).serialize() == O.run_optimize(buf)
    q = np.concatenate([v[::997], v[::991] + 1, [0, (3 << 16) - 1, 15 << 16]])
    assert (eng.point_query("rank", built, q) == eng.point_query("rank", loaded, q)).all()
    assert (eng.point_query("rank", built, q) == np.searchsorted(v, q, side="right")).all()
    assert (eng.to_values(built) == v.astype(np.uint32)).all()
    for b in (built, loaded, other, rb_, rl):
        eng.release(b)


# ---- expansion ---------------------------------------------------------------------------------------------

KEYS = [1, 4, 7, 10, 13, 16, 19, 22, 65535]  # key gaps, and the top key: nothing sign-extended


@pytest.fixture(scope="module")
def mix(eng):
    """nine keys, A / B / R in turn -> (loaded batch, batch built on the device, values, containers)"""
    rng = np.random.default_rng(909)
    modes = ["a_mid", "b_mid", "r_mid", "a_small", "b_sparse_runs", "r_few", "a_edge", "b_dense", "r_many"]
    ctrs = [(k, *_gen.container(rng, m)) for k, m in zip(KEYS, modes)]
    buf = encode(ctrs)
    v = O.to_values(buf).astype(np.int64)
    loaded = eng.load([buf])
    built = eng.from_values(v, True)
    yield loaded, built, v, ctrs
    eng.release(loaded)
    eng.release(built)


def _bits(v, first, n):
    """the window [first, first + n) of the sorted values v as 0 / 1 bytes"""
    out = np.zeros(n, dtype=np.uint8)
    lo, hi = np.searchsorted(v, [first, first + n])
    out[v[lo:hi] - first] = 1
    return out


def test_whole_bitmap(eng, dev, mix):
    import torch
    loaded, built, v, _ = mix
    low = 23 << 16
    want_low = np.packbits(_bits(v, 0, low), bitorder="little").view("<u8").astype(np.uint64)
    want_top = np.packbits(_bits(v, 65535 << 16, 1 << 16), bitorder="little").view("<u8").astype(np.uint64)
    expect = torch.zeros(1 << 26, dtype=torch.int64, device=dev)
    expect[:low >> 6] = _t64(want_low, dev)
    expect[65535 << 10:] = _t64(want_top, dev)
    for b in (loaded, built):
        w = eng.to_words(b, n_words=1 << 26, dtype=torch.int64)  # the whole 32-bit universe
        same = bool(torch.equal(w, expect))  # on the current stream, no synchronisation in between
        assert w.dtype == torch.int64 and w.numel() == 1 << 26 and same
        del w
        got = eng.to_words(b, n_words=low >> 6)
        assert got.dtype == np.uint64 and (got == want_low).all()
        assert (eng.to_words(b, first_word=65535 << 10, n_words=1024) == want_top).all()
        m = eng.to_mask(b, n=low)
        assert m.dtype == np.bool_ and (m == _bits(v, 0, low).astype(bool)).all()
        assert (eng.to_mask(b, first=(65535 << 16) - 5, n=(1 << 16) + 5) == _bits(v, (65535 << 16) - 5, (1 << 16) + 5)).all()


def _windows(v, ctrs):
    """(first, n) windows in bit positions: the named cases, then seeded ones"""
    rng = np.random.default_rng(31)
    last = int(v[-1])
    wins = [(0, 1), (0, 64), (64, 64), (0, 1 << 16), (2 << 16, 2 << 16), (30000 << 16, 100000),  # in gaps
            (last, 1), (last + 1, 200), (last - 70, 300), ((1 << 32) - 64, 64), ((1 << 32) - 1000, 1000),
            (last + 1, (1 << 32) - last - 1)]  # past the last value, up to the end of the universe
    for key, _, lows in ctrs:  # starting and ending inside every container (A, B and R in turn)
        base = key << 16
        a, z = int(lows[len(lows) // 3]), int(lows[2 * len(lows) // 3])
        wins += [(base + a, z - a + 1), (base + a, 65536), (base - 5000, 5000 + z), (base + a + 1, 1),
                 (base, 65536), (base - 64, 65536 + 128), (base + 65536 - 100, 164)]
    while len(wins) < 200:
        key = KEYS[int(rng.integers(len(KEYS)))] + int(rng.integers(-1, 2))
        f = min(max((key << 16) + int(rng.integers(-70000, 70000)), 0), (1 << 32) - 1)
        n = int(rng.integers(1, 3000)) if rng.random() < 0.6 else int(rng.integers(1, 200000))
        wins.append((f, n))
    return [(f, min(n, (1 << 32) - f)) for f, n in wins]  # none reaches past the universe


def test_windows(eng, dev, mix):
    """about 200 windows through the device entry points into pre-filled buffers with guards: packed windows
    (first rounded down to a multiple of 64; n mostly no multiple of 64) and mask windows (any first, any
    output alignment); every fourth also through the host entry points"""
    import torch
    from roaringbitmap_amd import _lib as L
    loaded, built, v, ctrs = mix
    lib = L.lib()
    wins = _windows(v, ctrs)
    assert len(wins) >= 200 and sum(1 for f, n in wins if n % 64) > 100 and sum(1 for f, n in wins if f % 64) > 100
    cap = max(n for _, n in wins)
    gw = torch.empty(cap // 64 + 1 + 32, dtype=torch.int64, device=dev)
    gm = torch.empty(cap + 256 + 16, dtype=torch.uint8, device=dev)
    for i, (f, n) in enumerate(wins):
        b = (loaded, built)[i % 2]
        bits = _bits(v, f, n)
        # packed
        fp = f - f % 64
        np_ = min(n + (f - fp), (1 << 32) - fp)
        pb = _bits(v, fp, np_)
        nw = (np_ + 63) // 64
        want = np.packbits(np.concatenate([pb, np.zeros(-np_ % 64, dtype=np.uint8)]), bitorder="little").view("<u8")
        gw.fill_(-1)
        torch.cuda.synchronize()
        L.check(lib.rbg_ctx_to_bitset_device(eng._ctx, b, 0, fp, np_, L.RBG_BITS_PACKED,
                                             ctypes.c_void_p(gw.data_ptr() + 128)))
        eng.sync()
        got = gw.cpu().numpy().view(np.uint64)
        assert (got[16:16 + nw] == want).all(), ("packed", f, n)  # bits at or past n in the last word are zero
        assert (got[:16] == 0xFFFFFFFFFFFFFFFF).all() and (got[16 + nw:] == 0xFFFFFFFFFFFFFFFF).all(), ("guards", f, n)
        # mask, the output at every alignment in turn
        shift = 128 + i % 16
        gm.fill_(255)
        torch.cuda.synchronize()
        L.check(lib.rbg_ctx_to_bitset_device(eng._ctx, b, 0, f, n, L.RBG_BITS_BYTES,
                                             ctypes.c_void_p(gm.data_ptr() + shift)))
        eng.sync()
        got = gm.cpu().numpy()
        assert (got[shift:shift + n] == bits).all(), ("mask", f, n)
        assert (got[:shift] == 255).all() and (got[shift + n:] == 255).all(), ("mask guards", f, n)
        if i % 4 == 0:
            hw = np.full(nw + 32, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
            L.check(lib.rbg_ctx_to_bitset(eng._ctx, b, 0, fp, np_, L.RBG_BITS_PACKED, ctypes.c_void_p(hw.ctypes.data + 128)))
            assert (hw[16:16 + nw] == want).all() and (hw[:16] == hw[0]).all() and (hw[16 + nw:] == hw[0]).all()
            hm = np.full(n + 256, 255, dtype=np.uint8)
            L.check(lib.rbg_ctx_to_bitset(eng._ctx, b, 0, f, n, L.RBG_BITS_BYTES, ctypes.c_void_p(hm.ctypes.data + 128)))
            assert (hm[128:128 + n] == bits).all() and (hm[:128] == 255).all() and (hm[128 + n:] == 255).all()
            assert (eng.to_mask(b, first=f, n=n) == bits.astype(bool)).all()


def test_negative_bits_and_default_lengths(eng, mix):
    import roaringbitmap_amd as rb
    loaded, _, v, _ = mix
    with pytest.raises(rb.IllegalArgumentException, match="bitmap has negative bits set"):
        eng.to_words(loaded)  # the last value is at least 2^31: toLongArray refuses (:72-75)
    assert eng.to_mask(loaded, first=int(v[-1]) - 9).tolist() == _bits(v, int(v[-1]) - 9, 10).astype(bool).tolist()
    for last, n in ((0, 2), (63, 2), (64, 2), (127, 2), (128, 3), (65535, 1024), (65536, 1025)):
        b = eng.from_values([last])
        w = eng.to_words(b)
        assert w.size == n and int(w[last >> 6]) == 1 << (last & 63) and np.count_nonzero(w) == 1, last
        assert eng.to_mask(b).size == last + 1 and eng.to_words(b, first_word=1).size == n - 1
        eng.release(b)


def test_empty_bitmap(eng, dev):
    import torch
    e = eng.from_words(np.zeros(5000, dtype=np.uint64))
    assert eng.batch_stats(e)["containers"] == 0
    assert eng.to_words(e).shape == (0,) and eng.to_mask(e).shape == (0,)
    assert eng.to_words(e, dtype=torch.int64).numel() == 0 and eng.to_mask(e, dtype=torch.bool).numel() == 0
    assert not eng.to_words(e, first_word=1000, n_words=3000).any()
    m = eng.to_mask(e, first=77, n=100001, dtype=torch.bool)
    assert m.dtype == torch.bool and m.numel() == 100001 and int(m.sum()) == 0
    eng.release(e)


def test_torch_outputs(eng, dev, mix):
    import torch
    loaded, _, v, _ = mix
    low = 23 << 16
    m = eng.to_mask(loaded, n=low, dtype=torch.bool)
    total = int(m.sum())  # on the current stream right away
    assert m.dtype == torch.bool and m.device.type == "cuda" and total == int(np.searchsorted(v, low))
    idx = torch.nonzero(m).flatten()
    assert (idx.cpu().numpy() == v[:total]).all()
    w = eng.to_words(loaded, n_words=low >> 6, dtype=torch.int64)
    back = eng.from_words(w)
    assert (eng.to_values(back) == v[:total].astype(np.uint32)).all()
    eng.release(back)
    with pytest.raises(ValueError):
        eng.to_words(loaded, n_words=4, dtype=torch.int32)
    with pytest.raises(ValueError):
        eng.to_mask(loaded, n=4, dtype=torch.uint8)


# ---- round trips, refusals, one-shots --------------------------------------------------------------------------

def test_round_trips(eng, dev):
    import torch
    rng = np.random.default_rng(12)
    buf = _gen.bitmap(rng, np.arange(3, 15), p_present=1.0)
    assert O.stats(buf)["run"] > 0
    b = eng.load([buf])
    want = O.remove_run_compression(buf)
    assert _fetch(eng, eng.from_words(eng.to_words(b))) == want
    assert _fetch(eng, eng.from_words(eng.to_words(b, dtype=torch.int64))) == want
    assert _fetch(eng, eng.from_mask(eng.to_mask(b, dtype=torch.bool))) == want
    eng.release(b)
    m = torch.from_numpy(rng.random(1 << 20) < 0.37).to(dev)
    b = eng.from_mask(m)
    back = eng.to_mask(b, n=1 << 20, dtype=torch.bool)
    assert bool(torch.equal(back, m))
    eng.release(b)


def test_refusals_leak_nothing(eng, dev):
    import torch
    import roaringbitmap_amd as rb
    rng = np.random.default_rng(8)
    bufs = [_gen.bitmap(rng, np.arange(4), p_present=1.0), _gen.bitmap(rng, np.arange(2, 6), p_present=1.0)]
    packed = eng.load([O.from_values(np.arange(0, 3 << 16, 97, dtype=np.uint32))], packed=True)
    two = eng.load(bufs)
    one = eng.load([bufs[0]])
    probe = eng.from_values([1])
    eng.release(probe)
    bad = rb.IllegalArgumentException
    for f in (eng.to_words, eng.to_mask):
        with pytest.raises(bad, match="slot-aligned"):
            f(packed, 0, 0, 64)
        with pytest.raises(bad):
            f(two, 0, 0, 64)
        with pytest.raises(bad):
            f(one, 1, 0, 64)
        with pytest.raises(bad):
            f(12345, 0, 0, 64)  # no such batch
    with pytest.raises(bad, match="past 2\\^32"):
        eng.to_words(one, first_word=(1 << 26) - 1, n_words=2)
    with pytest.raises(bad, match="past 2\\^32"):
        eng.to_mask(one, first=(1 << 32) - 3, n=4, dtype=torch.bool)
    from roaringbitmap_amd import _lib as L
    out = ctypes.c_int32(-7)
    t = torch.zeros(64, dtype=torch.int64, device=dev)
    lib = L.lib()
    assert lib.rbg_ctx_to_bitset_device(eng._ctx, one, 0, 32, 64, L.RBG_BITS_PACKED, ctypes.c_void_p(t.data_ptr())) \
        == L.RBG_ERR_ILLEGAL_ARGUMENT and "multiple of 64" in lib.rbg_last_error().decode()
    assert lib.rbg_ctx_from_bitset_device(eng._ctx, ctypes.c_void_p(t.data_ptr() + 4), 16, L.RBG_BITS_PACKED, 0,
                                          ctypes.byref(out)) == L.RBG_ERR_ILLEGAL_ARGUMENT
    assert "8-byte aligned" in lib.rbg_last_error().decode()
    assert lib.rbg_ctx_from_bitset_device(eng._ctx, ctypes.c_void_p(t.data_ptr()), 16, 3, 0, ctypes.byref(out)) \
        == L.RBG_ERR_ILLEGAL_ARGUMENT and out.value == -7
    with pytest.raises(ValueError):
        eng.from_words(torch.zeros(4, dtype=torch.int32, device=dev))
    with pytest.raises(ValueError):
        eng.from_words(np.zeros(4, dtype=np.float64))
    again = eng.from_values([1])
    eng.release(again)
    assert again == probe  # no refusal left a batch behind
    # the engine works as before
    w = eng.to_words(one)
    assert _fetch(eng, eng.from_words(w)) == O.remove_run_compression(bufs[0])
    for b in (packed, two, one):
        eng.release(b)


def test_one_shots(gpu):
    import roaringbitmap_amd as rb
    BU = rb.BitSetUtil
    rng = np.random.default_rng(3)
    bits = (rng.random(5 << 16) < np.repeat([0.001, 0.05, 0.0626, 0.5, 0.99], 1 << 16)).astype(np.uint8)
    bits[-64 * 300:] = 0  # a short last block
    words = _words(bits)[:-300]
    for ro in (False, True):
        host = BU.bitmapOf(words, run_optimize=ro).serialize()
        assert BU.bitmapOf(words, run_optimize=ro, gpu=True).serialize() == host
        assert BU.bitmapOf(words.tobytes()[:-3], run_optimize=ro, gpu=True).serialize() \
            == BU.bitmapOf(words.tobytes()[:-3], run_optimize=ro).serialize()
    assert BU.bitmapOf(b"", gpu=True).serialize() == rb.RoaringBitmap().serialize()
    buf = _gen.bitmap(rng, np.concatenate([np.arange(5), [40, 300]]), p_present=1.0)
    x = rb.RoaringBitmap(buf)
    got = BU.toLongArray(x, gpu=True)
    assert got.dtype == np.uint64 and (got == BU.toLongArray(x)).all() and got.size == BU.wordsInUse(x.toArray()[-1])
    assert BU.toByteArray(x, gpu=True) == BU.toByteArray(x)
    assert BU.toLongArray(rb.RoaringBitmap(), gpu=True).shape == (0,)
    for last in (0, 63, 64, 128):
        assert BU.toLongArray(rb.RoaringBitmap.from_values([last]), gpu=True).size == BU.wordsInUse(last)
    with pytest.raises(rb.IllegalArgumentException, match="bitmap has negative bits set"):
        BU.toLongArray(rb.RoaringBitmap.from_values([7, 1 << 31]), gpu=True)
