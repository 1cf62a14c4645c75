"""The inputs of tests/test_gpu_manykeys.py, pinned on the CPU so that the GPU tests cannot pass vacuously.

The per-key kernels outside the pairwise family (addoffset.hip, rangemut.hip, the range selections, the
in-place and buffer pairwise paths, contains) change behaviour at three sizes that a bitmap of a few
dozen containers never reaches: the 64-record result tile, the 256-key plan workgroup (plan_emit,
wave.hpp) and the 8,192 waves an MI355X holds at once (256 CUs x 32), above which a wave of a
one-wave-per-task kernel takes a second task.  _gen.sparse_keys / sparse_bitmap build inputs past all
three with gaps in the key list; this file asserts that they do, and that the oracle's results for every
op the GPU file runs agree, as sets, with plain numpy set arithmetic on the decoded values.
"""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import _gen
import _oracle as O
from _fmt import A, B, R, container_table, decode, encode

SEEDS = (0x5A01, 0x5A02)
OFFSETS = [300, -300, 65536 - 300, (3 << 16) + 64, -(2 << 16) - 1, 1, 65535, (1 << 32) - 1]
RESIDENT_WAVES = 8192  # 256 CUs x 32 waves
U32 = 1 << 32


def vals(buf):
    return O.to_values(buf).astype(np.int64)


def perturbed(rng, buf):
    """A bitmap over most of buf's keys: a tenth of the keys dropped (65534 and 65535 kept), of the rest a
    third identical containers, a third with a few tiny values more, a third fresh tiny arrays."""
    out = []
    for key, kind, card, v, _ in decode(buf):
        r = rng.random()
        if r < 0.1 and key < 65534:
            continue
        if r < 0.4:
            out.append((key, kind, v))
        elif r < 0.7:
            u = np.union1d(v, _gen.tiny_values(rng, rng.random())).astype(np.uint16)
            out.append((key, B if kind == A and u.size > 4096 else kind, u))
        else:
            out.append((key, A, _gen.tiny_values(rng, rng.random())))
    return encode(out)


@functools.lru_cache(maxsize=None)
def inputs(seed):
    """Everything the many-key tests run on, built once per seed and never modified."""
    rng = np.random.default_rng(seed)
    keys = _gen.sparse_keys(rng)
    x = _gen.sparse_bitmap(rng, keys)
    xr = _gen.sparse_bitmap(np.random.default_rng(seed + 100), keys, run_every=3)
    y = perturbed(np.random.default_rng(seed + 200), x)
    z = perturbed(np.random.default_rng(seed + 300), x)
    g = _gen.empty_workgroup(keys)
    have = np.zeros(65537, dtype=bool)
    have[keys] = True
    # the dense middle block: the longest run of adjacent keys that does not start at key 0
    brk = np.nonzero(np.diff(keys) != 1)[0]
    starts, ends = np.concatenate([[0], brk + 1]), np.concatenate([brk, [keys.size - 1]])
    i = int(np.argmax(np.where(keys[starts] > 0, ends - starts, -1)))
    mid, mid_len = int(keys[starts[i]]), int(ends[i] - starts[i] + 1)
    a1 = int(np.nonzero(~have[1100:])[0][0]) + 1100  # an absent key above the dense head and the hole
    a2 = int(np.nonzero(~have[a1 + 200:])[0][0]) + a1 + 200
    ranges = {"absent": ((a1 << 16) + 1234, (a2 << 16) + 4321),
              "mid_to_end": (((mid + 1000) << 16) + 1500, U32),
              "all": (0, U32),
              "hole": ((256 * g) << 16, (256 * (g + 1)) << 16)}
    cards = container_table(x)[2]
    cum = np.cumsum(cards)
    heavy = next(i for i in range(RESIDENT_WAVES, keys.size) if i % 97 == 96 and cards[i] > 100)
    limits = {"first": int(cards[0] + 1) // 2,
              "heavy_late": int(cum[heavy - 1]) + max(1, int(cards[heavy]) // 2),
              "last": int(cum[-2]) + int(cards[-1] + 1) // 2,
              "card": int(cum[-1]),
              "card_plus_1": int(cum[-1]) + 1}
    vx = vals(x)
    late = vx >= (int(keys[8500]) << 16)
    sub = vx[~late | (rng.random(vx.size) < 0.5)]
    free = np.setdiff1d(np.arange(65535 << 16, U32, dtype=np.int64), vx)
    non = np.union1d(vx, free[:1])
    return SimpleNamespace(seed=seed, keys=keys, x=x, xr=xr, y=y, z=z, hole=g, mid=mid, mid_len=mid_len,
                           ranges=ranges, limits=limits, heavy=heavy, vx=vx, sub=O.from_values(sub),
                           non=O.from_values(non), sub_dist=int(vx.size - sub.size),
                           ornot_end=((256 * g + 100) << 16) + 777)


# ---- plain numpy restatements of the ops (sets of int64 values; no container logic) ------------------
def np_add_offset(v, off):
    w = v + off
    return w[(w >= 0) & (w < U32)]


def np_select(v, st, en):
    return v[(v >= st) & (v < en)]


def np_range_mut(op, v, st, en):
    if op == "remove":
        return v[(v < st) | (v >= en)]
    r = np.arange(st, en, dtype=np.int64)
    return np.union1d(v, r) if op == "add" else np.setxor1d(v, r)


def np_range_op(op, vs, st, en):
    sel = [np_select(v, st, en) for v in vs]
    if op == "andnot":
        return np.setdiff1d(sel[0], sel[1])
    f = {"and": np.intersect1d, "or": np.union1d, "xor": np.setxor1d}[op]
    return functools.reduce(f, sel)


def np_pair(op, a, b):
    return {"and": np.intersect1d, "or": np.union1d, "xor": np.setxor1d, "andnot": np.setdiff1d}[op](a, b)


def ornot_mask(va, vb, end):
    """membership mask over [0, end) of va | ([0, end) \\ vb)"""
    want = np.ones(end, dtype=bool)
    want[vb[vb < end]] = False
    want[va[va < end]] = True
    return want


def ornot_agrees(got, va, want, end):
    """got == va | ([0, end) \\ vb) as sets: want = ornot_mask(va, vb, end) below end, va's values from end on"""
    have = np.zeros(end, dtype=bool)
    have[got[got < end]] = True
    return bool(np.array_equal(have, want)) and bool(np.array_equal(got[got >= end], va[va >= end]))


# ---- the inputs ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
def test_key_skeleton(seed):
    s = inputs(seed)
    keys = s.keys
    assert 9000 <= keys.size <= 10000 and keys.size > RESIDENT_WAVES
    assert np.array_equal(keys, np.unique(keys)) and keys[0] == 0
    assert np.array_equal(keys[:300], np.arange(300))
    assert keys[-2] == 65534 and keys[-1] == 65535
    assert s.mid_len >= 6000 and 20000 < s.mid < 40000
    # one whole plan workgroup without a key, keys in workgroups on both sides, >= 300 empty keys around it
    g = s.hole
    assert g is not None and not np.any((keys >> 8) == g)
    below, above = keys[keys < 256 * g], keys[keys >= 256 * (g + 1)]
    assert below.size and above.size and int(above[0]) - int(below[-1]) - 1 >= 300
    # blocks of 1, 2, 3 and 5 adjacent keys
    brk = np.nonzero(np.diff(keys) != 1)[0]
    lens = np.diff(np.concatenate([[-1], brk, [keys.size - 1]]))
    assert {1, 2, 3, 5} <= set(lens.tolist())
    for b in (s.x, s.xr, s.y, s.z):
        assert len(b) < 2_000_000
    assert len(container_table(s.y)[0]) > RESIDENT_WAVES and len(container_table(s.z)[0]) > RESIDENT_WAVES


@pytest.mark.parametrize("seed", SEEDS)
def test_container_mix(seed):
    s = inputs(seed)
    keys, kinds, cards, _, lens = container_table(s.x)
    assert np.array_equal(keys, s.keys)
    tiny = np.ones(keys.size, dtype=bool)
    tiny[96::97] = False
    assert np.all(kinds[tiny] == A) and cards[tiny].min() >= 1 and cards[tiny].max() <= 8
    dec = decode(s.x)
    low = np.array([c[3].max() < 2000 for c in dec])[tiny]
    high = np.array([c[3].min() >= 63000 for c in dec])[tiny]
    for part in (low, high, ~low & ~high):
        assert 0.25 < part.mean() < 0.42
    # heavy containers of every kind on late tasks: a bitmap and a run container past the 8,192nd, and a
    # run container above 2,047 runs and a full one past the first 256 records
    assert s.heavy >= RESIDENT_WAVES and not tiny[s.heavy]
    late = np.arange(keys.size) >= RESIDENT_WAVES
    assert np.any(late & (kinds == B)) and np.any(late & (kinds == R))
    assert np.any((kinds[256:] == R) & (lens[256:] > 2 + 4 * 2047))
    assert np.any(cards[256:] == 65536)
    # the run variant: thousands of one- and two-run containers for removeRunCompression
    kr, kindr, _, _, lenr = container_table(s.xr)
    assert np.array_equal(kr, s.keys)
    assert int(np.sum((kindr == R) & (lenr <= 10))) > 3000
    assert np.any(late & (kindr == R) & (lenr <= 10))
    # limit's cuts: inside the first container, a heavy one past task 8,192, the last one
    cum = np.cumsum(cards)
    assert 0 < s.limits["first"] <= cards[0]
    assert cum[s.heavy - 1] < s.limits["heavy_late"] < cum[s.heavy] and cards[s.heavy] > 100
    assert cum[-2] < s.limits["last"] <= cum[-1] == s.limits["card"] < (1 << 31) - 1


@pytest.mark.parametrize("seed", SEEDS)
def test_ranges(seed):
    s = inputs(seed)
    have = np.zeros(65536, dtype=bool)
    have[s.keys] = True
    st, en = s.ranges["absent"]
    assert not have[st >> 16] and not have[(en - 1) >> 16] and have[st >> 16:en >> 16].sum() >= 3
    st, en = s.ranges["mid_to_end"]
    assert s.mid < st >> 16 < s.mid + s.mid_len - 1 and en == U32
    assert int(np.sum(s.keys > st >> 16)) > 4000  # ADD_INPLACE's keys between the first and the last
    st, en = s.ranges["hole"]
    assert st >> 16 == 256 * s.hole and en >> 16 == 256 * (s.hole + 1) and not have[st >> 16:en >> 16].any()
    assert (s.ornot_end >> 16) >> 8 == s.hole


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("off", [300, -300])
def test_add_offset_task_counts(seed, off):
    """more result containers than resident waves; output keys fed by one input container and by two"""
    s = inputs(seed)
    res = O.add_offset(s.x, off)
    assert len(container_table(res)[0]) > RESIDENT_WAVES
    w = s.vx + off
    ok = (w >= 0) & (w < U32)
    pairs = np.unique(((w[ok] >> 16) << 16) | (s.vx[ok] >> 16))
    feeds = np.bincount(pairs >> 16, minlength=65536)
    assert set(np.unique(feeds).tolist()) <= {0, 1, 2}
    assert int(np.sum(feeds == 1)) >= 100 and int(np.sum(feeds == 2)) >= 100
    # output keys with an input container at k - co or k - co - 1 (the kernel's tasks), and those of them
    # that stay empty because the one part that reaches them holds no value
    task = np.zeros(65536, dtype=bool)
    for d in (off // 65536, off // 65536 + 1):
        k = s.keys + d
        task[k[(k >= 0) & (k < 65536)]] = True
    assert int(task.sum()) > RESIDENT_WAVES and not np.any(~task & (feeds > 0))
    assert int(np.sum(task & (feeds == 0))) >= 100


@pytest.mark.parametrize("seed", SEEDS)
def test_subset_inputs(seed):
    s = inputs(seed)
    vs, vn = vals(s.sub), vals(s.non)
    assert s.sub_dist > 100 and vs.size + s.sub_dist == s.vx.size and np.isin(vs, s.vx).all()
    dropped = np.setdiff1d(s.vx, vs)
    assert dropped.min() >> 16 >= s.keys[8500]  # late keys only
    extra = np.setxor1d(vn, s.vx)
    assert extra.size == 1 and extra[0] >> 16 == 65535 and vn.size == s.vx.size + 1


# ---- the oracle against numpy, on the cases the GPU file runs ------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
def test_oracle_add_offset_sets(seed):
    s = inputs(seed)
    for off in OFFSETS:
        assert np.array_equal(vals(O.add_offset(s.x, off)), np_add_offset(s.vx, off)), off


@pytest.mark.parametrize("seed", SEEDS)
def test_oracle_range_mut_sets(seed):
    s = inputs(seed)
    st, en = s.ranges["absent"]
    for op in ("add", "remove", "flip"):
        want = np_range_mut(op, s.vx, st, en)
        for buffer in (False, True):
            assert np.array_equal(vals(O.range_mut(op, s.x, st, en, buffer=buffer)), want), (op, buffer)
            ip = "add_inplace" if op == "add" else op
            assert np.array_equal(vals(O.range_mut(ip, s.x, st, en, buffer=buffer)), want), (ip, buffer)
    for name in ("mid_to_end", "all", "hole"):  # remove needs no materialised range
        st, en = s.ranges[name]
        assert np.array_equal(vals(O.range_mut("remove", s.x, st, en)), np_range_mut("remove", s.vx, st, en)), name


@pytest.mark.parametrize("seed", SEEDS)
def test_oracle_derun_limit_select_sets(seed):
    s = inputs(seed)
    out = O.remove_run_compression(s.xr)
    assert np.array_equal(vals(out), vals(s.xr)) and not np.any(container_table(out)[1] == R)
    for name, n in s.limits.items():
        assert np.array_equal(vals(O.limit(s.x, n)), s.vx[:n]), name
    for name, (st, en) in s.ranges.items():
        for sel in ("select", "select_buf"):
            assert np.array_equal(vals(O.range_op(sel, [s.x], st, en)), np_select(s.vx, st, en)), (name, sel)


@pytest.mark.parametrize("seed", SEEDS)
def test_oracle_range_op_sets(seed):
    s = inputs(seed)
    bufs = [s.x, s.y, s.z]
    vs = [s.vx, vals(s.y), vals(s.z)]
    for name, (st, en) in s.ranges.items():
        for op in ("and", "or", "xor", "andnot"):
            b = bufs[:2] if op == "andnot" else bufs
            want = np_range_op(op, vs, st, en)
            assert np.array_equal(vals(O.range_op(op, b, st, en)), want), (name, op)
            assert np.array_equal(vals(O.range_op(op + "_buf", b, st, en)), want), (name, op, "buffer")
    assert np_range_op("and", vs, 0, U32).size > 1000  # the three bitmaps share containers


@pytest.mark.parametrize("seed", SEEDS)
def test_oracle_pairwise_sets(seed):
    s = inputs(seed)
    vy = vals(s.y)
    for oop, op in (("and", "and"), ("ior", "or"), ("xor", "xor"), ("andnot", "andnot"), ("and_buf", "and"),
                    ("andnot_buf", "andnot")):
        assert np.array_equal(vals(O.pairwise(oop, s.x, s.y)), np_pair(op, s.vx, vy)), oop


@pytest.mark.parametrize("seed", SEEDS)
def test_oracle_ornot_sets(seed):
    s = inputs(seed)
    want = ornot_mask(s.vx, vals(s.y), s.ornot_end)
    for inplace in (False, True):
        for buffer in (False, True):
            got = O.to_values(O.ornot(s.x, s.y, s.ornot_end, inplace=inplace, buffer=buffer))
            assert ornot_agrees(got, s.vx, want, s.ornot_end), (inplace, buffer)
