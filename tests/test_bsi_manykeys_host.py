"""The inputs of tests/test_gpu_bsi_manykeys.py and tests/test_gpu_resident_manykeys.py, pinned on the CPU so
that the GPU tests cannot pass vacuously.

The bit-sliced index kernels (csrc/bsi.hip) change behaviour at sizes that an index of a few dozen keys never
reaches: k_bsi_types stages 64 keys per workgroup and picks one of 16 sum replicas by workgroup (they wrap
past 1,024 keys), k_bsi_reg hands out 4 units per key from per-group claim counters once the units exceed
the resident grid, k_bsi_defer / k_bsi / k_bsi_buf / k_bsi_owen_pre stride over keys by their grid, the plan
adds up 256-key plan workgroups, and result records leave the first 64-record tile.  _gen.sparse_bsi builds
an index past all of them; this file asserts that it does (deferred keys counted from the oracle's results),
and that the oracle's results for every query the GPU file runs agree, as sets, with plain numpy on
(columns, values).  The numpy restatements follow the reference's behaviour, quirks included:
  heap (RoaringBitmapSliceIndex.oNeilCompare): only EQ is intersected with the found set for LE and GE, so
  the result is (strict part over all columns) | (equal part & found); RANGE is the AND of two such halves;
  the circuit reads only the index's bitCount() low bits of the predicate.
  buffer (BitSliceIndexBase): rangeEQ starts from and(ebM, found); NEQ is andNot(ebM, rangeEQ) -- ebM, not
  the found set -- and ebM itself when rangeEQ's own min/max check answers "empty"; owenGreatEqual's result
  is intersected with the found set, and it has no input at all (the empty bitmap) for start - 1 == -1.
"""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import _bsi
import _gen
import _oracle as O
import test_manykeys_host as MK
from _fmt import A, B, R, container_table

SEEDS = (0xB501, 0xB502)
N_KEYS, NBITS = 6000, 20
RESIDENT_WORKGROUPS = 2048  # 256 CUs x 32 waves / 4: no kernel of 256 threads holds more workgroups at once
CIRCUIT_OPS = ("LT", "GT", "GE", "RANGE")


def vals64(buf):
    return O.to_values(buf).astype(np.int64)


@functools.lru_cache(maxsize=None)
def inputs(seed, run_optimize):
    """Everything the many-key BSI tests run on, built once per (seed, run_optimize) and never modified."""
    rng = np.random.default_rng(seed)
    keys, cols, vals = _gen.sparse_bsi(rng, N_KEYS, NBITS)
    heap = _bsi.BSI.from_columns(cols, vals, run_optimize)
    buf = _bsi.BufferBSI.from_columns(cols, vals, run_optimize)
    heap.memo, buf.memo = {}, {}  # the chains depend on the predicate alone: one pass serves every op and found set
    fsel = np.zeros(cols.size, dtype=bool)
    fsel[rng.choice(cols.size, cols.size // 3, replace=False)] = True
    found = O.from_values(cols[fsel], run_optimize)
    lo, hi = int(vals.min()), int(vals.max())
    med = int(np.median(vals))
    uniq, cnt = np.unique(vals, return_counts=True)
    freq = int(uniq[np.argmax(cnt)])
    single = int(uniq[cnt == 1][len(uniq[cnt == 1]) // 2])
    # (name, start or value, end): every op takes every predicate; RANGE reads both numbers, the others the first
    preds = [("median", med, med + med // 2),
             ("around_median", med // 2, 3 * med // 2),
             ("frequent", freq, freq + 3),
             ("single", single, single),
             ("zero", 0, 0),
             ("max", hi, hi),
             ("narrow", med - 2, med + 2),
             ("whole", lo, hi),          # GE and RANGE: compareUsingMinMax answers "all"; LT: "empty"
             ("above_max", hi + 1, hi + 5),  # LT and LE: "all"; GT, GE, EQ and RANGE: "empty"
             ("below_min", lo - 1, lo - 1)]  # GT and GE: "all"; LT, LE, EQ and RANGE: "empty"
    return SimpleNamespace(seed=seed, run_optimize=run_optimize, keys=keys, cols=cols, vals=vals, heap=heap, buf=buf,
                           found=found, fsel=fsel, lo=lo, hi=hi, med=med, freq=freq, single=single, preds=preds,
                           nbits=heap.bit_count(), hole=_gen.empty_workgroup(keys))


@functools.lru_cache(maxsize=None)
def expected(seed, run_optimize, package):
    """The oracle's bytes for every (op, predicate, found set or none) of one index, computed once:
    {(op, predicate name, with found): bytes}; package "heap" or "buffer" (op "NEQ_DIRECT" = rangeNEQ)."""
    s = inputs(seed, run_optimize)
    o = s.heap if package == "heap" else s.buf
    out = {}
    for name, a, e in s.preds:
        for wf in (False, True):
            f = s.found if wf else None
            for op in _bsi.OPS:
                out[op, name, wf] = o.compare(op, a, e, f)
            if package == "buffer":
                out["NEQ_DIRECT", name, wf] = o._andnot(o.ebm, o.range_eq(f, a))
    return out


# ---- plain numpy restatements over (columns, values): masks over s.cols -----------------------------------
def minmax(op, a, e, lo, hi):
    """compareUsingMinMax: "all", "empty" or None (run the circuit)"""
    if op == "LT":
        return "all" if a > hi else "empty" if a <= lo else None
    if op == "LE":
        return "all" if a >= hi else "empty" if a < lo else None
    if op == "GT":
        return "all" if a < lo else "empty" if a >= hi else None
    if op == "GE":
        return "all" if a <= lo else "empty" if a > hi else None
    if op == "EQ":
        return "all" if lo == hi == a else "empty" if (a < lo or a > hi) else None
    if op == "NEQ":
        return None if lo != hi else "empty" if lo == a else "all"
    return "all" if (a <= lo and e >= hi) else "empty" if (a > hi or e < lo) else None


def np_compare(s, package, op, a, e, with_found):
    """-> the columns of the reference's result, ascending"""
    v = s.vals
    inf = s.fsel if with_found else np.ones(v.size, dtype=bool)
    none = np.zeros(v.size, dtype=bool)
    bits = (1 << s.nbits) - 1  # the circuits read bitCount() bits of the predicate
    if op == "NEQ_DIRECT":
        mm = None
    else:
        mm = minmax(op, a, e, s.lo, s.hi)
    if mm == "all":
        return s.cols[inf]
    if mm == "empty":
        return s.cols[none]

    def half(hop, p):  # oNeilCompare's LE / GE: only the equal part meets the found set
        p &= bits
        strict = v < p if hop == "LE" else v > p
        return strict | ((v == p) & inf)

    if package == "heap":
        p = a & bits
        m = {"EQ": lambda: (v == p) & inf, "NEQ": lambda: (v != p) & inf, "LT": lambda: (v < p) & inf,
             "GT": lambda: (v > p) & inf, "LE": lambda: half("LE", a), "GE": lambda: half("GE", a),
             "RANGE": lambda: half("GE", a) & half("LE", e)}[op]()
        return s.cols[m]

    def owen_ge(p):  # v > p - 1 over the found set; no orInput at all for p - 1 == -1
        if p - 1 == -1:
            return none
        assert 0 <= p - 1 <= bits
        return (v >= p) & inf

    p = a & bits
    if op in ("NEQ", "NEQ_DIRECT"):  # andNot(ebM, rangeEQ(found, a)); rangeEQ checks min / max itself
        eq = none if minmax("EQ", a, 0, s.lo, s.hi) == "empty" else (v == p) & inf
        return s.cols[~eq]
    m = {"EQ": lambda: (v == p) & inf, "LT": lambda: (v < p) & inf, "GT": lambda: (v > p) & inf,
         "LE": lambda: half("LE", a), "GE": lambda: owen_ge(a), "RANGE": lambda: owen_ge(a) & half("LE", e)}[op]()
    return s.cols[m]


def np_sum(s, mask):
    return int(s.vals[mask].sum()), int(mask.sum())


# ---- which containers of a result the kernels had to compute ------------------------------------------------
def _mix(x):
    x = x.astype(np.uint64) + np.uint64(0x9E3779B97F4A7C15)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def fingerprints(buf):
    """per key (65,536 entries) a fingerprint of the container's value set, 0 where there is none"""
    v = O.to_values(buf)
    fp = np.zeros(65536, dtype=np.uint64)
    if v.size:
        k = (v >> 16).astype(np.int64)  # ascending, as the values are
        first = np.concatenate([[0], np.nonzero(np.diff(k))[0] + 1])
        with np.errstate(over="ignore"):
            fp[k[first]] = np.add.reduceat(_mix(v) | np.uint64(1), first)
    return fp


@functools.lru_cache(maxsize=None)
def input_fingerprints(seed, run_optimize):
    s = inputs(seed, run_optimize)
    return np.stack([fingerprints(b) for b in [s.heap.ebm] + s.heap.ba + [s.found]])


def computed(s, result, kind):
    """how many containers of `kind` in `result` hold a value set that no input container under the same
    key holds (ebM, the slices, the found set): such a container cannot be a clone, the kernels built it"""
    keys, kinds, _, _, _ = container_table(result)
    fp = fingerprints(result)
    clone = np.any(input_fingerprints(s.seed, s.run_optimize) == fp[None, :], axis=0)
    return int(np.sum(~clone[keys[kinds == kind]]))


CASES = [(seed, ro) for seed in SEEDS for ro in (False, True)]
IDS = [f"seed{seed:x}-{'ro' if ro else 'plain'}" for seed, ro in CASES]


# ---- the inputs ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,ro", CASES, ids=IDS)
def test_index_shape(seed, ro):
    s = inputs(seed, ro)
    keys = s.keys
    assert 4096 < N_KEYS <= keys.size < N_KEYS + 5 and s.nbits == NBITS and s.lo == 0 and s.hi >> (NBITS - 1) == 1
    assert np.array_equal(keys[:300], np.arange(300)) and keys[-2] == 65534 and keys[-1] == 65535
    g = s.hole
    assert g is not None and not np.any((keys >> 8) == g)
    assert np.any(keys < 256 * g) and np.any(keys >= 256 * (g + 1))
    assert np.array_equal(s.cols, np.unique(s.cols)) and np.array_equal(np.unique(s.cols >> 16), keys)
    ek, ekind, ecard, _, elen = container_table(s.heap.ebm)
    assert np.array_equal(ek, keys)
    # arrays, bitmaps, and run containers above 2,047 runs or full ones on late keys
    assert np.any(ekind == A) and np.any(ekind[1024:] == B)
    absent = 0
    for b in s.heap.ba:
        absent += int(np.setdiff1d(keys, container_table(b)[0]).size)
    assert absent > 1000  # slices without a container under a key that ebM holds
    assert len(container_table(s.heap.ba[NBITS - 1])[0]) < keys.size
    if ro:
        assert int(np.sum(ekind == R)) > 1500
        assert np.any((ekind == R) & (elen > 2 + 4 * 2047)) or np.any((ekind == R) & (ecard == 65536))
        for b in s.heap.ba[:4]:
            assert int(np.sum(container_table(b)[1] == R)) > 100
    else:
        assert not np.any(ekind == R)
    fv = vals64(s.found)
    assert fv.size == s.cols.size // 3 and np.array_equal(fv, s.cols[s.fsel])
    assert (s.buf.ebm, s.buf.ba, s.buf.min, s.buf.max) == (s.heap.ebm, s.heap.ba, s.lo, s.hi)


@pytest.mark.parametrize("seed,ro", CASES, ids=IDS)
def test_predicates(seed, ro):
    s = inputs(seed, ro)
    p = {name: (a, e) for name, a, e in s.preds}
    assert int(np.sum(s.vals == s.single)) == 1 and int(np.sum(s.vals == s.freq)) > 1000
    assert s.lo < p["median"][0] < s.hi and 0 < p["narrow"][1] - p["narrow"][0] < 8
    got = {(op, name): minmax(op, a, e, s.lo, s.hi) for name, a, e in s.preds for op in _bsi.OPS}
    for op in ("LT", "LE", "GT", "GE", "RANGE"):  # "all" and "empty" for every op that has the shortcut
        assert {"all", "empty"} <= {got[op, name] for name in p}, op
    assert "empty" in {got["EQ", name] for name in p}
    for name in ("median", "around_median", "frequent", "single", "narrow"):
        assert all(got[op, name] is None for op in _bsi.OPS), name
    # owenGreatEqual with three or more orInputs (the host's replay of horizontal_or's queue)
    for name in ("median", "around_median", "narrow"):
        assert len(s.buf.owen_inputs(p[name][0])) >= 3, name


@pytest.mark.parametrize("seed,ro", CASES, ids=IDS)
def test_deferred_keys_exceed_the_resident_grid(seed, ro):
    """array and run results that the kernels build from the scratch bits (k_bsi_defer), more of them than
    any kernel has resident workgroups; with run-optimized inputs, results whose type needs a run count"""
    s = inputs(seed, ro)
    ex = expected(seed, ro, "heap")
    over, runs = 0, 0
    for op in CIRCUIT_OPS:
        res = ex[op, "median", False]
        n_a, n_r = computed(s, res, A), computed(s, res, R)
        over += n_a + n_r > RESIDENT_WORKGROUPS
        if op != "RANGE":
            runs += n_r >= 100
    assert over >= 3
    if ro:
        assert runs == 3


@pytest.mark.parametrize("seed,ro", CASES, ids=IDS)
@pytest.mark.parametrize("package", ["heap", "buffer"])
def test_results_are_not_trivial(seed, ro, package):
    s = inputs(seed, ro)
    ex = expected(seed, ro, package)
    bitmaps = 0
    for op in _bsi.OPS:
        good = 0
        for name, _, _ in s.preds:
            res = ex[op, name, False]
            st = O.stats(res)
            good += st["card"] > 0 and res != s.heap.ebm
            bitmaps += st["bitmap"]
        assert good >= 1, op
    assert bitmaps > 0
    assert len(container_table(ex["GT", "median", False])[0]) > 2048  # result records far past the first tile


# ---- the oracle against numpy, on the cases the GPU file runs -----------------------------------------------
@pytest.mark.parametrize("seed,ro", CASES, ids=IDS)
@pytest.mark.parametrize("package", ["heap", "buffer"])
def test_oracle_compare_sets(seed, ro, package):
    s = inputs(seed, ro)
    for (op, name, wf), res in expected(seed, ro, package).items():
        a, e = next((a, e) for n, a, e in s.preds if n == name)
        want = np_compare(s, package, op, a, e, wf)
        assert np.array_equal(vals64(res), want), (package, op, name, a, e, wf)


@pytest.mark.parametrize("seed,ro", CASES, ids=IDS)
def test_oracle_sums(seed, ro):
    s = inputs(seed, ro)
    assert s.heap.sum(s.found) == s.buf.sum(s.found) == np_sum(s, s.fsel)
    ex = expected(seed, ro, "heap")
    for op, name in (("RANGE", "around_median"), ("GT", "median"), ("EQ", "frequent"), ("LE", "narrow")):
        res = ex[op, name, True]
        assert s.heap.sum(res) == np_sum(s, np.isin(s.cols, vals64(res))), (op, name)


# ---- the resident-bitmap queries (tests/test_gpu_resident_manykeys.py) --------------------------------------
@functools.lru_cache(maxsize=None)
def resident_input(seed):
    """The bitmap of test_manykeys_host.inputs(seed) that the resident-query tests run on: the first of x, xr,
    y, z with a bitmap container and a run container of more than 64 runs at container index 8,192 or
    above, where a wave of k_rd_fill and of a full k_to_values expansion takes its second container.
    -> (name, bytes, values, index of that bitmap container, index of that run container)"""
    s = MK.inputs(seed)
    for name in ("x", "xr", "y", "z"):
        buf = getattr(s, name)
        _, kinds, _, _, lens = container_table(buf)
        late = np.arange(kinds.size) >= MK.RESIDENT_WAVES
        ib, ir = np.nonzero(late & (kinds == B))[0], np.nonzero(late & (kinds == R) & (lens > 2 + 4 * 64))[0]
        if ib.size and ir.size:
            return name, buf, MK.vals(buf), int(ib[0]), int(ir[0])
    raise AssertionError("no bitmap of the many-key inputs has a late bitmap and a late long-run container")


def short_window_heavies(seed):
    """{kind: container index} for bitmap and run: the first container of that kind in the dense middle block
    with more than 300 values that follows five containers of at most 16 values, so that a window of 256
    values or fewer spans those five and reaches into it"""
    s = MK.inputs(seed)
    keys, kinds, cards, _, _ = container_table(resident_input(seed)[1])
    inmid = (keys >= s.mid) & (keys < s.mid + s.mid_len)
    out = {}
    for h in np.nonzero(inmid & (kinds != A) & (cards > 300))[0]:
        h = int(h)
        if int(kinds[h]) not in out and inmid[h - 5] and cards[h - 5:h].max() <= 16:
            out[int(kinds[h])] = h
    return out


@pytest.mark.parametrize("seed", MK.SEEDS)
def test_resident_input(seed):
    assert set(short_window_heavies(seed)) == {B, R}
    name, buf, v, ib, ir = resident_input(seed)
    keys, kinds, cards, _, lens = container_table(buf)
    assert keys.size > MK.RESIDENT_WAVES and v.size == int(cards.sum())
    assert ib >= MK.RESIDENT_WAVES and kinds[ib] == B and cards[ib] > 4096
    assert ir >= MK.RESIDENT_WAVES and kinds[ir] == R and (lens[ir] - 2) // 4 > 64
    assert MK.inputs(seed).hole is not None
