"""Many-key parity of the bit-sliced index compare / sum kernels (csrc/bsi.hip, engine_bsi.cpp ctx_bsi and
ctx_bsi_buffer), byte for byte against the oracle (tests/_bsi.py).

The small-shape files (test_gpu_bsi.py, test_gpu_bsi_buffer.py) mix every container kind on 16 keys or fewer,
and the full-size C5 test runs one op over full-run and dense bitmap containers.  Neither reaches, with
arrays, runs, absent slice containers, a found set or run-optimized inputs: k_bsi_types past its first
64-key workgroup and its 16 sum replicas wrapping (past 1,024 keys); k_bsi_reg's per-group unit pools with
more units (4 per key) than resident workgroups, and the claim counters zeroed again for the next query;
k_bsi_defer's stride loop with more deferred keys than resident workgroups (2,048 at most); the stride loops
of k_bsi (BSI_ALL, sum alone), k_bsi_buf and k_bsi_owen_pre; the plan past one 256-key plan workgroup with
an empty one in between; result records past the first 64-record tile; and the per-batch cached task list
and input table reused by dozens of queries.  The inputs are _gen.sparse_bsi: 6,000 keys, 20 slices.
tests/test_bsi_manykeys_host.py pins them, counts the deferred keys from the oracle's results, and checks
the oracle against plain numpy; one assertion per op here checks the GPU's result against numpy as well.
"""
import hashlib
from types import SimpleNamespace

import numpy as np
import pytest

import _bsi
import _oracle as O
from test_bsi_manykeys_host import CASES, IDS, expected, inputs, np_compare, np_sum, vals64

pytestmark = pytest.mark.gpu


def _same(got: bytes, exp: bytes, what):
    """bytes equality with a short message (a pytest diff of two 1 MB strings takes minutes)"""
    if got == exp:
        return
    n = min(len(got), len(exp))
    first = next((i for i in range(n) if got[i] != exp[i]), n)
    raise AssertionError(f"{what}: {len(got)} B (sha {hashlib.sha1(got).hexdigest()[:12]}) vs oracle {len(exp)} B "
                         f"(sha {hashlib.sha1(exp).hexdigest()[:12]}), first difference at byte {first}")


@pytest.fixture(scope="module")
def eng(gpu):
    import roaringbitmap_amd as rb
    e = rb.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module", params=CASES, ids=IDS)
def idx(request, eng):
    """one index resident as [ebM] + slices (.b) and once more with the found set appended (.bf)"""
    s = inputs(*request.param)
    s = SimpleNamespace(**vars(s), b=eng.load([s.heap.ebm] + s.heap.ba),
                        bf=eng.load([s.heap.ebm] + s.heap.ba + [s.found]))
    yield s
    eng.release(s.b)
    eng.release(s.bf)


def _heap(eng, s, op, a, e, wf, want_sum=False):
    eng.bsi(s.bf if wf else s.b, op, s.nbits, a, e, s.lo, s.hi, has_found=wf, want_sum=want_sum)
    return eng.fetch().serialize()


def _buffer(eng, s, op, a, e, wf):
    eng.bsi_buffer(s.bf if wf else s.b, op, s.nbits, a, e, s.lo, s.hi, has_found=wf)
    return eng.fetch().serialize()


def test_heap_compare(eng, idx):
    """every op x every predicate x {no found set, found set}, one after the other on the same two resident
    batches: the cached plan and the re-zeroed claim counters serve 140 queries"""
    s = idx
    ex = expected(s.seed, s.run_optimize, "heap")
    for wf in (False, True):
        for name, a, e in s.preds:
            for op in _bsi.OPS:
                got = _heap(eng, s, op, a, e, wf)
                _same(got, ex[op, name, wf], f"heap {op} {name} ({a}, {e}) found={wf}")
                if name == "median":
                    assert np.array_equal(vals64(got), np_compare(s, "heap", op, a, e, wf)), (op, wf, "not the numpy set")


def test_heap_sums(eng, idx):
    """want_sum fuses sum(result) (20 slices: above the kBsiCut split of the sum shares); the next query
    without it leaves (0, 0) and the same bytes; sum alone (op 8) over the found set"""
    s = idx
    ex = expected(s.seed, s.run_optimize, "heap")
    p = {name: (a, e) for name, a, e in s.preds}
    for name in ("median", "around_median", "frequent"):
        a, e = p[name]
        for op in _bsi.OPS:
            for wf in (False, True):
                exp = ex[op, name, wf]
                _same(_heap(eng, s, op, a, e, wf, want_sum=True), exp, f"heap {op} {name} found={wf} with sum")
                assert eng.bsi_sums() == s.heap.sum(exp), (op, name, wf)
                _same(_heap(eng, s, op, a, e, wf), exp, f"heap {op} {name} found={wf} after a sum")
                assert eng.bsi_sums() == (0, 0), (op, name, wf)
    a, e = p["around_median"]
    got = _heap(eng, s, "RANGE", a, e, True, want_sum=True)
    assert eng.bsi_sums() == np_sum(s, np.isin(s.cols, vals64(got)))
    want = np_sum(s, s.fsel)
    assert s.heap.sum(s.found) == want
    for _ in range(2):
        eng.bsi(s.bf, 8, s.nbits, 0, 0, s.lo, s.hi, has_found=True, want_sum=True)
        assert eng.bsi_sums() == want
        _same(_heap(eng, s, "GT", *p["median"], True), ex["GT", "median", True], "heap GT after sum alone")


def test_heap_shortcuts(eng, idx):
    """compareUsingMinMax: "all" with a found set is and(ebM, found) through the streamed BSI_ALL, "all"
    without one is ebM's clone, "empty" is the empty bitmap"""
    s = idx
    both = O.pairwise("and", s.heap.ebm, s.found)
    p = {name: (a, e) for name, a, e in s.preds}
    alls = [("LT", "above_max"), ("LE", "above_max"), ("LE", "max"), ("GT", "below_min"), ("GE", "below_min"),
            ("GE", "whole"), ("RANGE", "whole")]
    empties = [("LT", "whole"), ("LT", "below_min"), ("LE", "below_min"), ("GT", "max"), ("GT", "above_max"),
               ("GE", "above_max"), ("EQ", "above_max"), ("EQ", "below_min"), ("RANGE", "above_max"),
               ("RANGE", "below_min")]
    for op, name in alls:
        _same(_heap(eng, s, op, *p[name], True), both, f"heap {op} {name}: all & found")
        _same(_heap(eng, s, op, *p[name], False), s.heap.ebm, f"heap {op} {name}: all")
        _same(_buffer(eng, s, op, *p[name], True), s.buf._and(s.buf.ebm, s.found), f"buffer {op} {name}: all & found")
        _same(_buffer(eng, s, op, *p[name], False), s.heap.ebm, f"buffer {op} {name}: all")
    for op, name in empties:
        for wf in (False, True):
            _same(_heap(eng, s, op, *p[name], wf), _bsi.EMPTY, f"heap {op} {name}: empty")
            _same(_buffer(eng, s, op, *p[name], wf), _bsi.EMPTY, f"buffer {op} {name}: empty")
    assert np.array_equal(vals64(both), s.cols[s.fsel])


def test_two_indexes_interleaved(eng, idx):
    """the 99-column known-answer index queried between two queries of the large one, on the same engine:
    each batch keeps its own cached task list and input table"""
    s = idx
    ex = expected(s.seed, s.run_optimize, "heap")
    small = _bsi.BSI.from_columns(np.arange(1, 100), np.arange(1, 100))
    b2 = eng.load([small.ebm] + small.ba)
    p = {name: (a, e) for name, a, e in s.preds}
    for op, name, sop, sa, se, sexp in (("GT", "median", "GT", 50, 0, range(51, 100)),
                                        ("RANGE", "around_median", "RANGE", 10, 20, range(10, 21)),
                                        ("LE", "narrow", "LE", 50, 0, range(1, 51)),
                                        ("EQ", "frequent", "EQ", 7, 0, [7])):
        _same(_heap(eng, s, op, *p[name], False), ex[op, name, False], f"large {op} {name}, first")
        eng.bsi(b2, sop, small.bit_count(), sa, se, small.min, small.max, want_sum=True)
        got = eng.fetch().serialize()
        assert got == small.compare(sop, sa, se) and list(O.to_values(got)) == list(sexp), (sop, sa, se)
        assert eng.bsi_sums() == (sum(sexp), len(sexp))
        _same(_heap(eng, s, op, *p[name], False), ex[op, name, False], f"large {op} {name}, again")
    eng.release(b2)


def test_buffer_compare(eng, idx):
    """the buffer package's circuit: every op and rangeNEQ called directly (op 7) x every predicate x {no
    found set, found set}; GE and RANGE at the median run owenGreatEqual over three or more orInputs, whose
    chain order the host replays over thousands of keys (owen_order)"""
    s = idx
    ex = expected(s.seed, s.run_optimize, "buffer")
    for wf in (False, True):
        for name, a, e in s.preds:
            for op in _bsi.OPS + ("NEQ_DIRECT",):
                got = _buffer(eng, s, 7 if op == "NEQ_DIRECT" else op, a, e, wf)
                _same(got, ex[op, name, wf], f"buffer {op} {name} ({a}, {e}) found={wf}")
                if name == "median":
                    assert np.array_equal(vals64(got), np_compare(s, "buffer", op, a, e, wf)), (op, wf, "not the numpy set")


def test_one_shot_api(idx):
    """RoaringBitmapSliceIndex / ImmutableBitSliceIndex built from the oracle's bytes: one compare and one
    sum per class (each call loads the index anew)"""
    import roaringbitmap_amd as rb
    s = idx
    bms = [rb.RoaringBitmap(b) for b in [s.heap.ebm] + s.heap.ba]
    found = rb.RoaringBitmap(s.found)
    for cls, package in ((rb.RoaringBitmapSliceIndex, "heap"), (rb.ImmutableBitSliceIndex, "buffer")):
        g = cls(bms[0], bms[1:], s.lo, s.hi)
        ex = expected(s.seed, s.run_optimize, package)
        a, e = next((a, e) for n, a, e in s.preds if n == "around_median")
        _same(g.compare("RANGE", a, e, found).serialize(), ex["RANGE", "around_median", True], f"{package} one-shot RANGE")
        assert g.sum(found) == np_sum(s, s.fsel), package
