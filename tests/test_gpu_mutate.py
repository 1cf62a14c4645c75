"""Batches of values added to or removed from a resident bitmap on the MI355X (rbg_ctx_mutate_values[_device],
rbg_mutate_values; RoaringBitmap.add(int...) / addN / remove(int) / checkedAdd / checkedRemove,
RB/RoaringBitmap.java:483-570, 2637-2648, 1610, 1646).  The acceptance throughout: the result, fetched, is byte
for byte what the model of tests/_mutate.py (the reference's add / remove replayed value by value) gives,
`changed` is the model's count of checkedAdd / checkedRemove hits, and the operand's fetched bytes are unchanged
after the call."""
import ctypes

import numpy as np
import pytest

import _mutate as M
import _oracle as O
from _fmt import A, B, R, decode, encode

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng(gpu):
    import roaringbitmap_amd as rb
    e = rb.Engine(0)
    yield e
    e.close()


def _u32(v):
    return np.ascontiguousarray(np.asarray(v, dtype=np.int64).astype(np.uint32))


def _check(eng, x, v, remove, want, tag=""):
    """one call on the loaded batch of x against want = (bytes, changed); the operand before and after"""
    a = eng.load_pair(x)[0]
    before = eng.batch_fetch(a).serialize()
    r, changed = eng.mutate_values(a, v, remove)
    got = eng.batch_fetch(r).serialize()
    after = eng.batch_fetch(a).serialize()
    st = eng.batch_stats(r)
    eng.release(r)
    eng.release(a)
    assert before == x and after == x, tag
    assert got == want[0], (tag, len(got), len(want[0]), [c[1] for c in decode(got)][:20])
    assert changed == want[1], (tag, changed, want[1])
    kinds = [c[1] for c in decode(got)]
    assert (st["bitmaps"], st["containers"], st["array"], st["bitmap"], st["run"]) == \
        (1, len(kinds), kinds.count(A), kinds.count(B), kinds.count(R)), tag
    assert st["serialized_bytes"] == len(got) and st["cardinality"] == sum(len(c[3]) for c in decode(got)), tag


@pytest.mark.parametrize("name", M.case_names())
def test_case(eng, name):
    x, v, remove = M.cases()[name]
    _check(eng, x, v, remove, M.expected(name), name)


def test_add_into_empty_is_from_values(eng):
    rng = np.random.default_rng(3)
    v = np.concatenate([rng.integers(0, 1 << 32, 20000), (9 << 16) | rng.integers(0, 65536, 9000), [0, 0xFFFFFFFF]])
    e = eng.from_values([])
    r, changed = eng.add_values(e, v)
    want = O.from_values(_u32(v), False)
    assert eng.batch_fetch(r).serialize() == want and changed == len(np.unique(v))
    assert eng.batch_stats(e)["containers"] == 0
    eng.release(r)
    eng.release(e)


@pytest.mark.parametrize("remove", [False, True])
def test_nine_keys_in_five_orders(eng, remove):
    rng = np.random.default_rng(4)
    x, v = M.nine_keys_batch()
    want = M.mutate_reference(x, v, remove)
    for i, order in enumerate((v, np.sort(v), np.sort(v)[::-1], rng.permutation(v),
                               rng.permutation(np.concatenate([v, v[:999]])))):
        _check(eng, x, order, remove, want, i)


def test_every_key_emptied_then_added_to_again(eng):
    x, v, _ = M.cases()["drop_all"]
    a = eng.load_pair(x)[0]
    r, changed = eng.remove_values(a, v)
    assert eng.batch_fetch(r).serialize() == encode([]) and changed == M.expected("drop_all")[1]
    st = eng.batch_stats(r)
    assert st["containers"] == 0 and st["cardinality"] == 0
    again = np.array([5, (3 << 16) | 7, (3 << 16) | 8, 0xFFFFFFFF])
    r2, changed = eng.add_values(r, again)
    assert changed == 4 and eng.batch_fetch(r2).serialize() == M.mutate_reference(encode([]), again, False)[0]
    r3, changed = eng.remove_values(r, again)  # a remove from the empty result
    assert changed == 0 and eng.batch_fetch(r3).serialize() == encode([])
    for b in (a, r, r2, r3):
        eng.release(b)


def test_result_as_operand(eng):
    """the result against the loaded batch of the model's bytes, in the ops that take a loaded bitmap"""
    rng = np.random.default_rng(8)
    x = M.passthrough_operand()
    v = np.concatenate([(149 << 16) | rng.integers(0, 65536, 3000), (150 << 16) | np.arange(1, 400, 4),
                        (152 << 16) | np.arange(1, 65536, 2), (9 << 16) | np.arange(5000), (400 << 16) | np.arange(3)])
    want, hits = M.mutate_reference(x, v, False)
    a = eng.load_pair(x)[0]
    res, changed = eng.add_values(a, v)
    model = eng.load([want])
    other_bytes = O.from_values(_u32(np.concatenate([rng.integers(0, 420 << 16, 200000), (152 << 16) | np.arange(999)])))
    other = eng.load([other_bytes])
    assert changed == hits and eng.batch_fetch(res).serialize() == want
    assert eng.batch_stats(res) == eng.batch_stats(model)
    for op in ("and", "or"):
        eng.pairwise(op, res, other)
        got = eng.fetch().serialize()
        eng.pairwise(op, model, other)
        assert got == eng.fetch().serialize() == O.pairwise(op, want, other_bytes), op
    vals = O.to_values(want).astype(np.int64)
    q = np.concatenate([rng.choice(vals, 3000), rng.integers(0, 420 << 16, 3000), [0, 0xFFFFFFFF]])
    for op in ("rank", "contains"):
        assert (eng.point_query(op, res, q) == eng.point_query(op, model, q)).all(), op
    assert (eng.point_query("contains", res, q) == np.isin(q, vals)).all()
    ranks = rng.integers(0, len(vals), 3000)
    assert (eng.point_query("select", res, ranks) == vals[ranks]).all()
    assert (eng.to_values(res) == vals).all()
    ro_res, ans_res = eng.run_optimize(res)
    ro_model, ans_model = eng.run_optimize(model)
    assert ans_res == ans_model
    assert eng.batch_fetch(ro_res).serialize() == eng.batch_fetch(ro_model).serialize() == O.run_optimize(want)
    # a second mutation of its own result, and of the run-optimized result
    v2 = np.concatenate([(152 << 16) | np.arange(0, 65536, 2), (149 << 16) | np.arange(65536), v[::3]])
    want2 = M.mutate_reference(want, v2, True)
    res2, changed2 = eng.remove_values(res, v2)
    assert (eng.batch_fetch(res2).serialize(), changed2) == want2
    want3 = M.mutate_reference(O.run_optimize(want), v2[::5], True)
    res3, changed3 = eng.remove_values(ro_res, v2[::5])
    assert (eng.batch_fetch(res3).serialize(), changed3) == want3
    assert eng.batch_fetch(res).serialize() == want and eng.batch_fetch(a).serialize() == x
    for b in (a, res, model, other, ro_res, ro_model, res2, res3):
        eng.release(b)


def test_torch_tensors(eng):
    import torch
    rng = np.random.default_rng(9)
    x = M.mixed_operand()
    v = np.concatenate([rng.integers(0, 12 << 16, 30000), [0xFFFFFFFF, 0, 0xFFFF0000, (65535 << 16) | 77]])
    dev = torch.device("cuda", 0)
    a = eng.load_pair(x)[0]
    signed = np.where(v >= 1 << 31, v - (1 << 32), v).astype(np.int64)  # 0xFFFFFFFF as -1: the low 32 bits count
    for remove in (False, True):
        want = M.mutate_reference(x, v, remove)
        for t in (torch.from_numpy(v.astype(np.int64)).to(dev), torch.from_numpy(signed).to(dev),
                  torch.from_numpy(_u32(v).view(np.int32)).to(dev).view(torch.uint32)):
            r, changed = eng.mutate_values(a, t, remove)
            assert (eng.batch_fetch(r).serialize(), changed) == want, (remove, t.dtype)
            eng.release(r)
    r, changed = eng.add_values(a, torch.zeros(0, dtype=torch.int64, device=dev))
    assert changed == 0 and eng.batch_fetch(r).serialize() == x
    eng.release(r)
    with pytest.raises(ValueError):
        eng.add_values(a, torch.zeros(4, dtype=torch.int32, device=dev))
    eng.release(a)


def test_refusals_leak_no_batch(eng):
    import roaringbitmap_amd as rb
    from roaringbitmap_amd import _lib as L
    lib = L.lib()
    arrays = [encode([(1, A, [1, 2, 3])]), encode([(1, A, [2]), (4, A, [9, 10])])]
    good = eng.load_pair(arrays[0])[0]
    packed = eng.load(arrays[:1], packed=True)
    multi = eng.load(arrays)
    bm_major = eng.synth(rb.engine.SYNTH_C4_PAIRS, 5, 4)
    probe = eng.from_values([1])  # the next free batch id
    eng.release(probe)
    v = np.arange(4, dtype=np.uint32)
    p = v.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
    out, ch = ctypes.c_int32(-7), ctypes.c_uint64(99)
    for batch in (packed, multi, bm_major, probe, -1, 1 << 20):  # probe: released
        for remove in (False, True):
            with pytest.raises(rb.IllegalArgumentException):
                eng.mutate_values(batch, v, remove)
    for f, vals in ((lib.rbg_ctx_mutate_values, p), (lib.rbg_ctx_mutate_values_device, ctypes.c_void_p(v.ctypes.data))):
        for op in (2, -1):
            assert f(eng._ctx, good, op, vals, 4, ctypes.byref(out), ctypes.byref(ch)) == L.RBG_ERR_ILLEGAL_ARGUMENT
        assert f(eng._ctx, good, 0, vals, 4, None, ctypes.byref(ch)) == L.RBG_ERR_ILLEGAL_ARGUMENT
        assert f(eng._ctx, good, 0, vals, 4, ctypes.byref(out), None) == L.RBG_ERR_ILLEGAL_ARGUMENT
        assert f(eng._ctx, good, 0, None, 4, ctypes.byref(out), ctypes.byref(ch)) == L.RBG_ERR_ILLEGAL_ARGUMENT
    assert out.value == -7 and ch.value == 99
    again = eng.from_values([1])
    assert again == probe  # no refusal took a batch
    r, changed = eng.add_values(good, [(1 << 16) | 7])  # and the context still works
    assert changed == 1 and eng.batch_fetch(r).serialize() == encode([(1, A, [1, 2, 3, 7])])
    for b in (good, packed, multi, bm_major, again, r):
        eng.release(b)


def test_one_shot(gpu):
    import roaringbitmap_amd as rb
    for name in ("passthrough_three_keys", "passthrough_three_keys_remove", "run_maximum", "drop_all", "n0_add",
                 "add_into_empty", "a4096_new_x3"):
        x, v, remove = M.cases()[name]
        y = rb.RoaringBitmap(x)
        changed = (y.remove_many if remove else y.add_many)(v, gpu=True)
        assert (y.serialize(), changed) == M.expected(name), name
    y = rb.RoaringBitmap()
    assert y.add_many([3, 3, 1 << 31], gpu=True) == 2 and y.remove_many([3, 4], gpu=True) == 1
    assert y.toArray().tolist() == [1 << 31]
    y.add(5, 8)  # two ints are the range form add(rangeStart, rangeEnd); one int to remove is remove(int)
    y.remove(6)
    assert y.toArray().tolist() == [5, 7, 1 << 31]
    y.remove(0, 8)
    assert y.toArray().tolist() == [1 << 31]
