"""One context, a stream of independent ops: a pairwise op that finds the last result's serialization enqueued and
not consumed takes the context's other result set and runs on that set's stream, so ops alternate between two
in-order lanes.  Only ordering changed, so every check here is bytes against the oracle, in the
sequences where an ordering mistake would show: the op after a serialization (the other lane, which must not touch
what the serialization still reads), the op after that (the first lane again, behind its own serialization),
consumers between ops (which join the lane first), operands released while the other lane still reads their
payload, and ops of other kinds, which run on the context's stream behind both lanes.

Inputs: pairs of 300 and 450 keys holding all nine container-kind pairs (array / bitmap / run on either
side), two sevenths of the keys in one operand only (cloned by or / xor / andnot: pass-through records that
point into operand memory), and a pair with disjoint keys whose AND is empty.  Each sequence runs in the
planned form (full key range: k_plan_pairwise + k_pair_wave) and in the balanced one (a dense key range:
k_plan_balanced + k_pair_cu, the headline's kernels), both serialized by k_serialize_agg.

The device error word (a look-back spin that timed out) lives in each set's own look-back block, so one op's
word cannot reach the next op's result; no input makes a spin time out, so what is tested is the errors inputs
can cause: they are reported by the call that consumes the bad result or makes it, and the op after succeeds.
"""
import struct

import numpy as np
import pytest

import _gen
import _oracle as O
from _fmt import A, B, R, decode, encode

pytestmark = pytest.mark.gpu

KIND_MODE = {A: "a_mid", B: "b_mid", R: "r_mid"}
FORMS = ("planned", "balanced")


def _pair(seed, n_keys):
    """Two bitmaps over keys [0, n_keys): key k holds kind pair k % 9; every 7th key (from 1) in the first
    operand only, every 7th (from 4) in the second only."""
    rng = np.random.default_rng(seed)
    ca, cb = [], []
    for k in range(n_keys):
        ka, kb = (A, B, R)[(k % 9) // 3], (A, B, R)[k % 3]
        if k % 7 != 4:
            ca.append((k, ka, _gen.container(rng, KIND_MODE[ka])[1]))
        if k % 7 != 1:
            cb.append((k, kb, _gen.container(rng, KIND_MODE[kb])[1]))
    return encode(ca), encode(cb)


class _Inputs:
    def __init__(self):
        self.a, self.b = _pair(0x51, 300)
        self.c, self.d = _pair(0x52, 450)
        rng = np.random.default_rng(0x53)
        # disjoint keys: the AND is the empty bitmap
        self.e1 = encode([(k, A, _gen.container(rng, "a_small")[1]) for k in range(0, 200, 2)])
        self.e2 = encode([(k, R, _gen.container(rng, "r_few")[1]) for k in range(1, 200, 2)])
        self.bufs = {"a": self.a, "b": self.b, "c": self.c, "d": self.d, "e1": self.e1, "e2": self.e2}
        self._exp = {}

    def exp(self, op, x, y):
        """oracle bytes of op(x, y), computed once"""
        if (op, x, y) not in self._exp:
            self._exp[(op, x, y)] = O.pairwise(op, self.bufs[x], self.bufs[y])
        return self._exp[(op, x, y)]


@pytest.fixture(scope="module")
def inp():
    return _Inputs()


def _engine():
    from roaringbitmap_amd import Engine
    return Engine(0)


def _load(e, inp, names):
    return dict(zip(names, e.load_pair(*[inp.bufs[n] for n in names])))


def _op(e, ids, form, op, x, y, n_keys):
    """op(x, y) + serialize; balanced: over the dense key range [0, n_keys) that holds every key"""
    if form == "balanced":
        e.pairwise(op, ids[x], ids[y], key_lo=0, key_hi=n_keys)
    else:
        e.pairwise(op, ids[x], ids[y])
    e.serialize()


def _layout(exp):
    """(containers, has_run, descriptor offset, payload offset, has an offset table) of serialized bytes"""
    n = len(decode(exp))
    has_run = int((struct.unpack("<I", exp[:4])[0] & 0xFFFF) == 12347)
    desc_base = 4 + (n + 7) // 8 if has_run else 8
    offsets = not has_run or n >= 4
    return n, has_run, desc_base, desc_base + 4 * n + (4 * n if offsets else 0), offsets


def test_inputs_cover_the_cases(inp):
    for x, y in ((inp.a, inp.b), (inp.c, inp.d)):
        dx, dy = {c[0]: c[1] for c in decode(x)}, {c[0]: c[1] for c in decode(y)}
        assert {(dx[k], dy[k]) for k in dx if k in dy} == {(p, q) for p in (A, B, R) for q in (A, B, R)}
        assert set(dx) - set(dy) and set(dy) - set(dx)
    assert len(decode(inp.exp("and", "e1", "e2"))) == 0
    assert len(decode(inp.exp("and", "a", "b"))) > 100 and len(decode(inp.exp("or", "c", "d"))) == 450


@pytest.mark.parametrize("form", FORMS)
def test_alternating_ops(gpu, inp, form):
    """and(a, b) + serialize, or(c, d) + serialize, fetch -> (c, d)'s bytes; five times, alternating the order;
    then the same with the empty result on either side"""
    e = _engine()
    try:
        ids = _load(e, inp, ("a", "b", "c", "d", "e1", "e2"))
        first, second = ("and", "a", "b", 300), ("or", "c", "d", 450)
        for rep in range(5):
            _op(e, ids, form, *first)
            _op(e, ids, form, *second)
            assert e.fetch().serialize() == inp.exp(*second[:3]), (rep, second)
            first, second = second, first
        # no fetch in between: the third op reuses the first op's set behind its serialization
        for rep in range(5):
            _op(e, ids, form, *first)
            first, second = second, first
        assert e.fetch().serialize() == inp.exp(*second[:3])
        for seq in ((("and", "e1", "e2", 200), ("xor", "a", "b", 300)), (("andnot", "c", "d", 450), ("and", "e1", "e2", 200))):
            for o in seq:
                _op(e, ids, form, *o)
            assert e.fetch().serialize() == inp.exp(*seq[1][:3]), seq
    finally:
        e.close()


@pytest.mark.parametrize("form", FORMS)
def test_consumers_between_ops(gpu, inp, form):
    """with one serialization behind it and its own in flight, a result's statistics, bytes and key-shard pieces
    are its own; the next op's are the next op's"""
    exp = inp.exp("xor", "a", "b")
    n, has_run, desc_base, head, offsets = _layout(exp)
    e = _engine()
    try:
        ids = _load(e, inp, ("a", "b", "c", "d"))
        _op(e, ids, form, "or", "c", "d", 450)
        _op(e, ids, form, "xor", "a", "b", 300)
        st = e.result_stats()
        assert (st["containers"], st["has_run"], st["payload_bytes"]) == (n, has_run, len(exp) - head)
        assert st["cardinality"] == O.pairwise_card("xor", inp.a, inp.b)
        assert e.fetch().serialize() == exp
        _op(e, ids, form, "or", "c", "d", 450)
        assert e.fetch().serialize() == inp.exp("or", "c", "d")
        # a key-shard fetch right behind the serialization: descriptors, offsets and payload of the result
        _op(e, ids, form, "or", "c", "d", 450)
        _op(e, ids, form, "xor", "a", "b", 300)
        d, o, p = e.fetch_shard(n, has_run, 0, 0)
        assert d == exp[desc_base:desc_base + 4 * n]
        if offsets:
            assert o == exp[desc_base + 4 * n:head]
        assert p == exp[head:]
        assert e.fetch().serialize() == exp
    finally:
        e.close()


@pytest.mark.parametrize("form", FORMS)
def test_operands_released_while_serializing(gpu, inp, form):
    """or keeps the unmatched keys' containers as records that point into operand memory.  Released operands'
    buffers go to the pool and a load of the same size takes them at once: it must land behind the
    serialization that still reads them."""
    exp = inp.exp("or", "a", "b")
    e = _engine()
    try:
        # as a caller would: the bytes fetched before the release, the next op on the new batches
        ids = _load(e, inp, ("a", "b"))
        _op(e, ids, form, "or", "a", "b", 300)
        assert e.fetch().serialize() == exp
        e.release(ids["a"])
        e.release(ids["b"])
        ids = _load(e, inp, ("b", "a"))  # the same sizes, the other way round: over the released payloads
        _op(e, ids, form, "andnot", "b", "a", 300)
        assert e.fetch().serialize() == inp.exp("andnot", "b", "a")
        # the release while the serialization is in flight, the reload over it, and only then the fetch
        _op(e, ids, form, "or", "a", "b", 300)
        e.release(ids["a"])
        e.release(ids["b"])
        ids = _load(e, inp, ("b", "a"))
        assert e.fetch().serialize() == exp
        _op(e, ids, form, "xor", "a", "b", 300)
        assert e.fetch().serialize() == inp.exp("xor", "a", "b")
        # ... with another op's serialization in flight behind it
        _op(e, ids, form, "or", "a", "b", 300)
        _op(e, ids, form, "and", "a", "b", 300)
        e.release(ids["a"])
        e.release(ids["b"])
        ids = _load(e, inp, ("b", "a"))
        assert e.fetch().serialize() == inp.exp("and", "a", "b")
    finally:
        e.close()


def test_ops_without_a_set_of_their_own(gpu, inp):
    """a card-only op, a wide op, a key-range op with its shard fetch and an op through the big-run arena, each
    right behind a pairwise + serialize; and the pairwise + serialize behind each of them"""
    wide_bufs = [inp.a, inp.b, inp.c, inp.d]
    exp_wide = O.wide("or", wide_bufs)
    exp_and = inp.exp("and", "a", "b")
    e = _engine()
    try:
        ids = _load(e, inp, ("a", "b", "c", "d"))
        w = e.load(wide_bufs)
        for rep in range(2):
            _op(e, ids, "planned", "or", "c", "d", 450)
            e.and_cardinality(ids["a"], ids["b"])
            assert e.card() == O.pairwise_card("and", inp.a, inp.b)
            _op(e, ids, "balanced", "and", "a", "b", 300)
            e.wide("or", w)
            assert e.fetch().serialize() == exp_wide
            _op(e, ids, "planned", "or", "c", "d", 450)
            e.wide_card("or", w)
            assert e.card() == O.wide_card("or", wide_bufs)
            # keys [0, 150) of and(a, b) as a shard: a prefix of the whole result's containers
            _op(e, ids, "balanced", "or", "c", "d", 450)
            e.pairwise("and", ids["a"], ids["b"], key_lo=0, key_hi=150)
            part = [c for c in decode(exp_and) if c[0] < 150]
            st = e.result_stats()
            assert st["containers"] == len(part)
            pexp = encode([(c[0], c[1], c[3]) for c in part])
            n, has_run, desc_base, head, offsets = _layout(pexp)
            d, o, p = e.fetch_shard(n, has_run, 0, 0)
            assert d == pexp[desc_base:desc_base + 4 * n] and p == pexp[head:]
            # the buffer package's and: its run results may go to the context's big-run arena
            _op(e, ids, "planned", "or", "c", "d", 450)
            e.pairwise("and_buffer", ids["a"], ids["b"])
            e.serialize()
            _op(e, ids, "planned", "and", "a", "b", 300)
            assert e.fetch().serialize() == exp_and
    finally:
        e.close()


def test_error_then_good_op(gpu, inp):
    """an op its inputs make fail is reported by its own call, a consumer with nothing to consume by that
    consumer; neither reaches the results before or after"""
    import roaringbitmap_amd as rb
    full01 = encode([(0, R, np.arange(65536)), (1, R, np.arange(65536))])
    e = _engine()
    try:
        ids = _load(e, inp, ("a", "b", "c", "d"))
        empty, full = e.load_pair(encode([]), full01)
        two = e.load([inp.a, inp.b])  # two bitmaps in one batch: no pairwise operand
        with pytest.raises(rb.IllegalArgumentException):
            e.fetch()  # nothing pending
        _op(e, ids, "planned", "and", "a", "b", 300)
        with pytest.raises(rb.IllegalArgumentException):
            e.pairwise("or", ids["a"], two)  # refused before it takes a set
        assert e.fetch().serialize() == inp.exp("and", "a", "b")
        _op(e, ids, "planned", "or", "c", "d", 450)
        _op(e, ids, "planned", "and", "a", "b", 300)
        with pytest.raises(rb.IllegalArgumentException):
            e.ornot(empty, full, 0)  # the reference's NegativeArraySizeException: found after the op ran
        with pytest.raises(rb.IllegalArgumentException):
            e.fetch()  # the failed op left no result
        _op(e, ids, "planned", "or", "c", "d", 450)
        assert e.fetch().serialize() == inp.exp("or", "c", "d")
        assert e.result_stats()["containers"] == 450
    finally:
        e.close()


def test_two_contexts_alternately(gpu, inp):
    e1, e2 = _engine(), _engine()
    try:
        i1, i2 = _load(e1, inp, ("a", "b", "c", "d")), _load(e2, inp, ("a", "b", "c", "d"))
        for rep in range(3):
            _op(e1, i1, "balanced", "and", "a", "b", 300)
            _op(e2, i2, "planned", "or", "c", "d", 450)
            _op(e1, i1, "planned", "xor", "c", "d", 450)
            _op(e2, i2, "balanced", "andnot", "a", "b", 300)
            assert e1.fetch().serialize() == inp.exp("xor", "c", "d")
            assert e2.fetch().serialize() == inp.exp("andnot", "a", "b")
        e1.sync()
        e2.sync()
    finally:
        e1.close()
        e2.close()
