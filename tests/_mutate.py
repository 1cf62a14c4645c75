"""The model of the point mutations: RoaringBitmap.add(int) / remove(int) replayed one value at a time, as the
reference's text has them.  Test-only, written from the Java and independent of the library's host form.

    RoaringBitmap.add(int)            RB/RoaringBitmap.java:1162 (addN :498-570 is the same per value)
    RoaringBitmap.remove(int)         :2637-2648 (an emptied container is removed, :2645-2647)
    checkedAdd / checkedRemove        :1610 / :1646 (true iff the cardinality changed)
    ArrayContainer.add / remove       RB/ArrayContainer.java:143-171 / :1007-1014
    BitmapContainer.add / remove      RB/BitmapContainer.java:149-159 / :1184-1202
    RunContainer.add / remove         RB/RunContainer.java:248-302 / :2038-2070

Containers: an ArrayContainer is a sorted list, a BitmapContainer a bytearray of 65,536 flags with its
cardinality, a RunContainer two parallel lists (start, length - 1)."""
from bisect import bisect_left, bisect_right

import numpy as np

from _fmt import A, B, R, decode, encode

MAX = 4096  # ArrayContainer.DEFAULT_MAX_SIZE


class Arr:
    kind = A

    def __init__(self, vals=()):
        self.c = [int(v) for v in vals]

    def card(self):
        return len(self.c)

    def contains(self, x):
        i = bisect_left(self.c, x)
        return i < len(self.c) and self.c[i] == x

    def add(self, x):  # :143-171
        c = self.c
        if not c or x > c[-1]:
            if len(c) >= MAX:
                return self.to_bitmap().add(x)
            c.append(x)
        else:
            loc = bisect_left(c, x)
            if loc >= len(c) or c[loc] != x:
                if len(c) >= MAX:  # an ArrayContainer becomes a BitmapContainer at DEFAULT_MAX_SIZE
                    return self.to_bitmap().add(x)
                c.insert(loc, x)
        return self

    def remove(self, x):  # :1007-1014
        loc = bisect_left(self.c, x)
        if loc < len(self.c) and self.c[loc] == x:
            del self.c[loc]
        return self

    def to_bitmap(self):
        return Bmp(self.c)

    def values(self):
        return np.asarray(self.c, dtype=np.uint16)


class Bmp:
    kind = B

    def __init__(self, vals=()):
        flags = np.zeros(65536, dtype=np.uint8)
        flags[np.asarray(vals, dtype=np.int64)] = 1
        self.bits = bytearray(flags.tobytes())
        self.n = len(vals)

    def card(self):
        return self.n

    def contains(self, x):
        return self.bits[x] == 1

    def add(self, x):  # :149-159: returns this, whatever the cardinality
        if not self.bits[x]:
            self.bits[x] = 1
            self.n += 1
        return self

    def remove(self, x):  # :1184-1202
        if self.n == MAX + 1:  # the uncommon path
            if self.bits[x]:
                self.n -= 1
                self.bits[x] = 0
                return Arr(np.nonzero(np.frombuffer(self.bits, dtype=np.uint8))[0])
        if self.bits[x]:
            self.bits[x] = 0
            self.n -= 1
        return self

    def values(self):
        return np.nonzero(np.frombuffer(self.bits, dtype=np.uint8))[0].astype(np.uint16)


class Run:
    kind = R

    def __init__(self, runs=()):
        self.s = [int(s) for s, _ in runs]
        self.l = [int(le) for _, le in runs]
        self.branch = None  # the branch the last add / remove took (the tests of the branches read it)

    def card(self):
        return sum(self.l) + len(self.l)

    def _search(self, k):
        """unsignedInterleavedBinarySearch over the starts: the index of k, or -(insertion point) - 1"""
        i = bisect_left(self.s, k)
        return i if i < len(self.s) and self.s[i] == k else -i - 1

    def contains(self, x):
        i = bisect_right(self.s, x) - 1
        return i >= 0 and x - self.s[i] <= self.l[i]

    def add(self, k):  # :248-302
        s, l = self.s, self.l
        index = self._search(k)
        if index >= 0:
            self.branch = "add:present"
            return self  # already there
        index = -index - 2  # points to the preceding value, possibly -1
        if index >= 0:  # possible match
            offset = k - s[index]
            le = l[index]
            if offset <= le:
                self.branch = "add:present"
                return self
            if offset == le + 1:
                if index + 1 < len(s) and s[index + 1] == k + 1:  # fusion
                    l[index] = s[index + 1] + l[index + 1] - s[index]
                    del s[index + 1], l[index + 1]
                    self.branch = "add:fuse"
                    return self
                l[index] += 1
                self.branch = "add:extend-up"
                return self
            if index + 1 < len(s) and s[index + 1] == k + 1:
                s[index + 1] = k
                l[index + 1] += 1
                self.branch = "add:extend-down"
                return self
        if index == -1 and s and s[0] == k + 1:  # we may need to extend the first run
            l[0] += 1
            s[0] -= 1
            self.branch = "add:extend-down"
            return self
        s.insert(index + 1, k)
        l.insert(index + 1, 0)
        self.branch = "add:new-run"
        return self

    def remove(self, x):  # :2038-2070
        s, l = self.s, self.l
        index = self._search(x)
        if index >= 0:
            if l[index] == 0:
                del s[index], l[index]
            else:
                s[index] += 1
                l[index] -= 1
            self.branch = "remove:first"
            return self
        index = -index - 2
        if index >= 0:
            offset = x - s[index]
            le = l[index]
            if offset < le:  # need to break in two
                l[index] = offset - 1
                s.insert(index + 1, x + 1)
                l.insert(index + 1, le - offset - 1)
                self.branch = "remove:split"
                return self
            if offset == le:
                l[index] -= 1
                self.branch = "remove:last"
                return self
        self.branch = "remove:absent"
        return self

    def runs(self):
        return list(zip(self.s, self.l))

    def values(self):
        if not self.s:
            return np.zeros(0, dtype=np.uint16)
        return np.concatenate([np.arange(a, a + b + 1) for a, b in zip(self.s, self.l)]).astype(np.uint16)


def _runs_of_values(vals):
    from _fmt import runs_of
    return runs_of(vals)


def load(serialized):
    out = {}
    for key, kind, card, vals, nr in decode(serialized):
        if kind == A:
            out[key] = Arr(vals)
        elif kind == B:
            out[key] = Bmp(vals)
        else:
            out[key] = Run(_runs_of_values(vals))
    return out


def dump(ctrs):
    recs = []
    for key in sorted(ctrs):
        c = ctrs[key]
        vals = c.values()
        if c.kind == R:  # encode() writes the maximal runs of the values: the model's runs must be those
            assert c.runs() == _runs_of_values(vals), "the replay left runs that are not maximal"
        recs.append((key, c.kind, vals))
    return encode(recs)


def mutate_reference(serialized, values, remove):
    """-> (the serialized bitmap after x.add(v) / x.remove(v) for every v in order, the number of checkedAdd /
    checkedRemove calls that would have returned true)"""
    ctrs = load(serialized)
    hits = 0
    for v in np.asarray(values, dtype=np.int64).reshape(-1).tolist():
        v &= 0xFFFFFFFF
        hb, lb = v >> 16, v & 0xFFFF
        c = ctrs.get(hb)
        if remove:
            if c is None:
                continue
            if c.contains(lb):
                hits += 1
            c = c.remove(lb)
            if c.card() == 0:
                del ctrs[hb]  # :2645-2647
            else:
                ctrs[hb] = c
        else:
            if c is None:
                ctrs[hb] = Arr([lb])  # a fresh ArrayContainer
                hits += 1
            else:
                if not c.contains(lb):
                    hits += 1
                ctrs[hb] = c.add(lb)
    return dump(ctrs), hits


# ---- the case list of the device and host tests: name -> (operand bytes, values, remove) ------------------------
def _k(key, lows):
    return (int(key) << 16) | np.asarray(lows, dtype=np.int64)


def thrice_shuffled(rng, v):
    return rng.permutation(np.repeat(np.asarray(v, dtype=np.int64), 3))


def mixed_operand():
    """keys 3 (A), 7 (B), 9 (R), 65535 (A, with 0xFFFFFFFF)"""
    return encode([(3, A, np.arange(0, 3000, 3)), (7, B, np.arange(0, 65536, 5)),
                   (9, R, np.concatenate([np.arange(100, 200), np.arange(1000, 1001), np.arange(40000, 50000)])),
                   (65535, A, [0, 77, 65535])])


def passthrough_operand():
    """300 keys mixing A, B and R; keys 150 and 152 hold run containers of 4,096 and 32,768 runs"""
    rng = np.random.default_rng(77)
    ctrs = []
    for i, key in enumerate(range(10, 310)):
        if key == 150:
            ctrs.append((key, R, np.arange(0, 4096 * 4, 4)))
        elif key == 152:
            ctrs.append((key, R, np.arange(0, 65536, 2)))
        elif i % 15 == 0:
            ctrs.append((key, B, np.sort(rng.choice(65536, 5000 + 37 * i, replace=False))))
        elif i % 15 == 1:
            ctrs.append((key, R, np.concatenate([np.arange(50 * j, 50 * j + 20 + i % 7) for j in range(0, 900, 3)])))
        else:
            ctrs.append((key, A, np.sort(rng.choice(65536, 1 + (i * 13) % 700, replace=False))))
    return encode(ctrs)


def _build_cases():
    rng = np.random.default_rng(2024)
    c = {}
    mixed = mixed_operand()
    empty = encode([])
    # edges
    c["n0_add"] = (mixed, [], False)
    c["n0_remove"] = (mixed, [], True)
    c["n0_empty"] = (empty, [], False)
    c["add_into_empty"] = (empty, rng.integers(0, 1 << 32, 3000), False)
    c["ends_add"] = (mixed, [0, 0xFFFFFFFF, 0xFFFF, 0xFFFF0000], False)
    c["ends_remove"] = (encode([(0, A, [0, 5]), (65535, A, [0, 65535])]), [0, 0xFFFFFFFF], True)
    c["remove_absent_keys"] = (mixed, np.concatenate([_k(0, [1, 2]), _k(5, [0, 3000]), _k(8, [7]), _k(70000 >> 1, [9]),
                                                      _k(65534, [65535])]), True)
    # type boundaries, one container each
    lows = np.sort(rng.choice(65536, 4098, replace=False)).astype(np.int64)
    a4095, a4096, b4097 = encode([(5, A, lows[:4095])]), encode([(5, A, lows[:4096])]), encode([(5, B, lows[:4097])])
    absent = int(np.setdiff1d(np.arange(65536), lows)[123])
    bound = {"a4095_new": (a4095, _k(5, [lows[4095]]), False),
             "a4096_present": (a4096, _k(5, [lows[17]]), False),
             "a4096_new": (a4096, _k(5, [lows[4096]]), False),
             "b4097_present": (b4097, _k(5, [lows[4000]]), True),
             "b4097_absent": (b4097, _k(5, [absent]), True),
             "b_filled": (b4097, _k(5, np.arange(65536)), False)}
    for name, (op, v, rem) in bound.items():
        c[name] = (op, v, rem)
        c[name + "_x3"] = (op, thrice_shuffled(rng, v), rem)
    # run containers
    runs = encode([(2, R, np.concatenate([np.arange(10, 20), np.arange(22, 30), np.arange(500, 501)]))])
    c["run_add_inside"] = (runs, _k(2, [10, 15, 19, 500]), False)
    c["run_add_below"] = (runs, _k(2, [9]), False)
    c["run_add_above"] = (runs, _k(2, [30]), False)
    c["run_add_join"] = (runs, _k(2, [21, 20]), False)
    c["run_add_isolated"] = (runs, _k(2, [0, 300, 65535]), False)
    full = encode([(4, R, np.arange(65536))])
    c["run_full_add"] = (full, _k(4, rng.integers(0, 65536, 500)), False)
    c["run_remove_first"] = (runs, _k(2, [10]), True)
    c["run_remove_last"] = (runs, _k(2, [29]), True)
    c["run_remove_middle"] = (runs, _k(2, [25]), True)
    c["run_remove_single"] = (runs, _k(2, [500]), True)
    c["run_three_isolated"] = (runs, _k(2, np.setdiff1d(np.concatenate([np.arange(10, 20), np.arange(22, 30)]),
                                                        [12, 27])), True)
    c["run_emptied"] = (runs, _k(2, np.arange(0, 600)), True)
    c["run_grow_past_stage"] = (encode([(6, R, np.arange(10))]), _k(6, 100 + 2 * np.arange(3000)), False)
    c["run_maximum"] = (full, _k(4, np.arange(1, 65536, 2)), True)
    # dropped keys
    five = encode([(1, A, [5, 6]), (2, B, np.arange(0, 65536, 9)), (3, R, np.arange(100, 200)), (4, A, [9]),
                   (8, R, np.arange(7))])
    c["drop_first"] = (five, _k(1, [5, 6, 7]), True)
    c["drop_last"] = (five, _k(8, np.arange(10)), True)
    c["drop_middle_b"] = (five, _k(2, np.arange(65536)), True)
    c["drop_middle_r"] = (five, _k(3, np.arange(50, 250)), True)
    c["drop_all"] = (five, np.concatenate([_k(k, np.arange(65536)) for k in (1, 2, 3, 4, 8)]), True)
    # passthrough
    pt = passthrough_operand()
    c["passthrough_three_keys"] = (pt, np.concatenate([_k(149, rng.integers(0, 65536, 400)), _k(151, [3, 4, 5]),
                                                       _k(153, rng.integers(0, 65536, 5000))]), False)
    c["passthrough_three_keys_remove"] = (pt, np.concatenate([_k(149, np.arange(65536)), _k(151, np.arange(0, 65536, 2)),
                                                              _k(153, rng.integers(0, 65536, 5000))]), True)
    c["passthrough_every_key"] = (pt, _k(0, 0) + (np.arange(10, 310, dtype=np.int64) << 16) + 4097, False)
    # wave patterns
    c["wave_64_equal"] = (mixed, np.full(64, (3 << 16) | 1), False)
    c["wave_64_one_word"] = (mixed, _k(7, 64 + rng.permutation(64) % 32), False)
    present, missing = (3 << 16) | 3, (3 << 16) | 1
    for n in (65, 100000):
        for at, tag in ((0, "first"), (n - 1, "last")):
            v = np.full(n, present)
            v[at] = missing
            c[f"wave_{n}_{tag}_add"] = (mixed, v, False)
            v = np.full(n, missing)
            v[at] = present
            c[f"wave_{n}_{tag}_remove"] = (mixed, v, True)
    keys = rng.choice(65536, 2000, replace=False).astype(np.int64)
    c["sparse_2000_keys"] = (mixed, (keys << 16) | rng.integers(0, 65536, 2000), False)
    c["sparse_2000_keys_remove"] = (encode([(int(k), A, [1, 2]) for k in np.sort(keys)[::2]]), (keys << 16) | 1, True)
    return c


_CASES, _WANT = None, {}


def cases():
    global _CASES
    if _CASES is None:
        _CASES = {k: (op, np.asarray(v, dtype=np.int64).reshape(-1), rem) for k, (op, v, rem) in _build_cases().items()}
    return _CASES


def case_names():
    return list(cases())


def expected(name):
    """the model's (bytes, changed) of a case, computed once"""
    if name not in _WANT:
        op, v, rem = cases()[name]
        _WANT[name] = mutate_reference(op, v, rem)
    return _WANT[name]


def nine_keys_batch():
    """200,000 values over nine keys and the operand they meet (array, bitmap and run containers, two keys absent)"""
    rng = np.random.default_rng(9)
    op = encode([(20, A, np.arange(0, 4000, 2)), (21, B, np.arange(0, 65536, 3)), (22, R, np.arange(1000, 30000)),
                 (23, A, np.arange(4090)), (24, B, np.arange(4100)), (26, R, np.arange(0, 65536, 4)),
                 (28, A, [1]), (40, A, [2])])
    v = ((20 + rng.integers(0, 9, 200000)) << 16) | (rng.integers(0, 256, 200000) ** 2)
    return op, v
