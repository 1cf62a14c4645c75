"""The model of the point mutations (tests/_mutate.py: RoaringBitmap.add(int) / remove(int) replayed value by
value from the reference's text) against the CPU oracle and against hand-written containers.  CPU only."""
import numpy as np
import pytest

import _mutate as M
import _oracle as O
from _fmt import A, B, R, decode, encode


def _u32(v):
    return np.ascontiguousarray(np.asarray(v, dtype=np.int64).astype(np.uint32))


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_run_free_operands_equal_the_pairwise_route(seed):
    """without run containers add is or(x, from_values(v)) and remove is andNot(x, from_values(v)), byte for byte"""
    rng = np.random.default_rng(seed)
    base = np.concatenate([(1 << 16) | rng.choice(65536, 3000 + 1200 * seed, replace=False),   # A, near 4,096 on seed 1
                           (2 << 16) | rng.choice(65536, 4090 + seed, replace=False),          # A at the boundary
                           (3 << 16) | rng.choice(65536, 4097 + 5 * seed, replace=False),      # B just above it
                           (9 << 16) | rng.choice(65536, 30000, replace=False),
                           rng.integers(0, 1 << 32, 500)])
    x = O.from_values(_u32(base), False)
    assert R not in [c[1] for c in decode(x)]
    v = np.concatenate([rng.integers(0, 12 << 16, 20000), rng.choice(base, 6000), rng.integers(0, 1 << 32, 300)])
    v = np.concatenate([v, v[:5000]])  # duplicates
    rng.shuffle(v)
    delta = O.from_values(_u32(v), False)
    got, hits = M.mutate_reference(x, v, False)
    assert got == O.pairwise("or", x, delta)
    assert hits == len(O.to_values(got)) - len(O.to_values(x))
    got, hits = M.mutate_reference(x, v, True)
    assert got == O.pairwise("andnot", x, delta)
    assert hits == len(O.to_values(x)) - len(O.to_values(got))


def test_order_independent():
    """adds alone, or removes alone: five permutations of one batch give one result"""
    rng = np.random.default_rng(5)
    x = M.mixed_operand()
    v = np.concatenate([(3 << 16) | rng.integers(0, 65536, 4000), (7 << 16) | rng.integers(0, 65536, 3000),
                        (9 << 16) | rng.integers(0, 65536, 3000), (11 << 16) | rng.integers(0, 500, 600)])
    for remove in (False, True):
        want = M.mutate_reference(x, v, remove)
        for _ in range(4):
            assert M.mutate_reference(x, rng.permutation(v), remove) == want
        assert M.mutate_reference(x, np.sort(v)[::-1], remove) == want


RUNS = [(10, 9), (22, 7), (500, 0)]  # [10, 19], [22, 29], [500, 500]


@pytest.mark.parametrize("value,branch,want", [
    (15, "add:present", RUNS),                                   # inside a run: offset <= le
    (22, "add:present", RUNS),                                   # a run's start: the search finds it
    (20, "add:extend-up", [(10, 10), (22, 7), (500, 0)]),        # offset == le + 1, no fusion
    (9, "add:extend-down", [(9, 10), (22, 7), (500, 0)]),        # index == -1: the first run grows down
    (499, "add:extend-down", [(10, 9), (22, 7), (499, 1)]),      # the next run grows down
    (300, "add:new-run", [(10, 9), (22, 7), (300, 0), (500, 0)]),
    (0, "add:new-run", [(0, 0), (10, 9), (22, 7), (500, 0)]),
    (65535, "add:new-run", [(10, 9), (22, 7), (500, 0), (65535, 0)]),
])
def test_run_container_add_branches(value, branch, want):
    c = M.Run(RUNS)
    assert c.add(value) is c and c.branch == branch and c.runs() == want


def test_run_container_add_fuses_two_runs():
    c = M.Run([(10, 9), (21, 8), (500, 0)])  # [10, 19], [21, 29]
    assert c.add(20) is c and c.branch == "add:fuse" and c.runs() == [(10, 19), (500, 0)]


@pytest.mark.parametrize("value,branch,want", [
    (10, "remove:first", [(11, 8), (22, 7), (500, 0)]),          # a run's first value: value + 1, length - 1
    (500, "remove:first", [(10, 9), (22, 7)]),                   # a one-value run goes
    (25, "remove:split", [(10, 9), (22, 2), (26, 3), (500, 0)]),  # offset < le: broken in two
    (29, "remove:last", [(10, 9), (22, 6), (500, 0)]),           # offset == le
    (20, "remove:absent", RUNS),
    (5, "remove:absent", RUNS),
    (60000, "remove:absent", RUNS),
])
def test_run_container_remove_branches(value, branch, want):
    c = M.Run(RUNS)
    assert c.remove(value) is c and c.branch == branch and c.runs() == want


def test_array_bitmap_conversions():
    """ArrayContainer.add at 4,096 values, BitmapContainer.remove at 4,097, BitmapContainer.add returns this"""
    a = M.Arr(range(0, 8192, 2))
    assert a.card() == 4096 and a.add(4) is a and a.add(8190) is a  # present: stays an array
    b = a.add(1)
    assert isinstance(b, M.Bmp) and b.card() == 4097
    assert b.remove(3) is b and b.card() == 4097  # absent: stays a bitmap
    a2 = b.remove(1)
    assert isinstance(a2, M.Arr) and a2.c == list(range(0, 8192, 2))
    a = M.Arr(range(4096))
    assert isinstance(a.add(70), M.Arr) and isinstance(a.add(5000), M.Bmp)  # the append path converts too
    full = M.Bmp(range(65536))
    assert full.add(7) is full and full.card() == 65536


def test_whole_bitmap_rules():
    """a new key is an array container, a remove under an absent key does nothing, an emptied container goes, a
    run container keeps its type even where an array would be smaller"""
    x = encode([(2, R, [5, 6, 7, 9])])
    got, hits = M.mutate_reference(x, [(2 << 16) | 6, (1 << 16) | 3, (1 << 16) | 3], False)
    assert hits == 1 and [(c[0], c[1]) for c in decode(got)] == [(1, A), (2, R)]
    got, hits = M.mutate_reference(x, [(2 << 16) | 6, (3 << 16) | 6], True)
    assert hits == 1 and decode(got)[0][1] == R and decode(got)[0][4] == 3  # 5, 7, 9 as three runs
    got, hits = M.mutate_reference(x, (2 << 16) | np.arange(12), True)
    assert hits == 4 and got == encode([])
    assert M.mutate_reference(x, [], False) == (x, 0)


def test_case_facts():
    """what the case list of the device and host tests is meant to reach, read off the model's bytes"""
    def kinds(name):
        return [(c[0], c[1], c[4]) for c in decode(M.expected(name)[0])]
    assert kinds("a4095_new") == [(5, A, 0)] and kinds("a4096_present") == [(5, A, 0)]
    assert kinds("a4096_new") == [(5, B, 0)] and kinds("b4097_present") == [(5, A, 0)]
    assert kinds("b4097_absent") == [(5, B, 0)] and kinds("b_filled") == [(5, B, 0)]
    assert len(decode(M.expected("b_filled")[0])[0][3]) == 65536
    assert M.expected("run_add_inside") == (M.cases()["run_add_inside"][0], 0)  # identical bytes
    assert kinds("run_add_join") == [(2, R, 2)] and kinds("run_full_add") == [(4, R, 1)]
    assert kinds("run_remove_middle") == [(2, R, 4)] and kinds("run_remove_single") == [(2, R, 2)]
    assert kinds("run_three_isolated") == [(2, R, 3)] and len(decode(M.expected("run_three_isolated")[0])[0][3]) == 3
    assert M.expected("run_emptied")[0] == encode([]) and M.expected("drop_all")[0] == encode([])
    assert kinds("run_grow_past_stage") == [(6, R, 3001)]
    assert kinds("run_maximum") == [(4, R, 32768)] and len(M.expected("run_maximum")[0]) == 4 + 1 + 4 + 131074
    assert [k for k, _, _ in kinds("drop_first")] == [2, 3, 4, 8] and [k for k, _, _ in kinds("drop_last")] == [1, 2, 3, 4]
    assert [k for k, _, _ in kinds("drop_middle_b")] == [1, 3, 4, 8]
    pt = {c[0]: (c[1], c[4]) for c in decode(M.expected("passthrough_three_keys")[0])}
    assert pt[150] == (R, 4096) and pt[152] == (R, 32768) and len(pt) == 300
