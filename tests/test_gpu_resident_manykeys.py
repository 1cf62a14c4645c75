"""Queries on a resident many-key bitmap (csrc/rankdir.hip, csrc/expand.hip) against numpy over its values.

The small-shape files (test_gpu_rankselect.py, test_gpu_tovalues.py) never make a wave or a lane take a
second item, or do so on uniform input alone: k_rd_fill takes a second container per wave above 8,192
containers (the only test that large holds 65,536 one-run containers whose directory entry is 0 whatever the
loop does), k_point takes a second query per lane above 524,288 queries, and k_to_values reaches a second
container per wave for a short window over many small containers or a full expansion of more than 8,192 --
its bitmap path then reuses the wave's LDS stage and its run path searches the per-run directory, both in a
second iteration.  The input is the many-key bitmap of tests/test_manykeys_host.py (9,300 to 9,700 containers,
a heavy one on every 97th key) that tests/test_bsi_manykeys_host.py::resident_input picks: it holds a bitmap
container and a run container of more than 64 runs past container 8,192.
"""
import numpy as np
import pytest

import _oracle as O
import test_manykeys_host as MK
from _fmt import B, R, container_table
from test_bsi_manykeys_host import resident_input, short_window_heavies
from test_gpu_rankselect import OPS, _expect

pytestmark = pytest.mark.gpu

LANES = 2048 * 256  # k_point's grid cap x block: the query at which a lane takes its second one
N_QUERIES = 600_000


@pytest.fixture(scope="module")
def eng(gpu):
    import roaringbitmap_amd as rb
    e = rb.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module", params=MK.SEEDS, ids=[f"seed{x:x}" for x in MK.SEEDS])
def res(request, eng):
    """(inputs, bytes, values, container table, late bitmap / run container indices, resident batch, queries)"""
    s = MK.inputs(request.param)
    _, buf, v, ib, ir = resident_input(request.param)
    keys, kinds, cards, _, lens = container_table(buf)
    cum = np.concatenate([[0], np.cumsum(cards)])
    rng = np.random.default_rng(request.param + 7)
    # the special queries, all at positions >= LANES (a lane's second query)
    xs = []
    for i in (ib, ir):  # every value of the late heavy bitmap and run container, and its neighbours
        cv = v[cum[i]:cum[i + 1]]
        xs += [cv - 1, cv, cv + 1]
    base = keys << 16
    xs += [base, base + 65535, base - 1, base + 65536]  # the ends of every present key
    hole = np.arange(256 * s.hole, 256 * (s.hole + 1), dtype=np.int64) << 16
    xs += [hole, hole + 65535, hole + rng.integers(0, 65536, hole.size)]  # keys of the empty plan workgroup
    xs += [np.array([0, 0xFFFFFFFF, 0xFFFFFFFE, int(v[-1]), int(v[-1]) + 1, int(v[0]) - 1])]  # key 65535 is the last
    xs = np.concatenate(xs)
    xs = xs[(xs >= 0) & (xs <= 0xFFFFFFFF)]
    js = np.concatenate([cum - 1, cum, cum + 1, [v.size - 1, v.size, v.size + 1, 0xFFFFFFFF]])
    js = js[(js >= 0) & (js <= 0xFFFFFFFF)]

    def fill(special, hi):
        n = max(N_QUERIES, LANES + special.size)
        q = rng.integers(0, hi, size=n)
        q[n - special.size:] = rng.permutation(special)
        return q

    xs, js = fill(xs, 1 << 32), fill(js, v.size + 10)
    xs[:LANES:4] = v[rng.integers(0, v.size, LANES // 4)]  # a quarter of the first queries hit a value
    assert xs.size >= N_QUERIES and js.size >= N_QUERIES
    want = {op: _expect(v, op, js if op == "select" else xs) for op in OPS}  # once, shared by every batch and path
    b = eng.load([buf])
    yield dict(s=s, buf=buf, v=v, keys=keys, kinds=kinds, cards=cards, lens=lens, cum=cum, ib=ib, ir=ir, b=b, xs=xs, js=js,
               want=want)
    eng.release(b)


def _point(eng, b, r, device):
    import torch
    for op in OPS:
        q = r["js"] if op == "select" else r["xs"]
        want = r["want"][op]
        if device:
            out = eng.point_query(op, b, torch.from_numpy(q).to(torch.device("cuda", 0)))
            eng.sync()
            got = out.cpu().numpy()
        else:
            got = eng.point_query(op, b, q)
        assert got.dtype == np.int64 and got.shape == want.shape, op
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (op, device, bad.size, [(int(i), int(q[i]), int(got[i]), int(want[i])) for i in bad[:5]])


@pytest.mark.parametrize("device", [False, True], ids=["host", "torch"])
def test_point_queries(eng, res, device):
    """all five ops, 600,000 queries and more in one call: the edge queries sit where a lane takes its
    second query, and the directory they read was filled by waves that took a second container"""
    _point(eng, res["b"], res, device)


def _win(eng, r, first, count, tag):
    got = eng.to_values(r["b"], first=first, count=count)
    want = r["v"][first:first + count].astype(np.uint32)
    assert got.dtype == np.uint32 and got.shape == want.shape, (tag, got.shape, want.shape)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (tag, first, count, [(int(i), int(got[i]), int(want[i])) for i in bad[:5]])


def test_full_expansion(eng, res):
    """more than 8,192 containers of every kind: a wave's second container is a bitmap (the LDS stage
    reused) or a run container (the per-run directory searched) for some wave"""
    import torch
    r = res
    v = r["v"]
    got = eng.to_values(r["b"])
    assert got.dtype == np.uint32 and got.shape == v.shape and np.array_equal(got, v.astype(np.uint32))
    w = eng.to_values(r["b"], dtype=torch.int64)
    assert w.dtype == torch.int64 and np.array_equal(w.cpu().numpy(), v)
    u = eng.to_values(r["b"], dtype=torch.uint32)
    assert np.array_equal(u.cpu().view(torch.int32).numpy().view(np.uint32), v.astype(np.uint32))


def test_short_windows_over_many_containers(eng, res):
    """count <= 256 (one workgroup): the window starts five tiny containers in front of a heavy bitmap / run
    container of the dense middle block, so one wave walks the tiny ones and then the heavy one"""
    r = res
    kinds, cum = r["kinds"], r["cum"]
    heavies = short_window_heavies(r["s"].seed)
    assert set(heavies) == {B, R}
    for h in heavies.values():
        for count in (int(cum[h] - cum[h - 5]) + 100, 256, int(cum[h] - cum[h - 5]) + 1):
            assert count <= 256
            first = int(cum[h - 5]) + (count == 256)
            assert np.unique(r["v"][first:first + count] >> 16).size > 4
            _win(eng, r, first, count, f"kind {kinds[h]} at container {h}")


def test_window_across_late_heavy_containers(eng, res):
    """from the middle of the late bitmap container into the middle of the next heavy run container, and
    windows of 300 from every limit of the host inputs"""
    r = res
    kinds, cards, lens, cum, ib = r["kinds"], r["cards"], r["lens"], r["cum"], r["ib"]
    nxt = next(i for i in range(ib + 1, kinds.size) if kinds[i] == R and (lens[i] - 2) // 4 > 64)
    first = int(cum[ib]) + int(cards[ib]) // 2
    _win(eng, r, first, int(cum[nxt]) + int(cards[nxt]) // 2 - first, "late bitmap to late run")
    _win(eng, r, int(cum[r["ir"]]) + 37, 5000, "inside the late run container")
    for name, n in r["s"].limits.items():
        _win(eng, r, n, 300, f"limit {name}")
        _win(eng, r, max(0, n - 150), 300, f"around limit {name}")


@pytest.mark.parametrize("run_optimize", [False, True], ids=["plain", "ro"])
def test_built_batch(eng, res, run_optimize):
    """from_values of the shuffled, doubled values: the oracle's bytes, and the same answers to the same
    point queries as the loaded batch"""
    r = res
    rng = np.random.default_rng(5)
    b = eng.from_values(rng.permutation(np.repeat(r["v"], 2)), run_optimize)
    got = eng.batch_fetch(b).serialize()
    want = O.from_values(r["v"], run_optimize)
    assert got == want, (len(got), len(want))
    _point(eng, b, r, False)
    eng.release(b)
