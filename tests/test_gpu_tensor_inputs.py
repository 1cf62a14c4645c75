"""What the session API's torch paths accept and refuse (Engine._words, Engine._pairs): the dtypes of point_query
and from_values against those of the BSI calls, and a tensor that is not on the engine's GPU.  Four-element
tensors; the refusals come before any library call."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COLS, VALS = [1, 2, 3, 70000], [5, 0, 7, 9]


@pytest.fixture(scope="module")
def eng(gpu):
    import roaringbitmap_amd as rb
    e = rb.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def index(eng):
    batch, nbits, mn, mx = eng.bsi_from_columns(COLS, VALS)
    assert (nbits, mn, mx) == (4, 0, 9)
    yield batch
    eng.release(batch)


def test_point_query_refuses_int32(eng, index):
    import torch
    with pytest.raises(ValueError, match="point_query: an int64 or uint32 tensor is required"):
        eng.point_query("rank", index, torch.tensor(COLS, dtype=torch.int32, device="cuda:0"))


def test_bsi_get_values_takes_int32(eng, index):
    import torch
    got = eng.bsi_get_values(index, 4, torch.tensor([1, 2, 70000, 4], dtype=torch.int32, device="cuda:0"))
    assert got.dtype == torch.int64 and got.cpu().tolist() == [5, 0, 9, -1]


def _torch_paths(eng, index, t):
    return {"point_query": lambda: eng.point_query("rank", index, t),
            "from_values": lambda: eng.from_values(t),
            "bsi_from_columns": lambda: eng.bsi_from_columns(t, t),
            "bsi_set_values": lambda: eng.bsi_set_values(index, 4, t, t, 0, 9),
            "bsi_get_values": lambda: eng.bsi_get_values(index, 4, t)}


@pytest.mark.parametrize("what", ["point_query", "from_values", "bsi_from_columns", "bsi_set_values",
                                  "bsi_get_values"])
def test_cpu_tensor_is_refused(eng, index, what):
    import torch
    t = torch.from_numpy(np.array(COLS, dtype=np.int64))
    noun = "query tensor" if what == "point_query" else "tensor"
    with pytest.raises(ValueError, match=f"{what}: the {noun} must be on device 0"):
        _torch_paths(eng, index, t)[what]()
