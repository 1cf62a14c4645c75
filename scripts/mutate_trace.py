"""The 2^10 clustered delta of scripts/mutate_perf.py on its dense256 and sparse64k operands, add and remove, 300
calls of Engine.mutate_values + release each and nothing else: the process to put under
rocprofv3 --kernel-trace --stats (profiles/mutate/mutate_kernel_times.txt)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from roaringbitmap_amd import Engine  # noqa: E402

eng = Engine(0)
dev = torch.device("cuda", 0)
g = torch.Generator(device=dev)
g.manual_seed(1)
i = torch.arange(1 << 24, device=dev, dtype=torch.int64)
for name, vals, keys in (("dense256", i[(i & 3) != 3], 256), ("sparse64k", i * 256, 65536)):
    op = eng.from_values(vals)
    v = ((keys // 2 - 4) << 16) + torch.randint(0, 8 << 16, (1 << 10,), generator=g, device=dev, dtype=torch.int64)
    for remove in (False, True):
        for _ in range(300):
            eng.release(eng.mutate_values(op, v, remove)[0])
    eng.release(op)
print("trace run done")
