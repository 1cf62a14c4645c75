"""Host AddressSanitizer / UBSan run of the range-encoded index's format layer
(roaringbitmap_amd/csrc/rangebitmap_format.cpp).

tests/asan/rangebitmap_fuzz.cpp, a stand-alone program, feeds serialized indexes written by the oracle's
Appender, their truncations and seeded byte mutations through the parser and the re-lay of the containers; a
heap overflow, use-after-free or undefined behaviour aborts the run.  Sanitizers run on host code only."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import _rangebitmap as RBO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fuzz_bin(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    out = str(tmp_path_factory.mktemp("asan") / "rangebitmap_fuzz")
    cmd = [gxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "asan", "rangebitmap_fuzz.cpp"),
           os.path.join(ROOT, "roaringbitmap_amd", "csrc", "rangebitmap_format.cpp"), "-o", out]
    subprocess.run(cmd, check=True, capture_output=True)
    return out


def streams():
    rng = np.random.default_rng(11)
    mixed = np.where(rng.random(65536 + 70) < 0.03, rng.integers(0, 1 << 9, 65536 + 70), 511)
    mixed[10000:20000:2] &= 0x1FE  # array, bitmap and run records, two blocks
    return {"empty": RBO.Appender(1000).serialize(),
            "tiny": RBO.build([3, 1, 2, 0], 3),
            "wide": RBO.build([0, (1 << 64) - 1, 1 << 63, 12345], (1 << 64) - 1),
            "five_byte_mask": RBO.build(rng.integers(0, 1 << 33, 200), (1 << 33) - 1),
            "mixed": RBO.build(mixed, 511)}


def test_rangebitmap_format_layer_under_asan(fuzz_bin, tmp_path):
    files = []
    for name, buf in streams().items():
        p = tmp_path / f"{name}.rangebitmap"
        p.write_bytes(buf)
        files.append(str(p))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([fuzz_bin] + files, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "\n0 failures" in r.stdout
