"""Host AddressSanitizer / UBSan run of the range-encoded index's emitter
(roaringbitmap_amd/csrc/rangebitmap_format.cpp: rb_emit, the inverse of rb_relay).

tests/asan/rangebitmap_emit.cpp, a stand-alone program, runs parse, re-lay and emit over the streams of
test_rangebitmap_build_host.py and their truncations and compares the emitted bytes with the parsed ones; a
heap overflow, use-after-free or undefined behaviour aborts the run.  Sanitizers run on host code only."""
import os
import shutil
import subprocess

import pytest

from test_rangebitmap_build_host import STREAMS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def emit_bin(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    out = str(tmp_path_factory.mktemp("asan") / "rangebitmap_emit")
    cmd = [gxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "asan", "rangebitmap_emit.cpp"),
           os.path.join(ROOT, "roaringbitmap_amd", "csrc", "rangebitmap_format.cpp"), "-o", out]
    subprocess.run(cmd, check=True, capture_output=True)
    return out


def test_rangebitmap_emit_under_asan(emit_bin, tmp_path):
    files = []
    for name, buf in STREAMS.items():
        p = tmp_path / f"{name}.rangebitmap"
        p.write_bytes(buf)
        files.append(str(p))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([emit_bin] + files, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "\n0 failures" in r.stdout
