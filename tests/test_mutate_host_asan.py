"""Host AddressSanitizer / UBSan run of the host form of the point mutations
(roaringbitmap_amd/csrc/mutate_host.cpp, over the format layer format.cpp).

tests/asan/mutate_fuzz.cpp, a stand-alone program with its own main, applies random and hand-made batches of
adds and of removes to the reference's data files (the golden bitmaps and the crashproneinput*.bin adversarial
inputs) and to truncated copies of them; a heap overflow, use-after-free or undefined behaviour aborts the
run.  Sanitizers run on host code only: nothing is loaded into python."""
import glob
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "testdata")
CSRC = os.path.join(ROOT, "roaringbitmap_amd", "csrc")


@pytest.fixture(scope="module")
def fuzz_bin(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    out = str(tmp_path_factory.mktemp("asan") / "mutate_fuzz")
    cmd = [gxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "asan", "mutate_fuzz.cpp"),
           os.path.join(CSRC, "mutate_host.cpp"), os.path.join(CSRC, "format.cpp"), "-o", out]
    subprocess.run(cmd, check=True, capture_output=True)
    return out


def test_mutate_host_form_under_asan(fuzz_bin):
    files = sorted(glob.glob(os.path.join(GOLD, "*.bin")))
    assert any(os.path.basename(f).startswith("bitmapwith") for f in files)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([fuzz_bin] + files, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "\n0 failures" in r.stdout
