"""The float sums of joint_tensorf_amd/csrc/jt_lds_sum.h (what RecWalker::flush_lds runs on its LDS line) instantiated on the
host for std::atomic<uint32_t>: tests/csrc/lds_sum_host.cpp, a stand-alone program, adds integer-valued floats from twelve
threads into 1 .. 36 cells through the compare-and-swap and the exchange form, their one-round twins (which take the
float-atomic fallback whenever another thread gets in between), the fallback alone, and all of them at once, spread over the
cells and all on one cell.  Every total is exact.  The program is built and run twice: plainly, and under ThreadSanitizer."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "csrc", "lds_sum_host.cpp")
INC = os.path.join(ROOT, "joint_tensorf_amd", "csrc")


def _cxx():
    for c in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if c and shutil.which(c):
            return shutil.which(c)
    raise RuntimeError("no C++ compiler found")


@pytest.mark.parametrize("name,flags,adds", [("plain", ["-O2"], 20000), ("tsan", ["-O1", "-g", "-fsanitize=thread"], 4000)])
def test_host_sums_are_exact(tmp_path, name, flags, adds):
    exe = str(tmp_path / ("lds_sum_host_" + name))
    subprocess.check_call([_cxx(), "-std=c++17", "-pthread", "-I", INC] + flags + [SRC, "-o", exe])
    r = subprocess.run([exe, str(adds)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    if "unexpected memory mapping" in r.stdout and shutil.which("setarch"):
        # the sanitizer runtime of older compilers cannot place its shadow under a kernel with 32 bits of mmap randomisation
        # and says so before main(): the same program once more with address-space randomisation off for this one process
        r = subprocess.run(["setarch", os.uname().machine, "-R", exe, str(adds)], stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    assert "0 wrong" in r.stdout and "ThreadSanitizer" not in r.stdout, r.stdout
