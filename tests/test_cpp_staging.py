"""The staging carve on host memory (tests/cpp/staging_test.cpp, which includes csrc/host/staging.hpp alone): built and run
once with g++ and once as a stand-alone ASan + UBSan executable with the clang++ of the Makefile's asan target."""
import re
import subprocess

import pytest

from conftest import PKG, REPO


def asan_cxx():
    m = re.search(r"VARIANT=asan CXX=(\S+)", (PKG / "Makefile").read_text())
    assert m, "the Makefile's asan target names no compiler"
    return m.group(1)


@pytest.mark.parametrize("sanitize", [False, True], ids=["gxx", "clang_asan_ubsan"])
def test_staging_carve(tmp_path, sanitize):
    exe = tmp_path / "staging_test"
    cxx = [asan_cxx(), "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer"] if sanitize else ["g++"]
    cmd = cxx + ["-O1", "-std=c++17", "-Wall", "-Wextra", str(REPO / "tests" / "cpp" / "staging_test.cpp"),
                 f"-I{PKG / 'csrc' / 'host'}", "-o", str(exe)]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "staging (host): 0 failed" in r.stdout
