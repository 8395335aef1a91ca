"""Surface coatings through the C++ drop-in (tests/cpp/coat_test.cpp): both signatures, the refusals that need no
context and the two host functions; on a GPU box also bzr::traceChainCoated with mask 0 against bzr::traceChainBidir, a
perfect coating, a mirror face and the C ABI on cfg2 at 64 x 64."""
import subprocess

import pytest

from conftest import PKG, REPO


def build(tmp_path):
    exe = tmp_path / "coat_test"
    cmd = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-pthread", str(REPO / "tests" / "cpp" / "coat_test.cpp"),
           f"-I{REPO / 'include' / 'bzr'}", f"-I{REPO / 'include'}", f"-L{PKG / 'lib'}", "-lbzr",
           f"-Wl,-rpath,{PKG / 'lib'}", "-o", str(exe)]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return exe


def test_signatures_refusals_and_host_functions(built, tmp_path):
    exe = build(tmp_path)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "coat (host):" in r.stdout and "0 failed" in r.stdout


@pytest.mark.gpu
def test_trace_chain_coated_with_gpu(built, tmp_path):
    exe = build(tmp_path)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "hot path:" in r.stdout and "0 failed" in r.stdout
