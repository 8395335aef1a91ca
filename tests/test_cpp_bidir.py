"""The bidirectional chain through the C++ drop-in (tests/cpp/bidir_test.cpp): both signatures, the refusals that need no
context and bzr_bidir_uniform on the host; on a GPU box also bzr::traceChainBidir at budget 0 against
bzr::traceChainAbsorb, its determinism, the BACK rays, the weight invariant and the C ABI on cfg2 at 64 x 64."""
import subprocess

import pytest

from conftest import PKG, REPO


def build(tmp_path):
    exe = tmp_path / "bidir_test"
    cmd = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-pthread", str(REPO / "tests" / "cpp" / "bidir_test.cpp"),
           f"-I{REPO / 'include' / 'bzr'}", f"-I{REPO / 'include'}", f"-L{PKG / 'lib'}", "-lbzr",
           f"-Wl,-rpath,{PKG / 'lib'}", "-o", str(exe)]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return exe


def test_signatures_and_host_draw(built, tmp_path):
    exe = build(tmp_path)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "bidir (host):" in r.stdout and "0 failed" in r.stdout


@pytest.mark.gpu
def test_trace_chain_bidir_with_gpu(built, tmp_path):
    exe = build(tmp_path)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "hot path:" in r.stdout and "0 failed" in r.stdout
