"""Surrounding media through the C++ drop-in (tests/cpp/media_test.cpp): the header's constants, both signatures and the
gapTable size check on the host; on a GPU box also bzr::traceChainMedia against the C ABI's bzr_trace_chain_media on cfg2
at 64 x 64, bit for bit."""
import subprocess

import pytest

from conftest import PKG, REPO


def build(tmp_path):
    exe = tmp_path / "media_test"
    cmd = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-pthread", str(REPO / "tests" / "cpp" / "media_test.cpp"),
           f"-I{REPO / 'include' / 'bzr'}", f"-I{REPO / 'include'}", f"-L{PKG / 'lib'}", "-lbzr",
           f"-Wl,-rpath,{PKG / 'lib'}", "-o", str(exe)]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return exe


def test_constants_and_signatures_on_the_host(built, tmp_path):
    exe = build(tmp_path)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "media (host):" in r.stdout and "0 failed" in r.stdout


@pytest.mark.gpu
def test_trace_chain_media_with_gpu(built, tmp_path):
    exe = build(tmp_path)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "hot path:" in r.stdout and "0 failed" in r.stdout
