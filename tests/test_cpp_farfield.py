"""Far-field maps through the C++ drop-in (tests/cpp/farfield_test.cpp): the signatures, the frame checks and the host
helpers on the host; on a GPU box also bzr::farfieldBin over 5 000 rays against bzr_farfield_cell per ray, word for
word."""
import subprocess

import pytest

from conftest import PKG, REPO


def build(tmp_path):
    exe = tmp_path / "farfield_test"
    cmd = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-pthread", str(REPO / "tests" / "cpp" / "farfield_test.cpp"),
           f"-I{REPO / 'include' / 'bzr'}", f"-I{REPO / 'include'}", f"-L{PKG / 'lib'}", "-lbzr",
           f"-Wl,-rpath,{PKG / 'lib'}", "-o", str(exe)]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return exe


def test_signatures_and_host_helpers(built, tmp_path):
    exe = build(tmp_path)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "farfield (host):" in r.stdout and "0 failed" in r.stdout


@pytest.mark.gpu
def test_farfield_bin_with_gpu(built, tmp_path):
    exe = build(tmp_path)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "hot path:" in r.stdout and "0 failed" in r.stdout
