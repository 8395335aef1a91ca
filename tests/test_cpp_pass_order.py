"""The fused pass loop's near-first order on the host (tests/cpp/pass_order_test.cpp over csrc/device/pass_order.hpp):
the order word kept up while a batch's entries arrive is the stable ascending order of their keys -- exhaustively for
every sequence of up to 6 keys over 3 distinct values, and for full 16-entry batches."""
import subprocess

from conftest import PKG, REPO


def test_insertion_keeps_the_stable_order(tmp_path):
    exe = tmp_path / "pass_order_test"
    cmd = ["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", str(REPO / "tests" / "cpp" / "pass_order_test.cpp"),
           f"-I{PKG / 'csrc' / 'device'}", "-o", str(exe)]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "pass order (host):" in r.stdout and " 0 failed" in r.stdout
