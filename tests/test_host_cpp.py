"""The C++ host mirror (racing-slam_amd/host/) over the C-ABI: compile on the CPU (always),
run its self-test against the oracle on the GPU."""
import os
import shutil
import subprocess

import pytest

from host_build import build_host_binary

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_host_test(rs, oracle):
    return build_host_binary(rs, "test_host", oracle)


def build_boundary_bench(rs):
    """tests/host_cpp/bench_boundary.cpp: the caller's view of the drop-in (host objects in, host results out), timed.
    No oracle in it: it is a measurement of the product path (bench.py --boundary runs it)."""
    return build_host_binary(rs, "bench_boundary")


def test_host_mirror_compiles_and_links(rs, oracle):
    assert os.path.exists(build_host_test(rs, oracle))
    assert os.path.exists(build_boundary_bench(rs))


@pytest.mark.gpu
def test_host_mirror_selftest(rs, oracle):
    exe = build_host_test(rs, oracle)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0, r.stdout[-3000:]
    assert "all checks passed" in r.stdout


def test_host_only_entry_points_under_address_sanitizer():
    """csrc/host.cpp + csrc/pose_graph.cpp (no GPU code in them) built with g++ -fsanitize=address and driven with
    exactly-sized heap buffers: out-of-bounds reads that only crash under another heap layout abort here."""
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    exe = os.path.join(ROOT, "tests", "host_cpp", "asan_host.bin")
    srcs = [os.path.join(ROOT, "tests", "host_cpp", "asan_host.cpp"), os.path.join(ROOT, "racing-slam_amd", "csrc", "host.cpp"),
            os.path.join(ROOT, "racing-slam_amd", "csrc", "pose_graph.cpp")]
    subprocess.check_call([gxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-ffp-contract=off",
                           "-o", exe] + srcs + ["-lm"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "asan host checks passed" in r.stdout
