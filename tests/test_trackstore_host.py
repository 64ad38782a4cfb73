"""slam::DeviceTracks (racing-slam_amd/host/slam_host.cpp) over a 30-frame synthetic sequence with two key frames against
slam::HostTrackStore, the std::map restatement of TrackStore, from C++: tests/host_cpp/test_trackstore_host.cpp built
against librsgpu."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "host_cpp", "test_trackstore_host.bin")


def build_trackstore_host(rs):
    rs.load()
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    srcs = [os.path.join(ROOT, "tests", "host_cpp", "test_trackstore_host.cpp"), os.path.join(ROOT, "racing-slam_amd", "host", "slam_host.cpp")]
    deps = srcs + [os.path.join(ROOT, "racing-slam_amd", "host", "slam_host.h"), os.path.join(ROOT, "include", "rsgpu.h"),
                   os.path.join(ROOT, "racing-slam_amd", "librsgpu.so")]
    if os.path.exists(BIN) and all(os.path.getmtime(d) <= os.path.getmtime(BIN) for d in deps):
        return BIN
    subprocess.check_call([hipcc, "-O2", "-std=c++17", "-Wall", "-o", BIN] + srcs + [
        "-L" + os.path.join(ROOT, "racing-slam_amd"), "-lrsgpu", "-Wl,-rpath," + os.path.join(ROOT, "racing-slam_amd"), "-lm"])
    return BIN


def test_trackstore_host_mirror_compiles(rs):
    assert os.path.exists(build_trackstore_host(rs))


@pytest.mark.gpu
def test_device_tracks_equal_the_std_map_restatement(rs):
    r = subprocess.run([build_trackstore_host(rs)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-2000:])
    last = [ln for ln in r.stdout.split("\n") if ln.startswith("trackstore host ok:")]
    assert last and int(last[-1].split(":")[1]) > 150, r.stdout[-2000:]
