"""slam::DeviceTracks (racing-slam_amd/host/slam_host.cpp) over a 30-frame synthetic sequence with two key frames against
slam::HostTrackStore, the std::map restatement of TrackStore, from C++: tests/host_cpp/test_trackstore_host.cpp built
against librsgpu."""
import os
import subprocess

import pytest

from host_build import build_host_binary

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_trackstore_host(rs):
    return build_host_binary(rs, "test_trackstore_host")


def test_trackstore_host_mirror_compiles(rs):
    assert os.path.exists(build_trackstore_host(rs))


@pytest.mark.gpu
def test_device_tracks_equal_the_std_map_restatement(rs):
    r = subprocess.run([build_trackstore_host(rs)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-2000:])
    last = [ln for ln in r.stdout.split("\n") if ln.startswith("trackstore host ok:")]
    assert last and int(last[-1].split(":")[1]) > 150, r.stdout[-2000:]
