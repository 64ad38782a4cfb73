"""Argument validation of the frame-table calls (rs_frame_matches_*, rs_map_carry_matches, rs_map_refine_pose,
rs_map_match_frame) and of the host mirror's slam::track_tail (racing-slam_amd/host/slam_host.cpp), from C++:
tests/host_cpp/test_track_host.cpp built against librsgpu."""
import os
import subprocess

import pytest

from host_build import build_host_binary

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_track_host(rs):
    return build_host_binary(rs, "test_track_host")


def test_track_host_mirror_compiles(rs):
    assert os.path.exists(build_track_host(rs))


@pytest.mark.gpu
def test_track_calls_refuse_bad_arguments_and_the_mirror_runs(rs):
    r = subprocess.run([build_track_host(rs)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-2000:])
    last = [ln for ln in r.stdout.split("\n") if ln.startswith("track host ok:")]
    assert last and int(last[-1].split(":")[1]) > 60, r.stdout[-2000:]
