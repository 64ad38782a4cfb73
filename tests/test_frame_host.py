"""slam::Session::refresh_descriptors with its device-built rs_frame (racing-slam_amd/host/slam_host.cpp) — the C++ host
mirror's entry to rs_frame_assign_device — built against librsgpu.  The self-test (tests/host_cpp/test_frame_host.cpp)
compares, over two video frames, the session's frame with rs_frame_create on the same keypoints and rows: equal bytes in
rs_frame_download and equal rs_map_match results."""
import importlib
import os
import subprocess

import numpy as np
import pytest

from host_build import build_host_binary

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_frame_host(rs):
    return build_host_binary(rs, "test_frame_host")


def test_frame_host_mirror_compiles(rs):
    assert os.path.exists(build_frame_host(rs))


@pytest.mark.gpu
def test_session_device_frame_equals_the_host_built_frame(rs, tmp_path):
    exe = build_frame_host(rs)
    synth = importlib.import_module("racing-slam_amd").synth
    d = synth.make_klt_pair(1)
    W, H, n = d["width"], d["height"], len(d["pts"])
    (tmp_path / "meta.txt").write_text(f"{W} {H} {n}\n")
    for name, arr in [("img1.u8", d["img1"]), ("img2.u8", d["img2"]), ("mask.u8", d["mask"]), ("pts.f32", d["pts"])]:
        np.ascontiguousarray(arr).tofile(str(tmp_path / name))
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    last = [ln for ln in r.stdout.split("\n") if ln.startswith("frame host ok:")]
    assert last, r.stdout[-2000:]
    n1, m1, n2, m2 = (int(v) for v in last[-1].split(":")[1].split())
    # both video frames held a real frame and a real match: the equalities checked in the binary were not vacuous
    assert n1 > 500 and n2 > 500 and m1 > n1 // 6 and m2 > n2 // 6
