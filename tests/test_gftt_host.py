"""slam::Session::replenish_features (racing-slam_amd/host/slam_host.cpp) — the C++ host mirror of Tracker::track_features'
replenishment (reference src/Tracker.cpp:127-146) — built against librsgpu and checked against the restatements
tests/klt_ref.py and tests/gftt_ref.py."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import gftt_ref as G
import klt_ref as K

from host_build import build_host_binary

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_gftt_host(rs):
    return build_host_binary(rs, "test_gftt_host")


def test_gftt_host_mirror_compiles(rs):
    assert os.path.exists(build_gftt_host(rs))


def _read(path):
    lines = open(path).read().split("\n")
    detected, appended, total = (int(v) for v in lines[0].split())
    rows = np.array([[int(v, 16) for v in ln.split()] for ln in lines[1:1 + appended]], np.uint32).reshape(-1, 3)
    return detected, appended, total, rows[:, :2].copy().view(np.float32), rows[:, 2].copy().view(np.float32)


@pytest.mark.gpu
def test_session_replenish_features_matches_the_restatement(rs, tmp_path):
    exe = build_gftt_host(rs)
    synth = importlib.import_module("racing-slam_amd").synth
    d = synth.make_klt_pair(1)
    W, H, n = d["width"], d["height"], len(d["pts"])
    (tmp_path / "meta.txt").write_text(f"{W} {H} {n}\n")
    for name, arr in [("img1.u8", d["img1"]), ("img2.u8", d["img2"]), ("mask.u8", d["mask"]), ("pts.f32", d["pts"])]:
        np.ascontiguousarray(arr).tofile(str(tmp_path / name))
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    kt = K.track_features(K.build_pyramid(d["img1"]), K.build_pyramid(d["img2"]), d["pts"], d["mask"])
    m = len(kt["index"])
    want = [G.detect_features(d["img2"], d["mask"], kt["pts"], max_total=2000), G.detect_features(d["img1"], d["mask"])]
    totals = [m + want[0]["appended"], want[1]["detected"]]
    for call, ref in enumerate(want):
        detected, appended, total, pts, resp = _read(str(tmp_path / f"out_{call}.txt"))
        assert (detected, appended, total) == (ref["detected"], ref["appended"], totals[call]), call
        assert np.array_equal(pts.view(np.uint32), ref["pts"][:appended].view(np.uint32)), call
        assert np.array_equal(resp.view(np.uint32), ref["response"][:appended].view(np.uint32)), call
    assert want[0]["appended"] == min(want[0]["detected"], 2000 - m) and want[0]["appended"] > 0
