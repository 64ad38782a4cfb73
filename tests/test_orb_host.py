"""slam::Session::refresh_descriptors (racing-slam_amd/host/slam_host.cpp) — the C++ host mirror of
OrbFeatureExtractor::refresh_descriptors as Tracker::track_features calls it (reference src/Tracker.cpp:150) — built
against librsgpu and checked against the restatement tests/orb_ref.py on the keypoints the session produced."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import orb_ref as O

from host_build import build_host_binary

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_orb_host(rs):
    return build_host_binary(rs, "test_orb_host")


def test_orb_host_mirror_compiles(rs):
    assert os.path.exists(build_orb_host(rs))


@pytest.mark.gpu
def test_session_refresh_descriptors_matches_the_restatement(rs, tmp_path):
    exe = build_orb_host(rs)
    synth = importlib.import_module("racing-slam_amd").synth
    d = synth.make_klt_pair(1)
    W, H, n = d["width"], d["height"], len(d["pts"])
    (tmp_path / "meta.txt").write_text(f"{W} {H} {n}\n")
    for name, arr in [("img1.u8", d["img1"]), ("img2.u8", d["img2"]), ("mask.u8", d["mask"]), ("pts.f32", d["pts"])]:
        np.ascontiguousarray(arr).tofile(str(tmp_path / name))
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    lines = (tmp_path / "out.txt").read_text().split("\n")
    m, total = (int(v) for v in lines[0].split())
    kp = [ln.split() for ln in lines[1:1 + total]]
    prev_idx = np.array([int(v[0]) for v in kp[:m]], np.int64)
    pts = np.array([[int(v[1], 16), int(v[2], 16)] for v in kp], np.uint32).view(np.float32)
    rows = np.array([list(bytes.fromhex(ln)) for ln in lines[1 + total:1 + 2 * total]], np.uint8).reshape(-1, 32)
    prev = ((np.arange(n)[:, None] + np.arange(32)[None, :] + 1) % 256).astype(np.uint8)
    want = O.refresh(d["img2"], pts[:m], prev_idx, prev, pts[m:])
    assert m > 0 and total > m and want["n"] == total
    assert np.array_equal(rows, want["desc"])
    stale = np.flatnonzero(want["fresh"][:m] == 0)
    assert np.array_equal(rows[stale], prev[prev_idx[stale]])
