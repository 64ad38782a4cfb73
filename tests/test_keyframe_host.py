"""slam::insert_key_frame (racing-slam_amd/host/slam_host.cpp: Mapper::insert on the resident map) over a 31-frame synthetic
sequence with four key frames, from C++: tests/host_cpp/test_keyframe_host.cpp built against librsgpu.  The driver holds the
chain against the host form on a second map; its dump of every key frame's inputs and results is replayed here in
tests/keyframe_ref.py with the oracle's arithmetic, fed with the poses and points rs_map_bundle_adjust returned.  The mirror
edits' index arithmetic runs under the address sanitizer in a host-only program (tests/host_cpp/asan_keyframe.cpp)."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from host_build import build_host_binary

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_keyframe_host(rs):
    return build_host_binary(rs, "test_keyframe_host")


def test_keyframe_host_mirror_compiles(rs):
    assert os.path.exists(build_keyframe_host(rs))


def test_mirror_edits_under_address_sanitizer():
    """csrc/map_mirror.h (the mirror edits of rs_map_insert_keyframe and rs_map_add_track_points; no GPU code in it) built
    with -fsanitize=address,undefined into a program of its own and driven with exactly-sized heap buffers.  A missing
    compiler fails the test: it never passes without having run."""
    # any host C++ compiler with the sanitizers: g++, or the clang++ that hipcc drives (the library cannot be built without it)
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    rocm_clang = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "lib", "llvm", "bin", "clang++")
    found = [c for c in (shutil.which("g++"), shutil.which("clang++"), rocm_clang, "/opt/rocm/lib/llvm/bin/clang++") if c and os.path.exists(c)]
    assert found, "no host C++ compiler (g++ or clang++) to build the sanitizer program with"
    gxx = found[0]
    exe = os.path.join(ROOT, "tests", "host_cpp", "asan_keyframe.bin")
    subprocess.check_call([gxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-o", exe, os.path.join(ROOT, "tests", "host_cpp", "asan_keyframe.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "asan keyframe checks passed" in r.stdout


def f32(words):
    return np.array(words, np.uint32).view(np.float32)


@pytest.mark.gpu
def test_insert_key_frame_equals_the_host_form_and_the_restatement(rs, oracle, tmp_path):
    import keyframe_ref as R
    from map_model import MapModel
    dump = str(tmp_path / "keyframes.jsonl")
    r = subprocess.run([build_keyframe_host(rs), "--dump", dump], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-2000:])
    last = [ln for ln in r.stdout.split("\n") if ln.startswith("keyframe host ok:")]
    assert last and int(last[-1].split(":")[1]) > 100, r.stdout[-2000:]
    # the same key frames through keyframe_ref, with the oracle's arithmetic
    K = (1000.0, 1000.0, 960.0, 540.0)
    model = MapModel()
    frames = [json.loads(ln) for ln in open(dump)]
    assert len(frames) == 4
    culled = reanchored = 0
    for fr in frames:
        n = fr["n"]
        kf, _ = model.add_keyframe(f32(fr["keypoints"]).reshape(n, 2), np.zeros((n, 32), np.uint8), f32(fr["pose"]))
        assert kf == fr["key_frame"] and R.adopt(model, kf, fr["table"]) == fr["adopted"]
        res = dict(keypoint=fr["acc_keypoint"], xyz=f32(fr["acc_xyz"]).reshape(-1, 3), sightings=fr["acc_sightings"], kf_ptr=fr["acc_kf_ptr"],
                   kf_pairs=np.array(fr["acc_kf_pairs"], np.int32).reshape(-1, 2))
        assert R.add_track_points(model, kf, res, fr["window"][:-1])[0] == fr["created"]
        before = f32(fr["before"]).reshape(-1, 16)
        for k, T in zip(fr["window"], f32(fr["poses"]).reshape(-1, 16)):            # the adjustment's result, as returned
            model.set_pose(k, T)
        for p, x in zip(fr["adjusted"], f32(fr["adjusted_xyz"]).reshape(-1, 3)):
            model.set_position(p, x)
        pts, xyz = R.reanchor(model, fr["anchors"], before, oracle)
        assert pts.tolist() == fr["reanchored"] and xyz.tobytes() == f32(fr["reanchored_xyz"]).tobytes()
        want = R.cull(model, fr["window"], K, oracle, apply=True)
        assert want["removed"].tolist() == fr["culled"] and want["xyz"].tobytes() == f32(fr["culled_xyz"]).tobytes()
        assert len(want["local"]) == fr["local_points"]
        c = model.counts()
        assert [c["slots"], c["alive"], c["observations"], c["key_frames"]] == fr["counts"]
        assert model.positions().tobytes() == f32(fr["positions"]).tobytes()
        culled += len(fr["culled"])
        reanchored += len(fr["reanchored"])
    assert culled > 5 and reanchored > 20 and frames[-1]["usable"] == 1
