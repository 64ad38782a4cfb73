#!/usr/bin/env python3
"""Time of the two device stages of Mapper::insert on the resident map (csrc/map_keyframe.hip) on a map of 20 key frames x
2000 keypoints and 10000 points, in one run on one GPU.  Medians of --reps after warm-up.

  (a) forms     rs_map_reanchor and rs_map_cull_points (apply = 0, so that every repetition sees the same map) against the
                host forms they replace, both from C++ in ONE process (tests/host_cpp/test_keyframe_host.bin --time): the walk
                over the caller's own objects that builds the lists / the CSR, the upload, rs_reanchor_points_host_poses /
                rs_point_errors, the read-back and, for the re-anchoring, the rs_map_set_position loop.  Wall clock around a
                synchronised call.  Not in the host numbers: the full re-upload of the positions that the set_position loop
                causes at the map's next use.  The removal changes the map, so it cannot be repeated: cull_apply_once_* is ONE
                run each of rs_map_cull_points(apply = 1) and of the host form followed by its rs_map_remove_point loop, on two
                identical maps (a single sample, not a median).
  (b) kernels   mean device time per kernel from the library's own event brackets (rs_prof_begin / rs_prof_end) on a map of
                the same size built through the Python binding: KF1_map_reanchor, KF2_map_cull and KF3_map_compact, the
                one-workgroup ordered compaction both calls end with.

    python tools/keyframe_time.py [--reps 200] [--json profiles/keyframe_time.json]
"""
import argparse
import importlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    pkg = importlib.import_module("racing-slam_amd")
    rs = pkg.rsgpu
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_keyframe_host
    out = subprocess.run([test_keyframe_host.build_keyframe_host(rs), "--time", str(a.reps)], capture_output=True, text=True, timeout=900)
    line = [ln for ln in out.stdout.split("\n") if ln.startswith("{")]
    assert out.returncode == 0 and line, (out.stdout[-2000:], out.stderr[-2000:])
    res = dict(forms=json.loads(line[-1]))
    # (b) the kernels alone
    ctx = rs.Context(0)
    KF, n, P = 20, 2000, 10000
    K = (1000.0, 1000.0, 960.0, 540.0)
    rng = np.random.default_rng(5)
    m = rs.ResidentMap(ctx)
    X = np.stack([rng.uniform(-4, 6, P), rng.uniform(-2, 2, P), rng.uniform(4, 9, P)], axis=1).astype(np.float32)
    kp = np.zeros((KF, n, 2), np.float32)
    nxt, obs = [0] * KF, []
    for p in range(P):
        k0, ln = int(rng.integers(KF)), 1 + int(rng.integers(6))
        for k in range(k0, min(KF, k0 + ln)):
            if nxt[k] < n:
                kp[k, nxt[k]] = (K[0] * (X[p, 0] - 0.1 * k) / X[p, 2] + K[2] + rng.uniform(-0.5, 0.5), K[1] * X[p, 1] / X[p, 2] + K[3] + rng.uniform(-0.5, 0.5))
                obs.append((p, k, nxt[k]))
                nxt[k] += 1
    poses = np.tile(np.eye(4, dtype=np.float32), (KF, 1, 1))
    for k in range(KF):
        poses[k, 0, 3] = -0.1 * k
        f = rs.ResidentFrame(ctx, kp[k], np.zeros((n, 32), np.uint8))
        m.add_keyframe(f, poses[k])
        f.close()
    for p in range(P):
        m.add_point(X[p])
    for p, k, i in obs:
        m.add_observation(p, k, i)
    kfs = list(range(1, KF))
    before = poses[1:].reshape(-1, 16)
    for _ in range(5):
        m.reanchor(kfs, before)
        m.cull_points(list(range(KF)), K, apply=False)
    ctx.prof_begin()
    for _ in range(a.reps):
        moved = m.reanchor(kfs, before)[0]
        r = m.cull_points(list(range(KF)), K, apply=False)
    prof = ctx.prof_end()
    res["kernels_mean_us"] = {k: round(1e3 * ms / max(cnt, 1), 1) for k, (cnt, ms) in prof.items() if k.startswith("KF")}
    res["kernels_map"] = dict(key_frames=KF, keypoints=n, points=P, observations=len(obs), moved=moved, local=r["n_local"], culled=r["n_removed"])
    m.close()
    ctx.close()
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as fo:
            json.dump(res, fo, indent=1)


if __name__ == "__main__":
    main()
