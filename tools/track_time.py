#!/usr/bin/env python3
"""Time of the tracker's per-frame tail (csrc/frame_matches.hip) at the pass shapes: a frame of 2000 keypoints against a
resident map of 10 000 points in 20 key frames, about 600 matches carried from the previous frame.  Wall clock around
each stage (every stage but the carry-over synchronises once itself; the carry-over is followed by a stream
synchronisation here), median / min of --reps after --warmup:
  (a) the host form at the previous API: walk a host table, build and upload the refit's arrays, rs_refine_pose, then
      rs_map_match twice with the host lists rebuilt from the table in between, and the host fold;
  (b) the new calls: rs_map_carry_matches, rs_map_refine_pose, rs_map_match_frame twice.
Both start every repetition from the same state (form (b) restores the frame's table with rs_frame_matches_clear and
the carry-over; form (a) copies its host table).  The launch counts are those of the library's profiling brackets
(copies and memsets are not launches).

    python tools/track_time.py [--reps 200] [--warmup 20] [--json profiles/track_time.json]
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def stats(ts):
    return dict(median_us=round(float(np.median(ts)) * 1e6, 1), min_us=round(float(np.min(ts)) * 1e6, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--keypoints", type=int, default=2000)
    ap.add_argument("--points", type=int, default=10000)
    ap.add_argument("--carried", type=int, default=600)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import track_ref as T
    pkg = importlib.import_module("racing-slam_amd")
    rs, synth = pkg.rsgpu, pkg.synth
    ctx = rs.Context(0)
    w = synth.make_ba_window(n_kf=20, n_points=a.points, config_id=3)
    frame, mp = synth.make_match_scene(w, n_keypoints=a.keypoints, kdtree_build=rs.kdtree_build, config_id=3)
    m = rs.ResidentMap(ctx)
    obs_pt = np.repeat(np.arange(a.points), np.diff(w["obs_ptr"]))
    pool = mp["desc_pool"][mp["obs_desc"]]
    kp_index = np.zeros(len(obs_pt), np.int64)
    for k in range(20):
        sel = np.flatnonzero(w["obs_cam"] == k)
        kp_index[sel] = np.arange(len(sel))
        f = rs.ResidentFrame(ctx, w["obs_uv"][sel], pool[sel])
        m.add_keyframe(f, w["poses_true"][k].astype(np.float32))
        f.close()
    for p in range(a.points):
        m.add_point(mp["positions"][p])
        for o in range(w["obs_ptr"][p], w["obs_ptr"][p + 1]):
            m.add_observation(p, int(w["obs_cam"][o]), int(kp_index[o]))
    K, W, H, pose = w["K"], frame["width"], frame["height"], frame["pose"]
    N = a.keypoints
    nxt = rs.ResidentFrame(ctx, frame["keypoints"], frame["descriptors"])
    prev = rs.ResidentFrame(ctx, frame["keypoints"], frame["descriptors"])
    # the carried matches: what a first whole-map match finds, cut to --carried; prev holds them at the same keypoints
    mk, mpt = m.match(nxt, pose, K, W, H)
    mk, mpt = mk[:a.carried], mpt[:a.carried]
    base = np.full(N, -1, np.int32)
    base[mk] = mpt
    prev.matches_add(ctx.dev(mk), ctx.dev(mpt))
    d_index = ctx.dev(np.arange(N, dtype=np.int32))
    cam0 = rs.pack_pose(np.asarray(pose, np.float32).reshape(4, 4))
    pos = np.asarray(mp["positions"], np.float32)
    n_obs = np.diff(w["obs_ptr"])
    alive = np.ones(a.points, np.uint8)
    last_kf = 19

    def form_a(t):
        table = base.copy()
        t0 = time.perf_counter()
        pts, uv, n = T.gather(table, frame["keypoints"], alive, n_obs, pos)          # the walk over the host table
        cam, s = ctx.refine_pose(cam0, ctx.dev(pts), ctx.dev(uv), K)
        t1 = time.perf_counter()
        for i, req in enumerate((last_kf, -1)):
            matched, mpts = T.match_inputs(table)
            k_, p_ = m.match(nxt, pose, K, W, H, kp_matched=matched, matched_points=mpts, required_observer=req)
            table[k_] = p_                                                         # the fold (pairs are disjoint and unique)
        t2 = time.perf_counter()
        t["refine"].append(t1 - t0); t["match_x2"].append(t2 - t1); t["total"].append(t2 - t0)
        return table, cam

    def form_b(t):
        nxt.matches_clear()
        ctx.synchronize()
        t0 = time.perf_counter()
        m.carry_matches(prev, nxt, d_index, None, None, N, 15)
        ctx.synchronize()
        t1 = time.perf_counter()
        cam, _, s, used = m.refine_pose(nxt, cam0, K)
        t2 = time.perf_counter()
        m.match_frame(nxt, pose, K, W, H, required_observer=last_kf)
        m.match_frame(nxt, pose, K, W, H, required_observer=-1)
        t3 = time.perf_counter()
        t["carry"].append(t1 - t0); t["refine"].append(t2 - t1); t["match_x2"].append(t3 - t2); t["total"].append(t3 - t0)
        return cam

    out = dict(reps=a.reps, warmup=a.warmup, keypoints=N, points=a.points, carried=int(len(mk)))
    for name, fn in (("host_form", form_a), ("device_form", form_b)):
        for _ in range(a.warmup):
            fn(dict(carry=[], refine=[], match_x2=[], total=[]))
        t = dict(carry=[], refine=[], match_x2=[], total=[])
        for _ in range(a.reps):
            fn(t)
        out[name] = {k: stats(v) for k, v in t.items() if v}
        ctx.prof_begin()                  # a short pass of its own: the brackets' events cost time
        for _ in range(10):
            fn(dict(carry=[], refine=[], match_x2=[], total=[]))
        prof = ctx.prof_end()
        out[name]["bracketed_launches_per_frame"] = round(sum(v[0] for v in prof.values()) / 10, 2)
        out[name]["kernels_mean_us"] = {k: round(1e3 * v[1] / max(v[0], 1), 1) for k, v in prof.items()}
    table_a, cam_a = form_a(dict(carry=[], refine=[], match_x2=[], total=[]))
    cam_b = form_b(dict(carry=[], refine=[], match_x2=[], total=[]))
    out["same_table"] = bool(np.array_equal(nxt.matches()[0], table_a))
    out["same_camera"] = bool(cam_a.tobytes() == cam_b.tobytes())
    print(json.dumps(out, indent=1))
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
