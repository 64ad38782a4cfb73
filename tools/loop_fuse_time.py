#!/usr/bin/env python3
"""Time of one rs_map_fuse_loop (csrc/map_fuse.hip) against the host form it replaces, in one run on one GPU.

Shape: a 20-frame window of 2000-keypoint key frames, about 10 000 points, about 1500 sources (tests/fuse_cases.loop_scene;
the new key frames share fewer than 15 points with the candidate, so none of them is an old frame; the JSON records the
old frames, sources and outcomes that came out).
A fuse edits the map, so every repetition runs on a map built anew; medians over --reps repetitions after --warmup, wall
clock around a call that ends synchronised (the journal read-back), both forms in one process, alternating.

  device   one rs_map_fuse_loop (check off, journal wanted) through the Python binding, on a map whose image is current: the
           like-for-like number, since the host form is driven through the same binding.  The C call alone is timed by a
           second, bare ctypes call on a third map (its arguments made before the clock starts).
  host     what a resident-map caller had to do before: the old set and the sources from its own copy of the graph (here:
           the restatement's, NOT timed), the inliers as edits, then per window key frame that is not old one
           rs_map_match(n_only) from a kept rs_frame — which re-flattens and re-uploads the map after the previous frame's
           edits — and the frame's edits through rs_map_add_observation / rs_map_fuse_points.  The edits are driven from
           Python, one ctypes call per entry (a few hundred per frame): that overhead is part of the host number and is also
           reported on its own (host_form_edits_ms); the walk over the caller's own objects that decides each entry is not
           timed (the outcomes are taken from the device journal).

Both forms are checked to leave the same map (counts, and the journal entries of the device form are what the host form's
matches were).  Nothing is promised: the JSON records what was found, including a device form that loses.

    python tools/loop_fuse_time.py [--reps 7] [--warmup 2] [--json profiles/loop_fuse_time.json]
"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def build_map(ctx, rs, model, keep_frames=()):
    m, frames = rs.ResidentMap(ctx), {}
    for kf in range(model.n_kf()):
        f = rs.ResidentFrame(ctx, model.kf_kp[kf].reshape(-1, 2), model.kf_desc[kf].reshape(-1, 32))
        m.add_keyframe(f, model.kf_pose[kf])
        if kf in keep_frames:
            frames[kf] = f
        else:
            f.close()
    for p in range(model.n_slots()):
        m.add_point(model.pos[p])
        for kf, kp in model.obs[p]:
            m.add_observation(p, kf, kp)
    return m, frames


def bare_call_seconds(rs, ctx, m, query, candidate, inliers, window, cam):
    """wall clock of lib.rs_map_fuse_loop alone, journal wanted"""
    ptr = lambda x: x.ctypes.data_as(C.c_void_p)
    ik, ip = (np.ascontiguousarray([e[k] for e in inliers], np.int32) for k in (0, 1))
    win = np.ascontiguousarray(window, np.int32)
    opt = rs.FuseOptions(width=cam["width"], height=cam["height"], max_distance=64, min_shared=15, max_covisible=20, check=0)
    for i in range(4):
        opt.intrinsics[i] = cam["K"][i]
    rep, n = rs.FuseReport(), C.c_int(0)
    cap = len(ik) + 2000 * len(win)
    sec, jk, jp, jo = np.zeros(len(win) + 2, np.int32), np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(cap, np.int32)
    lib = rs.load()
    ctx.synchronize()
    t0 = time.perf_counter()
    rc = lib.rs_map_fuse_loop(ctx.h, m.h, query, candidate, ptr(ik), ptr(ip), len(ik), ptr(win), len(win), C.byref(opt), C.byref(rep), ptr(sec),
                              ptr(jk), ptr(jp), ptr(jo), cap, C.byref(n))
    t = time.perf_counter() - t0
    assert rc == 0
    return t, n.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    pkg = importlib.import_module("racing-slam_amd")
    rs = pkg.rsgpu
    import fuse_cases
    b, query, inliers, window, info = fuse_cases.loop_scene(77, n_old_kf=8, n_new_kf=20, n_old=1500, dup_frac=0.5, n_kp=2000, pairs=10,
                                                             free_frac=0.1, p_cand=0.7, p_old=0.5, n_new_only=7700, both_frac=0.01)
    c = fuse_cases.case("timing", b, query, 0, inliers, window)
    model, cam = c["model"], c["camera"]
    ctx = rs.Context(0)
    dev, call, host, edits, journal, counts = [], [], [], [], None, None
    for rep in range(a.warmup + a.reps):
        # ---- device form
        m, _ = build_map(ctx, rs, model)
        f0 = rs.ResidentFrame(ctx, model.kf_kp[0].reshape(-1, 2), model.kf_desc[0].reshape(-1, 32))
        m.match(f0, model.kf_pose[0], cam["K"], cam["width"], cam["height"])        # the image is current, as after loop verification
        ctx.synchronize()
        t0 = time.perf_counter()
        got = m.fuse_loop(query, 0, inliers, window, cam["K"], cam["width"], cam["height"], capacity=len(inliers) + 2000 * len(window))
        t_dev = time.perf_counter() - t0
        cd = m.counts()
        m.close()
        # ---- the C call alone, on a map of its own
        m, _ = build_map(ctx, rs, model)
        m.match(f0, model.kf_pose[0], cam["K"], cam["width"], cam["height"])
        t_call, n_bare = bare_call_seconds(rs, ctx, m, query, 0, inliers, window, cam)
        assert n_bare == got["n_entries"] and m.counts() == cd
        m.close()
        # ---- host form, from the device journal's decisions
        m, frames = build_map(ctx, rs, model, keep_frames=set(window))
        m.match(f0, model.kf_pose[0], cam["K"], cam["width"], cam["height"])
        ctx.synchronize()
        sources = got["sources"]
        old = set(got["old_frames"])
        same, t_edit = True, [0.0]
        t0 = time.perf_counter()

        gone = iter(got["removed"].tolist())       # the discarded point of each fuse, in order (a caller reads its own table)

        def edit(kf, section):
            t1 = time.perf_counter()
            for kp, pt, oc in section:
                if oc == 1:
                    m.add_observation(pt, kf, kp)
                elif oc == 5:
                    m.fuse_points(pt, next(gone))
            t_edit[0] += time.perf_counter() - t1

        edit(query, got["sections"][0])
        for w, kf in enumerate(window):
            if kf in old:
                continue
            seen = [int(p) for p in m.keyframe_matches(kf) if p >= 0]
            mk, mp = m.match(frames[kf], model.kf_pose[kf], cam["K"], cam["width"], cam["height"], matched_points=seen, only_points=sources,
                             replace=1)
            sec = got["sections"][1 + w]
            same = same and mk.tolist() == [e[0] for e in sec] and mp.tolist() == [e[1] for e in sec]
            edit(kf, sec)
        m.match(f0, model.kf_pose[0], cam["K"], cam["width"], cam["height"])        # the re-flatten after the last frame's edits
        t_host = time.perf_counter() - t0
        ch = m.counts()
        for f in frames.values():
            f.close()
        f0.close()
        m.close()
        assert same and ch == cd, "the two forms disagree"
        if rep >= a.warmup:
            dev.append(t_dev)
            call.append(t_call)
            host.append(t_host)
            edits.append(t_edit[0])
        journal, counts = got, cd
    res = dict(reps=a.reps, warmup=a.warmup,
               shape=dict(window=len(window), keypoints=2000, key_frames=model.n_kf(), points=model.n_slots(), observations=model.counts()["observations"],
                          sources=int(len(journal["sources"])), old_frames=len(journal["old_frames"]), entries=journal["n_entries"],
                          outcomes=journal["outcomes"], after=counts),
               device_form_ms=dict(median=round(1e3 * float(np.median(dev)), 3), min=round(1e3 * min(dev), 3)),
               host_form_ms=dict(median=round(1e3 * float(np.median(host)), 3), min=round(1e3 * min(host), 3)),
               host_form_edits_ms=dict(median=round(1e3 * float(np.median(edits)), 3), min=round(1e3 * min(edits), 3)),
               device_c_call_alone_ms=dict(median=round(1e3 * float(np.median(call)), 3), min=round(1e3 * min(call), 3)),
               note="device_form and host_form both go through the Python binding; host form: rs_map_match(n_only) per window frame + "
                    "edits driven from Python (one ctypes call per entry: host_form_edits_ms of host_form_ms); the caller's own graph "
                    "walk that decides each entry is not included")
    ctx.close()
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as fo:
            json.dump(res, fo, indent=1)


if __name__ == "__main__":
    main()
