#!/usr/bin/env python3
"""Time of loop verification (csrc/loop.hip) at the workload's shape: a query key frame of 2000 keypoints, 3 candidates
of 2000 keypoints with about 1200 map matches each, 200 hypotheses.  HIP events on the context stream around each
call (the call synchronises once, so host and device time are both inside), median / min of --reps after --warmup:
  (a) rs_map_verify_loop, both issue forms ("loop_verify_streams" 0, forked child contexts, and 1, one stream);
  (b) the same three verifications with what the library offered before it: walk the mirror on the host, gather rows and
      positions, upload, rs_match_descriptors, rs_estimate_pose_pnp, download, verdict on the host — written here;
  (c) key-frame retrieval (rs_bow_transform -> rs_bow_database_score -> read-back -> rs_rank_loop_candidates) followed by
      rs_map_verify_loop of three candidates;
  (d) the two new kernels alone, by the library's profiling brackets.

    python tools/loop_time.py [--reps 200] [--warmup 20] [--json out.json]
For the per-kernel split run it under `rocprofv3 --kernel-trace --stats -- python tools/loop_time.py --reps 50`.
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--points", type=int, default=2000)
    ap.add_argument("--matched", type=int, default=1200)
    ap.add_argument("--shared", type=int, default=500)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    import loop_ref as L
    pkg = importlib.import_module("racing-slam_amd")
    rs, synth = pkg.rsgpu, pkg.synth
    ctx = rs.Context(0)
    n = a.points
    s = synth.loop_scene(0, n, ((n, a.matched, a.shared, 0.3, None),) * 3)
    m = rs.ResidentMap(ctx)
    frames = [rs.ResidentFrame(ctx, k["kp"], k["desc"]) for k in s["key_frames"]]
    for k, f in zip(s["key_frames"], frames):
        m.add_keyframe(f, k["pose"])
    for xyz in s["points"]:
        m.add_point(xyz)
    for p, k, i in s["observations"]:
        m.add_observation(p, k, i)
    K, W, q = s["K"], s["width"], s["query"]
    ver = ctx.loop_verifier(max(n, 1), 3, 200)
    stream = torch.cuda.current_stream()

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        ts = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            ts.append(1e3 * e0.elapsed_time(e1))
        ts.sort()
        return dict(median_us=round(ts[len(ts) // 2], 1), min_us=round(ts[0], 1))

    def resident():
        return ver.verify(m, q, [0, 1, 2], K, W)

    # (b) the host form: the mirror as a caller holds it (kp_point tables, positions, rows on the host)
    kfs, pos = s["key_frames"], s["points"]
    est = ctx.pnp_estimator(max(n, 1), 200)
    d_query, d_qkp = ctx.dev(kfs[q]["desc"]), ctx.dev(kfs[q]["kp"])
    qc = L.centre_of(kfs[q]["pose"])

    def host_form():
        out = []
        for c in range(3):
            kp_point = kfs[c]["kp_point"]
            rows = np.flatnonzero(kp_point >= 0)
            d_train, d_obj = ctx.dev(kfs[c]["desc"][rows]), ctx.dev(pos[kp_point[rows]])
            mt = ctx.match_descriptors(d_query, d_train, n, len(rows))
            cnt = int(mt["cnt"].cpu()[0])
            if cnt < 12:
                out.append(L.finish(1, None, [], mt["mq"].cpu().numpy()[0, :cnt], mt["mt"].cpu().numpy()[0, :cnt],
                                    rows.astype(np.int32), kp_point, kfs[q]["kp"], W, qc, L.centre_of(kfs[c]["pose"])))
                continue
            r = ctx.estimate_pose_pnp(est, d_obj, d_qkp, mt["cnt"], n, K, d_object_index=mt["mt"], d_pixel_index=mt["mq"],
                                      threshold_px=4.0, max_hypotheses=200)
            k = int(r["inlier_count"].cpu()[0])
            inl = r["inlier_index"].cpu().numpy()[:k]
            mq, mtr = mt["mq"].cpu().numpy()[0, :cnt], mt["mt"].cpu().numpy()[0, :cnt]
            status = 0 if (int(r["status"].cpu()[0]) == 0 and k) else 2
            out.append(L.finish(status, r["pose"].cpu().numpy(), inl, mq, mtr, rows.astype(np.int32), kp_point, kfs[q]["kp"], W, qc,
                                L.centre_of(kfs[c]["pose"])))
        return out

    got, want = resident(), host_form()
    assert all(g["status"] == w["status"] and g["ok"] == w["ok"] and g["inliers"] == w["inliers"] for g, w in zip(got, want))
    res = dict(points=n, candidates=3, matched=a.matched, shared=a.shared, hypotheses=200, reps=a.reps,
               correspondences=[g["correspondences"] for g in got], inliers=[g["inliers"] for g in got],
               verify_forked=timed(resident))
    ctx.set_int("loop_verify_streams", 1)
    res["verify_one_stream"] = timed(resident)
    ctx.set_int("loop_verify_streams", 0)
    res["host_gather_upload_two_calls_download"] = timed(host_form)
    # (d) the new kernels alone
    ctx.prof_begin()
    for _ in range(a.reps):
        resident()
    prof = ctx.prof_end()
    for name in ("LOOP0_gather", "LOOP1_verdict"):
        if name in prof:
            res[name + "_mean_us"] = round(1e3 * prof[name][1] / max(prof[name][0], 1), 2)
    # (c) retrieval -> verification: a small vocabulary and 60 entries, three of them the candidates
    vt = synth.make_vocabulary(10, 4)
    voc = ctx.vocabulary(vt["k"], vt["L"], 0, 0, vt["parent"], vt["desc"], vt["weight"])
    bow, db = ctx.bow(voc, 8192), ctx.bow_database(voc, 64, 64 * n)
    d_n = ctx.dev(np.array([n], np.int32))
    for e in range(60):
        rows = kfs[e]["desc"] if e < 3 else synth.make_bow_descriptors(vt, n, seed=e)
        bow.transform(ctx.dev(rows), d_n, n, words=False)
        db.add(bow)
    scores = ctx.empty((60,), torch.float64)
    fi = 10 * np.arange(61, dtype=np.int64)

    def chain():
        bow.transform(d_query, d_n, n, words=False)
        sc = db.score(bow, 0, 60, out=scores).cpu().numpy()
        rs.rank_loop_candidates(sc, fi[:60], fi[60], 1.0 / 30.0)
        return ver.verify(m, q, [0, 1, 2], K, W)                  # (the synthetic rows rank nothing: the candidates are given)

    res["retrieve_then_verify"] = timed(chain)
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    for x in (bow, db, voc, ver, est, m, *frames):
        x.close()
    ctx.close()


if __name__ == "__main__":
    main()
