#!/usr/bin/env python3
"""GPU time of the relative-pose stage (csrc/pose.hip) by HIP events on the context stream, median / min of --reps
after --warmup:
  fixed_1000      rs_estimate_pose, n = 2000, 1000 hypotheses with no early stop (confidence 1 - 1e-12, 60 % outliers)
  adaptive_30     rs_estimate_pose, n = 2000 at 30 % outliers, confidence 0.99 (the adaptive stop after round one)
  known_rotation  rs_estimate_pose_known_rotation, n = 2000, 200 pairs
  chain           rs_track_features -> rs_detect_features -> rs_describe_features -> rs_estimate_pose at 1920x1080
                  with 2000 points (synth.make_klt_pair(2)) and no host synchronisation in between

    python tools/pose_time.py [--reps 50] [--warmup 5] [--json out.json]
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    pkg = importlib.import_module("racing-slam_amd")
    rs, synth = pkg.rsgpu, pkg.synth
    ctx = rs.Context(0)
    est = ctx.pose_estimator(8192, 1000)
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

    res = dict(reps=a.reps)
    for name, frac, conf in (("fixed_1000", 0.6, 1.0 - 1e-12), ("adaptive_30", 0.3, 0.99)):
        d = synth.make_pose_pair(0, 2000, frac, 0.5, "forward")
        pf, pt, cnt = ctx.dev(d["pts_from"]), ctx.dev(d["pts_to"]), ctx.dev(np.array([2000], np.int32))
        out = ctx.estimate_pose(est, pf, pt, cnt, 2000, d["K"], confidence=conf)
        res[name] = timed(lambda: ctx.estimate_pose(est, pf, pt, cnt, 2000, d["K"], confidence=conf, out=out))
        res[name].update(drawn=est.stats()["drawn"])
        if name == "adaptive_30":
            pairs = ctx.dev(np.random.default_rng(0).integers(0, 2000, (200, 2)).astype(np.int32))
            kr = ctx.estimate_pose_known_rotation(est, pf, pt, 2000, d["K"], d["R"], pairs, 200)
            res["known_rotation"] = timed(lambda: ctx.estimate_pose_known_rotation(est, pf, pt, 2000, d["K"], d["R"], pairs,
                                                                                   200, out=kr))
    d = synth.make_klt_pair(2)
    W, H, n = d["width"], d["height"], len(d["pts"])
    im1, im2 = ctx.image(W, H, frame=d["img1"]), ctx.image(W, H, frame=d["img2"])
    det, ds = ctx.detector(W, H, 3000), ctx.describer(W, H, 8192)
    d_pts, d_mask = ctx.dev(d["pts"]), ctx.dev(d["mask"])
    prev_desc = ctx.describe_features(ds, im1, d_pts, ctx.dev(np.array([n], np.int32)))["desc"].clone()
    K = np.array([1000.0, 1000.0, W / 2.0, H / 2.0], np.float32)
    out_f = ctx.track_features(im1, im2, d_pts, n, d_mask=d_mask)
    out_d = ctx.detect_features(det, im2, d_mask, out_f["pts"], out_f["count"], max_total=2000)
    out_o = ctx.describe_features(ds, im2, out_f["pts"], out_f["count"], out_f["index"], prev_desc, n, out_d["pts"],
                                  out_d["counts"][1:])
    out_p = ctx.estimate_pose(est, d_pts, out_f["pts"], out_f["count"], n, K, d_from_index=out_f["index"])

    def chain():
        ctx.track_features(im1, im2, d_pts, n, d_mask=d_mask, out=out_f)
        ctx.detect_features(det, im2, d_mask, out_f["pts"], out_f["count"], max_total=2000, out=out_d)
        ctx.describe_features(ds, im2, out_f["pts"], out_f["count"], out_f["index"], prev_desc, n, out_d["pts"],
                              out_d["counts"][1:], out=out_o)
        ctx.estimate_pose(est, d_pts, out_f["pts"], out_f["count"], n, K, d_from_index=out_f["index"], out=out_p)

    res["chain"] = timed(chain)
    res["chain"].update(tracked=int(out_f["count"].cpu()[0]), drawn=est.stats()["drawn"],
                        inliers=int(out_p["inlier_count"].cpu()[0]))
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    for x in (im1, im2, det, ds, est):
        x.close()
    ctx.close()


if __name__ == "__main__":
    main()
