#!/usr/bin/env python3
"""GPU time of the description stage (csrc/orb.hip) at 1920x1080 with 2000 tracked points (synth.make_klt_pair(2)), by
HIP events on the context stream: rs_describe_features alone (the tracked points of frame 2 with their carried rows,
then the appended corners), rs_orb_blur alone, and rs_track_features -> rs_detect_features -> rs_describe_features
with no host synchronisation in between (the per-frame front end of Tracker::track_features, src/Tracker.cpp:107-150).
Median / min of --reps after --warmup.

    python tools/orb_time.py [--reps 200] [--warmup 20] [--json out.json]
For the per-kernel split run it under `rocprofv3 --kernel-trace --stats -- python tools/orb_time.py --reps 50`.
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
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--config", type=int, default=2)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    pkg = importlib.import_module("racing-slam_amd")
    rs, synth = pkg.rsgpu, pkg.synth
    ctx = rs.Context(0)
    d = synth.make_klt_pair(a.config)
    W, H, n = d["width"], d["height"], len(d["pts"])
    im1, im2 = ctx.image(W, H, frame=d["img1"]), ctx.image(W, H, frame=d["img2"])
    det, ds = ctx.detector(W, H, 3000), ctx.describer(W, H, 8192)
    d_pts, d_mask = ctx.dev(d["pts"]), ctx.dev(d["mask"])
    prev = ctx.describe_features(ds, im1, d_pts, ctx.dev(np.array([n], np.int32)))
    prev_desc = prev["desc"].clone()
    out_f = ctx.track_features(im1, im2, d_pts, n, d_mask=d_mask)
    out_d = ctx.detect_features(det, im2, d_mask, out_f["pts"], out_f["count"], max_total=2000)
    cnt_b = out_d["counts"][1:]
    out_o = ctx.describe_features(ds, im2, out_f["pts"], out_f["count"], out_f["index"], prev_desc, n, out_d["pts"], cnt_b)
    plane = ctx.orb_blur(ds, im2)
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

    def describe():
        ctx.describe_features(ds, im2, out_f["pts"], out_f["count"], out_f["index"], prev_desc, n, out_d["pts"], cnt_b, out=out_o)

    def track_detect_describe():
        ctx.track_features(im1, im2, d_pts, n, d_mask=d_mask, out=out_f)
        ctx.detect_features(det, im2, d_mask, out_f["pts"], out_f["count"], max_total=2000, out=out_d)
        describe()

    res = dict(width=W, height=H, points=n, reps=a.reps,
               orb_blur=timed(lambda: ctx.orb_blur(ds, im2, out=plane)),
               describe_features=timed(describe),
               track_detect_describe=timed(track_detect_describe))
    fresh = out_o["fresh"].cpu().numpy()
    total = int(out_o["n"].cpu()[0])
    res.update(tracked=int(out_f["count"].cpu()[0]), appended=int(out_d["counts"].cpu()[1]), described=total,
               fresh=int(fresh[:total].sum()))
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    for x in (im1, im2, det, ds):
        x.close()
    ctx.close()


if __name__ == "__main__":
    main()
