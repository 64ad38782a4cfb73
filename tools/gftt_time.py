#!/usr/bin/env python3
"""GPU time of the replenishment stage (csrc/gftt.hip) at 1920x1080 with 2000 tracked points (synth.make_klt_pair(2)), by
HIP events on the context stream: rs_detect_features alone (the tracked points of frame 2 excluded), rs_corner_response
alone, rs_track_features followed by rs_detect_features with no host synchronisation in between (the per-frame front
end of Tracker::track_features, src/Tracker.cpp:107-146), and the same after a host upload + pyramid of frame 2.
Median / min of --reps after --warmup; the detector's diagnostic (candidates, selection rounds) of the last call.

    python tools/gftt_time.py [--reps 200] [--warmup 20] [--json out.json]
For the per-kernel split run it under `rocprofv3 --kernel-trace --stats -- python tools/gftt_time.py --reps 50`.
"""
import argparse
import importlib
import json
import os
import sys

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
    det = ctx.detector(W, H, 3000)
    d_pts, d_mask = ctx.dev(d["pts"]), ctx.dev(d["mask"])
    out_f = ctx.track_features(im1, im2, d_pts, n, d_mask=d_mask)
    out_d = ctx.detect_features(det, im2, d_mask, out_f["pts"], out_f["count"], max_total=2000)
    eig = ctx.corner_response(det, im2)
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

    def detect():
        ctx.detect_features(det, im2, d_mask, out_f["pts"], out_f["count"], max_total=2000, out=out_d)

    def track_detect():
        ctx.track_features(im1, im2, d_pts, n, d_mask=d_mask, out=out_f)
        detect()

    def upload_track_detect():
        im2.upload(d["img2"])
        track_detect()

    res = dict(width=W, height=H, points=n, reps=a.reps,
               corner_response=timed(lambda: ctx.corner_response(det, im2, out=eig)),
               detect_features=timed(detect),
               track_features=timed(lambda: ctx.track_features(im1, im2, d_pts, n, d_mask=d_mask, out=out_f)),
               track_then_detect=timed(track_detect),
               upload_track_detect=timed(upload_track_detect))
    c = out_d["counts"].cpu().tolist()
    res.update(tracked=int(out_f["count"].cpu()[0]), detected=c[0], appended=c[1], detector=det.stats())
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    for x in (im1, im2, det):
        x.close()
    ctx.close()


if __name__ == "__main__":
    main()
