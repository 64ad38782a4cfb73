#!/usr/bin/env python3
"""GPU time of the KLT stage (csrc/klt.hip) at 1920x1080 with 2000 points (synth.make_klt_pair(2)), by HIP events on the
context stream: upload + pyramid of one grey frame from pageable host memory (and from device memory), rs_klt_track
forward only, rs_track_features (forward + backward + filter + compaction).  Median / min of --reps after --warmup.

    python tools/klt_time.py [--reps 200] [--warmup 20] [--json out.json]
For the per-kernel split run it under `rocprofv3 --kernel-trace --stats -- python tools/klt_time.py --reps 50`.
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
    scratch = ctx.image(W, H)
    d_pts, d_mask, d_img = ctx.dev(d["pts"]), ctx.dev(d["mask"]), ctx.dev(d["img2"])
    out_t = ctx.klt_track(im1, im2, d_pts, n)
    out_f = ctx.track_features(im1, im2, d_pts, n, d_mask=d_mask)
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

    res = dict(width=W, height=H, points=n, reps=a.reps,
               upload_pyramid_host=timed(lambda: scratch.upload(d["img2"])),
               upload_pyramid_device=timed(lambda: scratch.upload(d_img)),
               klt_track_forward=timed(lambda: ctx.klt_track(im1, im2, d_pts, n, out=out_t)),
               track_features=timed(lambda: ctx.track_features(im1, im2, d_pts, n, d_mask=d_mask, out=out_f)))
    res["kept"] = int(out_f["count"].cpu()[0])
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    for im in (im1, im2, scratch):
        im.close()
    ctx.close()


if __name__ == "__main__":
    main()
