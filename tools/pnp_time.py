#!/usr/bin/env python3
"""GPU time of the absolute-pose stage (csrc/pnp.hip) by HIP events on the context stream, median / min of --reps after
--warmup, for n = 100, 300 and 2000 correspondences at 30 % outliers and 0.5 px noise:
  ref_200_n<n>        rs_estimate_pose_pnp with 200 hypotheses (the reference's call: one round, no adaptive stop inside it)
  adaptive_1000_n<n>  up to 1000 hypotheses, confidence 0.99 (the adaptive stop after round one)
  fixed_1000_n2000    n = 2000 at 60 % outliers, confidence 1 - 1e-12: all four rounds
  chain               rs_match_descriptors -> rs_estimate_pose_pnp on 1500 descriptor rows, the match lists and the count
                      staying on the device (synth.make_pnp_scene(descriptors=True)); match alone for the difference
Per-kernel totals of the library's own event brackets (rs_prof_begin / rs_prof_end) over 20 calls of ref_200_n2000 are
added as "kernels".  No CPU time of cv::solvePnPRansac exists to compare with.

    python tools/pnp_time.py [--reps 50] [--warmup 5] [--json out.json]
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
    est = ctx.pnp_estimator(8192, 1000)
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

    def case(name, n, frac, hyp, conf):
        d = synth.make_pnp_scene(0, n, frac, 0.5, "volume")
        obj, pix, cnt = ctx.dev(d["points"]), ctx.dev(d["pixels"]), ctx.dev(np.array([n], np.int32))
        out = ctx.estimate_pose_pnp(est, obj, pix, cnt, n, d["K"], max_hypotheses=hyp, confidence=conf)
        fn = lambda: ctx.estimate_pose_pnp(est, obj, pix, cnt, n, d["K"], max_hypotheses=hyp, confidence=conf, out=out)   # noqa: E731
        res[name] = timed(fn)
        st = est.stats()
        res[name].update(drawn=st["drawn"], inliers=st["inliers"], refit_kept=st["refit_kept"])
        return fn

    fn2000 = None
    for n in (100, 300, 2000):
        f = case(f"ref_200_n{n}", n, 0.3, 200, 0.99)
        fn2000 = f if n == 2000 else fn2000
        case(f"adaptive_1000_n{n}", n, 0.3, 1000, 0.99)
    case("fixed_1000_n2000", 2000, 0.6, 1000, 1.0 - 1e-12)

    d = synth.make_pnp_scene(6, 1500, 0.3, 0.5, "volume", descriptors=True)
    n = 1500
    dq, dt, obj, pix = ctx.dev(d["desc_pixels"]), ctx.dev(d["desc_points"]), ctx.dev(d["points"]), ctx.dev(d["pixels"])
    m = ctx.match_descriptors(dq, dt, n, n)
    out = ctx.estimate_pose_pnp(est, obj, pix, m["cnt"], n, d["K"], d_object_index=m["mt"], d_pixel_index=m["mq"])

    def chain():
        ctx.match_descriptors(dq, dt, n, n, out=m)
        ctx.estimate_pose_pnp(est, obj, pix, m["cnt"], n, d["K"], d_object_index=m["mt"], d_pixel_index=m["mq"], out=out)

    res["chain"] = timed(chain)
    res["chain"].update(matches=int(m["cnt"].cpu()[0]), drawn=est.stats()["drawn"], inliers=int(out["inlier_count"].cpu()[0]))
    res["chain_match_only"] = timed(lambda: ctx.match_descriptors(dq, dt, n, n, out=m))

    ctx.prof_begin()
    for _ in range(20):
        fn2000()
    res["kernels"] = {k: round(1e3 * v[1] / 20, 2) for k, v in ctx.prof_end().items() if k.startswith("PNP")}
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    est.close()
    ctx.close()


if __name__ == "__main__":
    main()
