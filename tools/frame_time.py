#!/usr/bin/env python3
"""Time of making an rs_frame from what the front end leaves on the device (csrc/frame.hip), with 1920x1080-like
keypoints at n = 2000 and n = 8192, in one run on one GPU.  Median / min of --reps after --warmup.

  (a) assign_device     rs_frame_assign_device: gather + ranks + KD build and pack + the 4-byte read-back.  It ends in a
                        host synchronisation, so wall clock and HIP events bracket the same work; both are given.
  (b) host_round_trip   the path it replaces: download of the two keypoint lists, their counts and the descriptor rows,
                        rs_frame_create (rs_kdtree_build on the CPU, five allocations, four uploads, a synchronisation)
                        and rs_frame_destroy.  Wall clock.
                        This is the PYTHON form of the round trip (five torch .cpu() transfers, slicing, a numpy
                        concatenate), so it carries interpreter overhead that a C caller's three hipMemcpy calls would
                        not, while (a) is one ctypes call: read (a) < (b), not the ratio.
  (c) kernels           mean device time of each of the three kernels, from the library's own event brackets
                        (rs_prof_begin / rs_prof_end), KF_frame_build being the KD kernel alone.
  (d) chain             rs_track_features -> rs_detect_features -> rs_describe_features -> rs_frame_assign_device ->
                        rs_map_match on synth.make_klt_pair(2), wall clock, with the same chain through the host round
                        trip beside it.

    python tools/frame_time.py [--reps 200] [--warmup 20] [--json profiles/frame_time.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    pkg = importlib.import_module("racing-slam_amd")
    rs, synth = pkg.rsgpu, pkg.synth
    ctx = rs.Context(0)
    stream = torch.cuda.current_stream()

    def stat(ts):
        ts = sorted(ts)
        return dict(median_us=round(ts[len(ts) // 2], 1), min_us=round(ts[0], 1))

    def wall(fn):
        for _ in range(a.warmup):
            fn()
        ts = []
        for _ in range(a.reps):
            ctx.synchronize()
            t0 = time.perf_counter()
            fn()
            ts.append(1e6 * (time.perf_counter() - t0))
        return stat(ts)

    def events(fn):
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
        return stat(ts)

    res = dict(reps=a.reps, warmup=a.warmup, sizes={})
    rng = np.random.default_rng(0)
    for n in (2000, 8192):
        na = (3 * n) // 4                                    # tracked points, then appended corners
        kp = (rng.uniform(0, 1, (n, 2)) * [1920, 1080]).astype(np.float32)
        desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        d_a, d_b, d_desc = ctx.dev(kp[:na]), ctx.dev(kp[na:]), ctx.dev(desc)
        d_ca, d_cb = ctx.dev(np.array([na], np.int32)), ctx.dev(np.array([n - na], np.int32))
        f = rs.DeviceFrame(ctx, 8192)

        def assign():
            f.assign(d_desc, d_a, d_ca, d_b, d_cb)

        def round_trip():
            ca, cb = int(d_ca.cpu()[0]), int(d_cb.cpu()[0])
            h_kp = np.concatenate([d_a[:ca].cpu().numpy(), d_b[:cb].cpu().numpy()])
            h_desc = d_desc[:ca + cb].cpu().numpy()
            rs.ResidentFrame(ctx, h_kp, h_desc).close()

        r = dict(assign_device_wall=wall(assign), assign_device_events=events(assign), host_round_trip_wall=wall(round_trip))
        ctx.prof_begin()
        for _ in range(a.reps):
            assign()
        prof = ctx.prof_end()
        r["kernels_mean_us"] = {k: round(1e3 * ms / max(cnt, 1), 1) for k, (cnt, ms) in prof.items() if k.startswith("KF_")}
        # what was timed is right
        hf = rs.ResidentFrame(ctx, kp, desc)
        x, y = f.download(), hf.download()
        r["equal_to_host_frame"] = all(np.array_equal(x[k], y[k]) for k in ("kp", "desc", "kd", "packed")) and x["n"] == y["n"] == n
        hf.close()
        f.close()
        res["sizes"][str(n)] = r

    # (d) the front end into a match
    p = synth.make_klt_pair(2)
    W, H, n = p["width"], p["height"], len(p["pts"])
    im1, im2 = ctx.image(W, H, frame=p["img1"]), ctx.image(W, H, frame=p["img2"])
    det, ds = ctx.detector(W, H, 3000), ctx.describer(W, H, 8192)
    d_pts, d_mask = ctx.dev(p["pts"]), ctx.dev(p["mask"])
    prev = ctx.describe_features(ds, im1, d_pts, ctx.dev(np.array([n], np.int32)))
    prev_desc = prev["desc"].clone()
    out_f = ctx.track_features(im1, im2, d_pts, n, d_mask=d_mask)
    out_d = ctx.detect_features(det, im2, d_mask, out_f["pts"], out_f["count"], max_total=2000)
    cnt_b = out_d["counts"][1:]
    out_o = ctx.describe_features(ds, im2, out_f["pts"], out_f["count"], out_f["index"], prev_desc, n, out_d["pts"], cnt_b)
    f = rs.DeviceFrame(ctx, 8192)
    nf = f.assign(out_o["desc"], out_f["pts"], out_f["count"], out_d["pts"], cnt_b)
    h = f.download()
    K = (1000.0, 1000.0, W / 2.0, H / 2.0)
    T = np.eye(4, dtype=np.float32)
    mp = rs.ResidentMap(ctx)
    kf = mp.add_keyframe(f, T)
    for i in range(0, nf, 2):                                # ~1000 points down the rays of the frame's own keypoints
        pt = mp.add_point([(h["kp"][i, 0] - K[2]) / K[0] * 5.0, (h["kp"][i, 1] - K[3]) / K[1] * 5.0, 5.0])
        mp.add_observation(pt, kf, i)
    T2 = T.copy()
    T2[0, 3] = 0.01

    def front():
        ctx.track_features(im1, im2, d_pts, n, d_mask=d_mask, out=out_f)
        ctx.detect_features(det, im2, d_mask, out_f["pts"], out_f["count"], max_total=2000, out=out_d)
        ctx.describe_features(ds, im2, out_f["pts"], out_f["count"], out_f["index"], prev_desc, n, out_d["pts"], cnt_b, out=out_o)

    got = {}

    def chain_device():
        front()
        f.assign(out_o["desc"], out_f["pts"], out_f["count"], out_d["pts"], cnt_b)
        got["device"] = mp.match(f, T2, K, W, H)

    def chain_host():
        front()
        ca, cb = int(out_f["count"].cpu()[0]), int(cnt_b.cpu()[0])
        h_kp = np.concatenate([out_f["pts"][:ca].cpu().numpy(), out_d["pts"][:cb].cpu().numpy()])
        hf = rs.ResidentFrame(ctx, h_kp, out_o["desc"][:ca + cb].cpu().numpy())
        got["host"] = mp.match(hf, T2, K, W, H)
        hf.close()

    res["chain"] = dict(width=W, height=H, keypoints=nf, map_points=(nf + 1) // 2, device_wall=wall(chain_device),
                        host_round_trip_wall=wall(chain_host), front_end_only_wall=wall(lambda: (front(), ctx.synchronize())))
    res["chain"]["matches"] = int(len(got["device"][0]))
    res["chain"]["equal_matches"] = bool(np.array_equal(got["device"][0], got["host"][0]) and np.array_equal(got["device"][1], got["host"][1]))
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as fo:
            json.dump(res, fo, indent=1)
    for x in (f, mp, im1, im2, det, ds):
        x.close()
    ctx.close()


if __name__ == "__main__":
    main()
