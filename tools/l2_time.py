#!/usr/bin/env python3
"""GPU time of the float-descriptor (L2) matchers (csrc/l2_match.hip) by HIP events on the context stream:
rs_match_descriptors_f32 at 1000 x 1000 x 128, 2000 x 2000 x 256 and 64 batched pairs of 2000 x 2000 x 256,
rs_reproj_match_l2 on tests/match_cases.scene(2000, 10000) with 256-float rows, and rs_match_descriptors (u8) at
2000 x 2000 from the same run as context.  Median / min of --reps after --warmup; for the brute-force search also
2 nq nt dim / t as a fraction of the 157.3 TF f32 matrix peak (the arithmetic floor at 2000 x 2000 x 256 is 13 us).

    python tools/l2_time.py [--reps 100] [--warmup 10] [--json profiles/l2_time.json]
For the per-kernel split run it under `rocprofv3 --kernel-trace --stats -- python tools/l2_time.py --reps 20`.
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
PEAK_TF = 157.3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    pkg = importlib.import_module("racing-slam_amd")
    rs = pkg.rsgpu
    import match_cases as MC
    import match_l2_cases as LC
    ctx = rs.Context(0)
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

    res = dict(reps=a.reps, peak_tf=PEAK_TF)
    for name, nq, nt, dim, batch in (("match_f32_1000x1000x128", 1000, 1000, 128, 1), ("match_f32_2000x2000x256", 2000, 2000, 256, 1),
                                     ("match_f32_64x2000x2000x256", 2000, 2000, 256, 64)):
        g = torch.Generator(device="cpu").manual_seed(nq + dim + batch)
        t = torch.nn.functional.normalize(torch.randn((batch, nt, dim), generator=g), dim=2)
        q = torch.nn.functional.normalize(t[:, torch.randperm(nt, generator=g)[:nq]] + 0.03 * torch.randn((batch, nq, dim), generator=g), dim=2)
        dq, dt = q.contiguous().to(ctx.device), t.contiguous().to(ctx.device)
        out = ctx.match_descriptors_f32(dq, dt, nq, nt, dim, batch=batch, max_distance=0.7)
        r = timed(lambda: ctx.match_descriptors_f32(dq, dt, nq, nt, dim, batch=batch, max_distance=0.7, out=out))
        r["matches"] = int(out["cnt"].sum().cpu())
        r["tf"] = round(2.0 * nq * nt * dim * batch / (r["median_us"] * 1e-6) / 1e12, 2)
        r["fraction_of_peak"] = round(r["tf"] / PEAK_TF, 4)
        res[name] = r
    # the u8 matcher at the same pair count, as context
    rng = np.random.default_rng(0)
    q8, t8 = MC.knn_set(2000, 2000, seed=1)
    d8q, d8t = ctx.dev(q8), ctx.dev(t8)
    out8 = ctx.match_descriptors(d8q, d8t, 2000, 2000)
    res["match_u8_2000x2000"] = timed(lambda: ctx.match_descriptors(d8q, d8t, 2000, 2000, out=out8))
    # the reprojection matcher
    frame, mp = MC.scene(2000, 10000, kdtree_build=rs.kdtree_build)
    fdesc, pool = LC.attach(frame, mp, 256, seed=int(rng.integers(1 << 20)))
    fv, k1 = ctx.make_frame_view(frame, pack=True)
    mv, k2 = ctx.make_map_view(mp)
    df, dp = ctx.dev(fdesc), ctx.dev(pool)
    o = ctx.reproj_match_l2(fv, mv, df, dp, 256, max_distance=1.0)
    r = timed(lambda: ctx.reproj_match_l2(fv, mv, df, dp, 256, max_distance=1.0, out=o))
    r["matches"] = int(o["count"].cpu()[0])
    res["reproj_l2_N2000_P10000_d256"] = r
    o8 = ctx.reproj_match(fv, mv)
    res["reproj_u8_N2000_P10000"] = timed(lambda: ctx.reproj_match(fv, mv, out=o8))
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
